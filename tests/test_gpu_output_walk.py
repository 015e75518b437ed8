"""The one layer walk of the engine (forward_chunk, host/vit_engine.c), output kind by output kind: the encoder layers a call
launches are exactly those up to the deepest one its kind needs (the kind's last_layer in OUT_KINDS), whatever runs behind them.

Every expected count is derived here from cfg.depth, the lanes in use and the kind.  With `profile` on, the engine counts a launch
per stage bracket; an unpruned encoder layer has one bracket per lane in each of qkv, attn, outproj, fc1 and fc2 (GELU model).  A
chunk of fewer than 2 * lanes images runs on one lane (chunk_setup), so 3 images use one lane on either engine and 4 use them all.
"""
import numpy as np
import pytest

from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

CFG = synth.VIT_TINY
ENCODER = ("qkv", "attn", "outproj", "fc1", "fc2")
CLASSES = 21
SEED = 261


@pytest.fixture(scope="module")
def engines():
    weights = synth.make_weights(CFG, SEED)
    made = {}
    for dtype in ("f32", "bf16"):
        for lanes in (1, 2):
            made[dtype, lanes] = B.Engine(CFG, max_batch=4, dtype=dtype, lanes=lanes, profile=True)
            made[dtype, lanes].load_weights(weights)
    yield made
    for eng in made.values():
        eng.close()


def dense_head(layers):
    F = len(layers) * CFG.embed_dim
    rng = np.random.default_rng(F)
    return (rng.standard_normal((CLASSES, F)) / np.sqrt(F)).astype(np.float32), rng.standard_normal(CLASSES).astype(np.float32)


def encoder_launches(eng, n, call):
    eng.reset_stage_times()
    call()
    t = eng.stage_times()
    assert t["images"] == n
    return {s: t["stages"][s]["launches"] for s in ENCODER}


@pytest.mark.parametrize("n", [3, 4])
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_every_kind_launches_the_layers_up_to_its_last_and_no_other(engines, dtype, lanes, n):
    eng, depth = engines[dtype, lanes], CFG.depth
    imgs = synth.make_images(CFG, n, SEED + n)
    used = lanes if n >= 2 * lanes else 1
    assert len(eng.pool_scratch_layout(n)) == used

    def layers_worth(layers, behind_qkv=None):
        """`layers` encoder layers; behind_qkv: the layers that run past their QKV GEMM, where those are fewer"""
        rest = layers if behind_qkv is None else behind_qkv
        return {s: (layers if s == "qkv" else rest) * used for s in ENCODER}

    full = layers_worth(depth)
    calls = [("forward", lambda: eng.forward(imgs), full), ("topk", lambda: eng.topk_host(imgs, 3), full)]
    calls += [(f"features {k}", lambda k=k: eng.features(imgs, k), full) for k in ("cls", "mean", "tokens", "head")]
    # the class token's attention is read from Q and K of the last layer: its QKV GEMM runs, nothing of the layer behind it -- and
    # the kind's own stage behind the walk is one launch per lane that the engine accounts to `attn` (stage_cls_attention)
    attention = dict(layers_worth(depth, depth - 1), attn=(depth - 1) * used + used)
    calls += [(f"attention {k}", lambda k=k: eng.cls_attention(imgs, k), attention) for k in ("heads", "head_mean")]
    calls += [(f"intermediate {k} [0]", lambda k=k: eng.intermediate(imgs, [0], k, 1), layers_worth(1)) for k in ("cls", "tokens", "patches", "map")]
    calls += [("intermediate cls [depth-1]", lambda: eng.intermediate(imgs, [depth - 1], "cls", 1), full)]
    for name, call, want in calls:
        assert encoder_launches(eng, n, call) == want, (name, want)
    # a dense call runs the layers of the head in force, whatever its spec asks for
    try:
        for layers in ([0, 1], [0]):
            eng.set_dense_head(*dense_head(layers), layers, 1)
            for kind in ("labels", "grid"):
                assert encoder_launches(eng, n, lambda: eng.dense(imgs, kind)) == layers_worth(layers[-1] + 1), (layers, kind)
    finally:
        eng.reset_dense_head()


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_the_normalised_cls_tap_of_the_last_layer_is_the_cls_feature_row(engines, dtype, lanes):
    eng = engines[dtype, lanes]
    for n in (3, 4):
        imgs = synth.make_images(CFG, n, SEED + n)
        tap = eng.intermediate(imgs, [CFG.depth - 1], "cls", 1).reshape(n, -1)
        feat = eng.features(imgs, "cls")
        assert tap.shape == feat.shape == (n, CFG.embed_dim)
        assert np.array_equal(tap.view(np.uint32), feat.view(np.uint32))
