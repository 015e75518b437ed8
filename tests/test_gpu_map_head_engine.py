"""The attention-pool head in the engine (vit_engine_set_map_head, features(imgs, "map")) against tests/map_head_model.py, the
float64 model of the UNFOLDED head: applied to the live oracle's final-LayerNorm tokens, and to the engine's own
features(imgs, "tokens") -- which isolates the head from the encoder; bitwise across everything the engine promises to keep
bit-identical; the state rules of vit_engine_set_head."""
import numpy as np
import pytest

import map_head_model as M
from engine_helpers import CONFIGS, CONSTS, device_features, engines, same_bits, weights  # noqa: F401 (fixtures)
from test_gpu_features import BF16_BAR, LOGIT_REL, oracle_tokens, rel_err
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

VIT_ERR_ARG, VIT_ERR_STATE = 1, 5
# The head alone, against the model on the engine's own tokens: max |d| / max |ref|.  Measured on an MI355X (profiles/r35/map_head.md):
# 3.3e-7 .. 6.5e-7 over the ten cases below, the largest on the fp32 tiny engine with 2 heads and GELU.  Four times the largest,
# rounded up to one digit; the rule's ceiling of 1e-4 is far away.
OWN_TOKENS_BAR = 3e-6
REG4_TINY = synth.ModelConfig(img_size=56, patch_size=14, num_classes=10, embed_dim=128, depth=2, num_heads=2, hidden_dim=256,
                              num_register_tokens=4)  # synth.DINOV2_B14_REG4's geometry at the tiny model's size: first = 5


def install(eng, heads, hidden, act="gelu", prefix=False, seed=77):
    w = synth.make_map_head(eng.cfg.embed_dim, heads, hidden, seed)
    eng.set_map_head(B.map_head_spec(heads, hidden, act, prefix), w)
    return w


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name,heads,act,prefix", [("tiny", 2, "gelu", False), ("tiny", 4, "gelu_tanh", True), ("small", 3, "gelu_tanh", False),
                                                   ("small", 6, "gelu", True), ("reg4", 2, "gelu_tanh", False)])
def test_map_rows_match_the_model_on_the_oracles_tokens_and_on_the_engines_own(oracle, name, heads, act, prefix, dtype):
    cfg = REG4_TINY if name == "reg4" else CONFIGS[name]
    W, imgs = synth.make_weights(cfg, 21), synth.make_images(cfg, 5, 105)
    eng = B.Engine(cfg, max_batch=4, dtype=dtype)
    try:
        eng.load_weights(W)
        w = install(eng, heads, 2 * cfg.embed_dim, act, prefix)
        first = 0 if prefix else cfg.tokens - cfg.patches
        got = eng.features(imgs, "map")
        assert got.shape == (5, cfg.embed_dim)
        if name != "reg4":  # the oracle knows no register tokens
            err = rel_err(got, M.head(oracle_tokens(oracle, cfg, imgs, W)[:, first:], w, heads, act))
            print(f"{dtype} {name} vs oracle tokens: {err:.3e}")
            assert err <= (LOGIT_REL if dtype == "f32" else BF16_BAR["mean"])
        err = rel_err(got, M.head(eng.features(imgs, "tokens")[:, first:], w, heads, act))
        print(f"{dtype} {name} heads={heads} {act} vs own tokens: {err:.3e}")
        assert err <= OWN_TOKENS_BAR
        l2 = eng.features(imgs, "map", True)
        assert np.abs(np.linalg.norm(l2.astype(np.float64), axis=1) - 1.0).max() <= 1e-5
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_same_bits_across_input_paths_lanes_pruning_batch_places_and_graph_replays(engines, dtype):
    cfg, n = CONFIGS["small"], 9
    rng = np.random.default_rng(5)
    u8 = rng.integers(0, 256, (n, cfg.img_size, cfg.img_size, 3), np.uint8)
    imgs = B.images_u8_to_f32(u8)
    d_f, d_u = B.DeviceArray.from_numpy(imgs), B.DeviceArray.from_numpy(u8)
    recs = [(d_u.ptr + i * u8[0].nbytes, cfg.img_size, cfg.img_size) for i in range(n)]
    eng = engines("small", max_batch=4, dtype=dtype)
    install(eng, 3, 384, "gelu_tanh")
    try:
        want = eng.features(imgs, "map")
        assert same_bits(eng.features_u8(u8, "map", False, *CONSTS), want)
        assert same_bits(eng.features_images(list(u8), cfg.img_size, "map", False, *CONSTS), want)
        assert same_bits(device_features(eng, d_f, n, "map"), want) and same_bits(device_features(eng, d_u, n, "map", u8=True), want)
        d_o = B.DeviceArray((n, cfg.embed_dim))
        eng.features_device_images(recs, d_o.ptr, cfg.img_size, "map", False, *CONSTS)
        eng.sync()
        assert same_bits(d_o.numpy(), want)
        for i in (0, 4, 8):  # alone, and first / last of a chunk
            assert same_bits(eng.features(imgs[i:i + 1], "map")[0], want[i]), i
        eng.set_lanes(2)
        assert same_bits(eng.features(imgs, "map"), want)
        eng.set_lanes(1)
        for opt in (dict(prune_last_layer=True), dict(use_graph=True)):
            other = engines("small", max_batch=4, dtype=dtype, **opt)
            install(other, 3, 384, "gelu_tanh")
            for _ in range(3):  # the capture, then replays
                assert same_bits(device_features(other, d_f, 4, "map"), want[:4]), opt
            other.reset_map_head()
    finally:
        eng.set_lanes(1)
        eng.reset_map_head()


def test_state_and_refusals_leave_the_previous_head_in_force(engines, weights):
    cfg = CONFIGS["tiny"]
    eng = engines("tiny", max_batch=4)
    imgs = synth.make_images(cfg, 3, 9)
    d_f, d_o = B.DeviceArray.from_numpy(imgs), B.DeviceArray((3, cfg.embed_dim))
    fresh = B.Engine(cfg, max_batch=4)
    with pytest.raises(B.VitError) as err:
        install(fresh, 2, 0)
    assert err.value.code == VIT_ERR_STATE  # before weights are loaded
    fresh.close()

    def no_head():
        with pytest.raises(B.VitError) as err:
            eng.features_device(d_f.ptr, 3, d_o.ptr, "map")
        return err.value.code == VIT_ERR_ARG  # the kind stays an unknown one, as tests/test_gpu_features.py has always seen 5

    assert no_head()
    w = install(eng, 2, 256)
    want = eng.features(imgs, "map")
    with pytest.raises(B.VitError):
        eng.logits(3)  # nothing wrote logits
    bad_specs = [B.map_head_spec(0, 256), B.map_head_spec(33, 256), B.map_head_spec(3, 256), B.map_head_spec(2, 100),
                 B.map_head_spec(2, 256, 2), B.map_head_spec(2, 256, reserved=1)]
    for spec, ws in [(s, w) for s in bad_specs] + [(B.map_head_spec(2, 256), {k: v for k, v in w.items() if k != name})
                                                   for name in ("probe", "in_proj_bias", "out_proj_weight", "ln_bias", "fc2_weight")]:
        with pytest.raises(B.VitError) as err:
            eng.set_map_head(spec, ws)
        assert err.value.code == VIT_ERR_ARG and same_bits(eng.features(imgs, "map"), want)
    eng.set_map_head(B.map_head_spec(2, 0), {k: v for k, v in w.items() if k in B.MAP_HEAD_TENSORS[:5]})  # hidden_dim = 0: out = a
    a = eng.features(imgs, "map")
    first = cfg.tokens - cfg.patches
    err = rel_err(a, M.head(eng.features(imgs, "tokens")[:, first:], {k: w[k] for k in B.MAP_HEAD_TENSORS[:5]}, 2))
    print(f"hidden_dim = 0 vs own tokens: {err:.3e}")
    assert err <= OWN_TOKENS_BAR
    eng.reset_map_head()
    assert no_head()
    install(eng, 2, 256)
    eng.load_weights(weights("tiny", 1234))  # every install removes the head
    assert no_head()
