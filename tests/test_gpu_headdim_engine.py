"""Engines at head dims 72, 80, 104 and 128 -- the attention launches of the layer sequence and the class-token attention stage go
through the _hd entries (csrc/vit_attention_hd.hip), the bf16 LayerNorm fold carries vithip_qscale(head_dim) -- against the live
oracle, whose attention is general in head_dim, and a transformers CLIP tower of head_dim 80 through INTEGRATION.md's mapping.

Reduced configs (tests/headdim_model.py): all have D % 64 == 0 and hidden % 64 == 0, so every ln_fold / dtype combination is open.
Bars: the ones of tests/test_gpu_forward.py (fp32: probabilities 1e-4 with the same top-1, logits 1e-3 of max |ref|) and of
tests/test_gpu_clip_engine.py (bf16: probabilities 2e-2, the same top-1 wherever the reference's top-2 gap exceeds 2e-2); class-token
attention 1e-4 (fp32) / 2e-2 (bf16).  Everything the engine promises to keep bit-identical is compared bitwise.
"""
import numpy as np
import pytest

import headdim_model
from conftest import oracle_config
from engine_helpers import device_attention, device_features, device_forward, same_bits
from headdim_model import cls_attention_ref
from test_cls_attention_abi import oracle_last_qkv
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

PROB_TOL, LOGIT_REL, BF16_PROB_TOL = 1e-4, 1e-3, 2e-2
CLS_CAP = {"f32": 1e-4, "bf16": 2e-2}
CONFIGS = {"HD80": headdim_model.HD80, "HD72": headdim_model.HD72, "HD104": headdim_model.HD104, "HD128": headdim_model.HD128,
           "HD80_257": headdim_model.HD80_257, "H14_LAYER": headdim_model.H14_LAYER}
W_SEED, IMG_SEED = 21, 7
_cache = {}


def rel_err(got, ref) -> float:
    return float(np.abs(got - ref).max()) / float(np.abs(ref).max())


def weights(name):
    if ("w", name) not in _cache:
        _cache[("w", name)] = synth.make_weights(CONFIGS[name], W_SEED)
    return _cache[("w", name)]


def images(name, n=5):
    if ("i", name, n) not in _cache:
        _cache[("i", name, n)] = synth.make_images(CONFIGS[name], n, IMG_SEED)
    return _cache[("i", name, n)]


def oracle_run(oracle, name, n=5):
    """(probs [n][NC], logits [n][NC]) of the live oracle on the first n images, computed once per model."""
    if ("o", name) not in _cache:
        cfg, W = CONFIGS[name], weights(name)
        runs = [oracle.forward_image(oracle_config(cfg), im, W) for im in images(name)]
        _cache[("o", name)] = (np.stack([r[0] for r in runs]), np.stack([r[1] for r in runs]))
    p, l = _cache[("o", name)]
    return p[:n], l[:n]


@pytest.fixture(scope="module")
def engines():
    cache = {}

    def get(name, **opt):
        key = (name, tuple(sorted(opt.items())))
        if key not in cache:
            cache[key] = B.Engine(CONFIGS[name], **opt)
            cache[key].load_weights(weights(name))
        return cache[key]

    yield get
    for eng in cache.values():
        eng.close()


# ---- 1: fp32 engines against the live oracle ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("fp32_split", [0, -1], ids=["split", "fp32-mfma"])
@pytest.mark.parametrize("ln_fold", [0, -1], ids=["ln-auto", "ln-kernels"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_fp32_engines_match_the_live_oracle(engines, oracle, name, ln_fold, fp32_split):
    eng = engines(name, max_batch=4, ln_fold=ln_fold, fp32_split=fp32_split)
    ref_p, ref_l = oracle_run(oracle, name)
    for n in (1, 3, 5):  # one chunk, a ragged one, the chunk loop
        probs = eng.forward(images(name)[:n])
        last = n % 4 or 4  # the logits tap holds the last chunk
        err, lerr = float(np.abs(probs - ref_p[:n]).max()), rel_err(eng.logits(last), ref_l[n - last:n])
        print(f"fp32 {name} n={n} ln_fold={ln_fold} fp32_split={fp32_split}: max |dprob| = {err:.3e}, logits {lerr:.3e}")
        assert err <= PROB_TOL and (probs.argmax(1) == ref_p[:n].argmax(1)).all(), (n, err)
        assert lerr <= LOGIT_REL, (n, lerr)


# ---- 2: bf16 engines ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ln_fold", [0, -1], ids=["ln-folded-qscaled", "ln-kernels-plain-q"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_bf16_engines_match_the_live_oracle(engines, oracle, name, ln_fold):
    eng = engines(name, max_batch=4, dtype="bf16", ln_fold=ln_fold)
    ref_p, _ = oracle_run(oracle, name)
    probs = eng.forward(images(name))
    err = float(np.abs(probs - ref_p).max())
    print(f"bf16 {name} ln_fold={ln_fold}: max |dprob| = {err:.3e}")
    assert err <= BF16_PROB_TOL, err
    top2 = np.sort(ref_p, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > BF16_PROB_TOL
    assert (probs.argmax(1) == ref_p.argmax(1))[clear].all()
    assert err > 1e-6  # really the bf16 path: fp32 engines sit orders below


# ---- 3: nothing changes a bit ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["HD80", "HD128"])
def test_lanes_pruning_graph_position_and_entry_change_no_bit(engines, name, dtype):
    cfg = CONFIGS[name]
    plain = engines(name, max_batch=8, dtype=dtype)
    base = images(name)
    idx = np.array([0, 1, 0, 3, 0])  # image 0 at places 0, 2 and 4 of a batch of 5
    imgs = base[idx]
    want, feat = plain.forward(imgs), plain.features(imgs, "cls")
    assert np.isfinite(want).all() and np.isfinite(feat).all()
    alone = plain.forward(base[:1])
    for place in (0, 2, 4):
        assert same_bits(want[place:place + 1], alone), place
    try:
        plain.set_lanes(2)
        assert same_bits(plain.forward(imgs), want) and same_bits(plain.features(imgs, "cls"), feat)
    finally:
        plain.set_lanes(1)
    pruned = engines(name, max_batch=8, dtype=dtype, prune_last_layer=True)
    assert same_bits(pruned.forward(imgs), want) and same_bits(pruned.features(imgs, "cls"), feat)
    # the device entry against the host entry, eager and as a replayed graph
    d5 = B.DeviceArray.from_numpy(imgs)
    dev, label, prob = device_forward(plain, d5, 5)
    assert same_bits(dev, want) and (label == want.argmax(1)).all() and same_bits(prob, want.max(1))
    assert same_bits(device_features(plain, d5, 5, "cls"), feat)
    graph = engines(name, max_batch=8, dtype=dtype, use_graph=True)
    first = device_forward(graph, d5, 5)[0]
    second = device_forward(graph, d5, 5)[0]  # the replay
    assert same_bits(first, want) and same_bits(second, want)
    # 8-bit pixels: the _u8 entry against the fp32 entry on the values it normalises to
    rng = np.random.default_rng(5)
    u8 = rng.integers(0, 256, (3, cfg.img_size, cfg.img_size, cfg.in_chans), dtype=np.uint8)
    f32 = B.images_u8_to_f32(u8)
    assert same_bits(plain.forward_u8(u8), plain.forward(f32))
    assert same_bits(plain.features_u8(u8, "cls"), plain.features(f32, "cls"))


# ---- 4: the class-token attention output -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["HD80", "HD104"])
def test_cls_attention_matches_the_restatement_on_the_oracles_q_and_k(engines, oracle, name, dtype):
    cfg, n = CONFIGS[name], 5
    T, heads, hd = cfg.tokens, cfg.num_heads, cfg.embed_dim // cfg.num_heads
    imgs = images(name)
    ref = np.concatenate([cls_attention_ref(oracle_last_qkv(oracle, cfg, im, weights(name)), 1, T, heads, hd) for im in imgs])
    eng = engines(name, max_batch=4, dtype=dtype)
    got = eng.cls_attention(imgs, "heads")
    mean = eng.cls_attention(imgs, "head_mean")
    assert got.shape == (n, heads, T) and mean.shape == (n, T)
    for p in (got, mean):
        assert np.isfinite(p).all()
        assert float(np.abs(p.astype(np.float64).sum(-1) - 1.0).max()) <= T * 2.0 ** -23
    err = float(np.abs(got - ref).max())
    merr = float(np.abs(mean - ref.mean(1)).max())
    print(f"cls attention {name} {dtype}: heads {err:.3e}, head_mean {merr:.3e}")
    assert err <= CLS_CAP[dtype] and merr <= CLS_CAP[dtype]
    want = got[:, 0].copy()
    for h in range(1, heads):
        want = want + got[:, h]
    assert same_bits(mean, want / np.float32(heads))  # HEAD_MEAN = the HEADS bits summed in head order
    # the same bits whatever prune_last_layer and lanes
    pruned = engines(name, max_batch=4, dtype=dtype, prune_last_layer=True)
    assert same_bits(pruned.cls_attention(imgs, "heads"), got) and same_bits(pruned.cls_attention(imgs, "head_mean"), mean)
    try:
        eng.set_lanes(2)
        assert same_bits(eng.cls_attention(imgs, "heads"), got) and same_bits(eng.cls_attention(imgs, "head_mean"), mean)
    finally:
        eng.set_lanes(1)
    d4 = B.DeviceArray.from_numpy(imgs[:4])
    assert same_bits(device_attention(eng, d4, 4, "heads"), got[:4])


# ---- 5: a transformers tower through the mapping -----------------------------------------------------------------------------------

def test_a_transformers_tower_of_head_dim_80_maps_through_the_table_to_the_engine():
    """The random CLIPVisionModelWithProjection of tests/test_headdim_model.py (hidden 320, 4 heads of 80, erf-GELU), mapped by
    clip_model.from_transformers and loaded with set_layernorm_eps, load_weights, set_pre_norm."""
    from test_clip_model import hf_run
    from test_headdim_model import make_tower
    torch, model, imgs = make_tower(80, "gelu")
    cfg, W, pre, eps = headdim_model.from_transformers(model)
    assert cfg.embed_dim // cfg.num_heads == 80 and cfg.mlp == "gelu"
    ref_e, ref_h = hf_run(torch, model, imgs)
    unit = ref_e / np.linalg.norm(ref_e, axis=1, keepdims=True)
    eng = B.Engine(cfg, max_batch=4)
    try:
        eng.set_layernorm_eps(eps)
        eng.load_weights(W)
        eng.set_pre_norm(*pre)
        x = imgs.numpy()
        head, got = eng.features(x, "head"), eng.features(x, "head", True)
        hid = eng.intermediate(x, [cfg.depth - 2], "tokens", False)[:, 0]
        eerr, uerr, herr = rel_err(head, ref_e), rel_err(got, unit), rel_err(hid, ref_h)
        print(f"transformers tower, head_dim 80: image_embeds {eerr:.3e}, unit {uerr:.3e}, hidden_states[-2] {herr:.3e} of max |ref|")
        assert eerr <= LOGIT_REL and uerr <= LOGIT_REL and herr <= LOGIT_REL
    finally:
        eng.close()


# ---- 6: refusals -------------------------------------------------------------------------------------------------------------------

def test_head_dims_off_the_set_are_refused_by_name():
    for D, heads in ((128, 4), (192, 4), (544, 4)):  # 32, 48, 136
        cfg = synth.ModelConfig(img_size=32, patch_size=16, num_classes=10, embed_dim=D, depth=1, num_heads=heads, hidden_dim=256)
        with pytest.raises(B.VitError) as err:
            B.Engine(cfg, max_batch=2)
        assert "head_dim" in str(err.value), str(err.value)
    # head_dim 72 at D = 288: fine for the attention kernels, refused by the bf16 path for the reason it always had
    cfg = synth.ModelConfig(img_size=32, patch_size=16, num_classes=10, embed_dim=288, depth=1, num_heads=4, hidden_dim=256)
    with pytest.raises(B.VitError) as err:
        B.Engine(cfg, max_batch=2, dtype="bf16")
    assert "multiples of 64" in str(err.value) and "head_dim" not in str(err.value), str(err.value)
