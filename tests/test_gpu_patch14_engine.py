"""Engines at patch 14 (DINOv2's geometry): the general fp32 patch embedding in front of everything else, fp32 and bf16 engines.

References are the live oracle's, the ones the existing engine tests use (oracle.forward_image, tests/tap_model.py with
oracle.layer_norm, the float64 class-attention restatement on the oracle's q and k).  Bars: fp32 probabilities 1e-4 (PROB_TOL) with the
same top-1, logits and every fp32 row output 1e-3 of max |ref| (LOGIT_REL), bf16 probabilities 2e-2 (BF16_PROB_TOL) with the same top-1:
the bars of tests/test_gpu_forward.py and tests/test_gpu_bf16.py.  bf16 row outputs have no project bar; they are held to 2e-2 of
max |ref| -- five roundings to bf16 (2^-8 each) stacked, the probability figure taken relatively.  Everything the engine promises to
keep bit-identical is compared bitwise.
"""
import dataclasses

import numpy as np
import pytest

import pos_resample_model as PM
import tap_model
from conftest import oracle_config
from engine_helpers import CONSTS, device_forward, same_bits
from patch14_model import B14, CONFIGS14, ODD14, SMALL14
from test_cls_attention_abi import head_mean_ref, oracle_cls_attention
from test_input_u8_model import normalise_u8
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

PROB_TOL, LOGIT_REL, BF16_PROB_TOL = 1e-4, 1e-3, 2e-2
BF16_ROW_REL = 2e-2
ROW_BAR = {"f32": LOGIT_REL, "bf16": BF16_ROW_REL}
SEED = 21
_cache = {}


def rel_err(got, ref) -> float:
    return float(np.abs(got - ref).max()) / float(np.abs(ref).max())


def weights(name):
    if ("w", name) not in _cache:
        _cache[("w", name)] = synth.make_weights(CONFIGS14[name], SEED)
    return _cache[("w", name)]


def oracle_run(oracle, name, n):
    """(images, probs [n][NC], logits [n][NC], stages per image) of the live oracle, computed once per (model, n)."""
    key = ("oracle", name, n)
    if key not in _cache:
        cfg = CONFIGS14[name]
        imgs = synth.make_images(cfg, n, 100 + n)
        runs = [oracle.forward_image(oracle_config(cfg), im, weights(name), want_stages=True) for im in imgs]
        _cache[key] = (imgs, np.stack([r[0] for r in runs]), np.stack([r[1] for r in runs]), [r[2] for r in runs])
    return _cache[key]


@pytest.fixture(scope="module")
def engines():
    cache = {}

    def get(name, dtype, **opt):
        key = (name, dtype, tuple(sorted(opt.items())))
        if key not in cache:
            eng = B.Engine(CONFIGS14[name], dtype=dtype, **opt)
            eng.load_weights(weights(name))
            cache[key] = eng
        return cache[key]

    yield get
    for eng in cache.values():
        eng.close()


def check_probs(probs, ref, dtype, what):
    err = float(np.abs(probs - ref).max())
    print(f"{dtype} {what}: max |dprob| = {err:.3e}")
    assert err <= (PROB_TOL if dtype == "f32" else BF16_PROB_TOL), (what, err)
    assert (probs.argmax(1) == ref.argmax(1)).all(), what


# ---- forward -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["tiny14", "small14", "odd14"])
def test_forward_matches_the_live_oracle_on_the_host_and_the_device_path(oracle, engines, name, dtype):
    eng = engines(name, dtype, max_batch=4)  # 8 images: the chunk loop; 3: a ragged chunk
    for n in (1, 3, 8):
        imgs, ref_p, ref_l, _ = oracle_run(oracle, name, n)
        probs = eng.forward(imgs)
        check_probs(probs, ref_p, dtype, f"{name} n={n} host")
        if dtype == "f32":
            last = n % 4 or 4  # the logits tap holds the last chunk
            assert rel_err(eng.logits(last), ref_l[-last:]) <= LOGIT_REL, (name, n)
        dev, label, prob = device_forward(eng, B.DeviceArray.from_numpy(imgs), n)
        check_probs(dev, ref_p, dtype, f"{name} n={n} device")
        assert same_bits(dev, probs), (name, n)
        assert (label == probs.argmax(1)).all() and same_bits(prob, probs.max(1)), (name, n)


# ---- the other outputs -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["small14", "odd14"])  # a 4 x 4 map (16-byte runs) and a 3 x 3 map (the unaligned store path)
def test_features_intermediate_and_class_attention_match_the_live_oracle(oracle, engines, name, dtype):
    cfg, W = CONFIGS14[name], weights(name)
    eng = engines(name, dtype, max_batch=4)
    n = 3
    imgs, _, _, stages = oracle_run(oracle, name, n)
    bar = ROW_BAR[dtype]
    # features: the final LayerNorm of the oracle's encoder output
    y = np.stack([oracle.layer_norm(st[cfg.depth], W[-4], W[-3]) for st in stages])
    for kind, ref in (("cls", y[:, 0]), ("mean", y[:, 1:].mean(1, dtype=np.float64)), ("tokens", y)):
        got = eng.features(imgs, kind)
        err = rel_err(got, ref)
        print(f"{dtype} {name} features {kind}: max |d| / max |ref| = {err:.3e}")
        assert got.shape == ref.shape and err <= bar, (kind, err)
    # intermediate: every layer, four kinds, raw and normalised
    layers, g = list(range(cfg.depth)), cfg.img_size // cfg.patch_size
    for kind in tap_model.LAYOUTS:
        for norm in (0, 1):
            ref = tap_model.intermediate_reference(oracle, stages, layers, W[-4], W[-3], kind, norm, grid=g)
            got = eng.intermediate(imgs, layers, kind, norm)
            assert got.shape == ref.shape == eng.intermediate_shape(n, layers, kind, norm)
            err = max(rel_err(got[:, j], ref[:, j]) for j in range(ref.shape[1]))
            print(f"{dtype} {name} intermediate {kind} norm={norm}: worst tap max |d| / max |ref| = {err:.3e}")
            assert err <= bar, (kind, norm, err)
    assert eng.intermediate(imgs, layers, "map", 1).shape == (n, cfg.depth, cfg.embed_dim, g, g)
    # the class token's attention in the last layer: float64 restatement on the oracle's q and k
    ref = oracle_cls_attention(oracle, cfg, imgs, W)
    for kind, r in (("heads", ref), ("head_mean", head_mean_ref(ref))):
        got = eng.cls_attention(imgs, kind)
        err = float(np.abs(got - r).max())
        print(f"{dtype} {name} cls_attention {kind}: max |p - ref| = {err:.3e}")
        assert got.shape == r.shape
        assert err <= bar * float(np.abs(r).max()) and err <= (PROB_TOL if dtype == "f32" else BF16_PROB_TOL), (kind, err)


# ---- byte input ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_u8_forward_is_the_fp32_forward_of_the_host_normalised_image(engines, dtype):
    cfg = SMALL14
    eng = engines("small14", dtype, max_batch=4)
    u8 = np.random.default_rng(5).integers(0, 256, (5, cfg.img_size, cfg.img_size, cfg.in_chans), dtype=np.uint8)
    assert same_bits(eng.forward_u8(u8, *CONSTS), eng.forward(normalise_u8(u8, *CONSTS)))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_byte_and_image_calls_are_refused_where_img_size_is_no_multiple_of_4(engines, dtype):
    cfg = ODD14
    eng = engines("odd14", dtype, max_batch=4)
    n, S = 2, cfg.img_size
    imgs = synth.make_images(cfg, n, 77)
    before = eng.forward(imgs)
    u8 = np.random.default_rng(6).integers(0, 256, (n, S, S, 3), dtype=np.uint8)
    decoded = [np.random.default_rng(7 + i).integers(0, 256, (50 + i, 60, 3), dtype=np.uint8) for i in range(n)]
    d_u8 = B.DeviceArray.from_numpy(u8)
    d_dec = [B.DeviceArray.from_numpy(im) for im in decoded]
    recs = [(d.ptr, im.shape[0], im.shape[1]) for d, im in zip(d_dec, decoded)]
    d_out = B.DeviceArray((n * cfg.depth * cfg.tokens * cfg.embed_dim,))  # room for the largest output
    layers = [0, cfg.depth - 1]
    calls = {
        "forward_u8": lambda: eng.forward_u8(u8, *CONSTS),
        "forward_device_u8": lambda: eng.forward_device_u8(d_u8.ptr, n, d_out.ptr, *CONSTS),
        "forward_images": lambda: eng.forward_images(decoded, 48, *CONSTS),
        "forward_device_images": lambda: eng.forward_device_images(recs, d_out.ptr, 48, *CONSTS),
        "features_u8": lambda: eng.features_u8(u8, "mean", False, *CONSTS),
        "features_device_u8": lambda: eng.features_device_u8(d_u8.ptr, n, d_out.ptr, "mean", False, *CONSTS),
        "features_images": lambda: eng.features_images(decoded, 48, "mean", False, *CONSTS),
        "features_device_images": lambda: eng.features_device_images(recs, d_out.ptr, 48, "mean", False, *CONSTS),
        "cls_attention_u8": lambda: eng.cls_attention_u8(u8, "heads", *CONSTS),
        "cls_attention_device_u8": lambda: eng.cls_attention_device_u8(d_u8.ptr, n, d_out.ptr, "heads", *CONSTS),
        "cls_attention_images": lambda: eng.cls_attention_images(decoded, 48, "heads", *CONSTS),
        "cls_attention_device_images": lambda: eng.cls_attention_device_images(recs, d_out.ptr, 48, "heads", *CONSTS),
        "intermediate_u8": lambda: eng.intermediate_u8(u8, layers, "map", True, *CONSTS),
        "intermediate_device_u8": lambda: eng.intermediate_device_u8(d_u8.ptr, n, d_out.ptr, layers, "map", True, *CONSTS),
        "intermediate_images": lambda: eng.intermediate_images(decoded, 48, layers, "map", True, *CONSTS),
        "intermediate_device_images": lambda: eng.intermediate_device_images(recs, d_out.ptr, 48, layers, "map", True, *CONSTS),
    }
    for name, call in calls.items():
        with pytest.raises(B.VitError) as err:
            call()
        assert "failed (1)" in str(err.value) and "img_size" in str(err.value), (name, str(err.value))  # VIT_ERR_ARG
        assert same_bits(eng.forward(imgs), before), name  # the engine stays usable, the fp32 calls untouched
    # the six fp32-input calls other than forward (host) work on this engine
    d_img = B.DeviceArray.from_numpy(imgs)
    assert same_bits(device_forward(eng, d_img, n)[0], before)
    for out, host, dev, shape in (("features", lambda: eng.features(imgs, "mean"), lambda: eng.features_device(d_img.ptr, n, d_out.ptr, "mean"),
                                   eng.feature_shape(n, "mean")),
                                  ("cls_attention", lambda: eng.cls_attention(imgs, "heads"),
                                   lambda: eng.cls_attention_device(d_img.ptr, n, d_out.ptr, "heads"), eng.attention_shape(n, "heads")),
                                  ("intermediate", lambda: eng.intermediate(imgs, layers, "map", True),
                                   lambda: eng.intermediate_device(d_img.ptr, n, d_out.ptr, layers, "map", True),
                                   eng.intermediate_shape(n, layers, "map", True))):
        want = host()
        dev()
        eng.sync()
        got = d_out.numpy()[:int(np.prod(shape))].reshape(shape)
        assert np.isfinite(want).all() and same_bits(got, want), out


# ---- position-embedding resampling -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", list(PM.MODES))
@pytest.mark.parametrize("name", ["small14", "odd14"])
def test_checkpoint_of_a_5x5_grid_loads_into_4x4_and_3x3_engines(name, mode):
    cfg = CONFIGS14[name]
    src = dataclasses.replace(SMALL14, img_size=70)  # grid 5
    if "w70" not in _cache:
        _cache["w70"] = synth.make_weights(src, 31)
    W = _cache["w70"]
    g = cfg.img_size // cfg.patch_size
    want = PM.resample(np.ascontiguousarray(W[3], np.float32).reshape(src.tokens, src.embed_dim), g, mode)
    eng = B.Engine(cfg, max_batch=2)
    try:
        eng.load_weights(W, pos_from=70, pos_mode=mode)
        img = eng.read_weight_image()
        pos = np.asarray(img.tensors()[3], np.float32).reshape(cfg.tokens, cfg.embed_dim)
        assert same_bits(pos, want)
        assert np.isfinite(eng.forward(synth.make_images(cfg, 2, 9))).all()
    finally:
        eng.close()


# ---- invariants ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_lanes_and_batch_position_change_no_bit(engines, dtype):
    cfg = SMALL14
    eng = engines("small14", dtype, max_batch=8)
    base = synth.make_images(cfg, 4, 301)
    idx = np.array([0, 1, 2, 3, 3, 0, 2, 1, 1, 3, 0])  # 11 images: chunks of 8 and 3, every image at several places
    imgs = base[idx]
    want = eng.forward(imgs)
    tokens = eng.features(imgs, "tokens")
    for k in range(4):
        assert (want[idx == k] == want[idx == k][0]).all(), k
        assert (tokens[idx == k] == tokens[idx == k][0]).all(), k
    assert same_bits(eng.forward(base), want[[0, 1, 2, 3]])  # and in another batch
    try:
        eng.set_lanes(2)
        assert same_bits(eng.forward(imgs), want)
        assert same_bits(eng.features(imgs, "tokens"), tokens)
    finally:
        eng.set_lanes(1)


# ---- full size -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_b14_at_224_matches_the_live_oracle(oracle, dtype):
    """ViT-B/14 at 224, full depth: 257 tokens, the chunked fp32 attention and the streamed bf16 attention behind the new embedding."""
    n = 2
    imgs, ref_p, ref_l, _ = oracle_run(oracle, "b14", n)
    eng = B.Engine(B14, max_batch=n, dtype=dtype)
    try:
        eng.load_weights(weights("b14"))
        probs = eng.forward(imgs)
        check_probs(probs, ref_p, dtype, "b14 n=2")
        if dtype == "f32":
            err = rel_err(eng.logits(n), ref_l)
            print(f"f32 b14: logits max |d| / max |ref| = {err:.3e}")
            assert err <= LOGIT_REL
    finally:
        eng.close()
