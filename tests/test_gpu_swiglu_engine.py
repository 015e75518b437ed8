"""Engines with the SwiGLU MLP (VIT_MLP_SWIGLU in vit_config.hidden_dim's kind bits) against tests/swiglu_model.py, which tests/test_swiglu_model.py pins
to transformers' Dinov2 modules.

Bars: fp32 probabilities 1e-4 (PROB_TOL) with the same top-1, logits and per-layer residual streams 1e-3 of max |ref| (LOGIT_REL, the
bar of tests/test_gpu_forward.py and of tests/test_gpu_intermediate.py); bf16 probabilities 2e-2 (the bar of tests/test_gpu_bf16.py)
with the same top-1 wherever the model's top-1 / top-2 margin exceeds that bar.  Everything the engine promises to keep bit-identical
(lanes, graph replay, the pruned last layer, host against device entry, batch position, copy_weights) is compared bitwise.
Measured on an MI355X: profiles/r18/swiglu.md.
"""
import dataclasses

import numpy as np
import pytest

import swiglu_model
from conftest import oracle_config
from engine_helpers import device_forward, same_bits
from swiglu_model import G14_LAYER, SMALL_SG, TINY_SG
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

PROB_TOL, LOGIT_REL, BF16_PROB_TOL = 1e-4, 1e-3, 2e-2
VIT_ERR_ARG, VIT_ERR_WEIGHTS = 1, 2
CONFIGS = {"tiny_sg": TINY_SG, "small_sg": SMALL_SG, "g14_layer": G14_LAYER}
SEED = 21
_cache = {}


def rel_err(got, ref) -> float:
    return float(np.abs(got - ref).max()) / float(np.abs(ref).max())


def weights(name):
    if ("w", name) not in _cache:
        _cache[("w", name)] = synth.make_weights(CONFIGS[name], SEED)
    return _cache[("w", name)]


def model_run(oracle, name, n):
    """(images, probs, logits, stages [n][depth + 1][T][D]) of tests/swiglu_model.py, computed once per (model, n)."""
    key = ("model", name, n)
    if key not in _cache:
        cfg = CONFIGS[name]
        imgs = synth.make_images(cfg, n, 100 + n)
        _cache[key] = (imgs,) + swiglu_model.forward(oracle, oracle_config(cfg), imgs, weights(name))
    return _cache[key]


@pytest.fixture(scope="module")
def engines():
    cache = {}

    def get(name, **opt):
        key = (name, tuple(sorted(opt.items())))
        if key not in cache:
            eng = B.Engine(CONFIGS[name], **opt)
            eng.load_weights(weights(name))
            cache[key] = eng
        return cache[key]

    yield get
    for eng in cache.values():
        eng.close()


def check_bf16_probs(probs, ref, what):
    err = float(np.abs(probs - ref).max())
    print(f"bf16 {what}: max |dprob| = {err:.3e}")
    assert err <= BF16_PROB_TOL, (what, err)
    top2 = np.sort(ref, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > BF16_PROB_TOL
    assert (probs.argmax(1) == ref.argmax(1))[clear].all(), what
    return err


# ---- fp32 against the model ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fp32_split", [0, -1], ids=["split", "fp32-mfma"])
@pytest.mark.parametrize("ln_fold", [0, -1], ids=["ln-folded", "ln-kernels"])
@pytest.mark.parametrize("name", ["tiny_sg", "small_sg"])
def test_fp32_probabilities_logits_and_stages_match_the_model(oracle, engines, name, ln_fold, fp32_split):
    cfg = CONFIGS[name]
    eng = engines(name, max_batch=4, ln_fold=ln_fold, fp32_split=fp32_split)
    layers = list(range(cfg.depth))
    for n in (1, 3, 5):   # one chunk, a ragged one, the chunk loop
        imgs, ref_p, ref_l, ref_s = model_run(oracle, name, n)
        probs = eng.forward(imgs)
        err = float(np.abs(probs - ref_p).max())
        last = n % 4 or 4  # the logits tap holds the last chunk
        lerr = rel_err(eng.logits(last), ref_l[-last:])
        got = eng.intermediate(imgs, layers, "tokens", 0)   # [n][depth][T][D]: the residual stream behind every layer
        assert got.shape == (n, cfg.depth, cfg.tokens, cfg.embed_dim)
        serr = max(rel_err(got[:, l], ref_s[:, l + 1]) for l in layers)
        print(f"fp32 {name} n={n} ln_fold={ln_fold} fp32_split={fp32_split}: max |dprob| = {err:.3e}, logits {lerr:.3e}, worst stage {serr:.3e}")
        assert err <= PROB_TOL and (probs.argmax(1) == ref_p.argmax(1)).all(), (n, err)
        assert lerr <= LOGIT_REL and serr <= LOGIT_REL, (n, lerr, serr)


# ---- bitwise identities ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["tiny_sg", "small_sg"])
def test_lanes_graph_pruning_entry_position_and_copy_change_no_bit(engines, name, dtype):
    cfg = CONFIGS[name]
    plain = engines(name, max_batch=8, dtype=dtype)
    base = synth.make_images(cfg, 4, 301)
    idx = np.array([0, 1, 2, 3, 3, 0, 2, 1, 1, 3, 0])   # 11 images: chunks of 8 and 3, every image at several places
    imgs = base[idx]
    want = plain.forward(imgs)
    assert np.isfinite(want).all()
    tokens = plain.features(imgs, "tokens")
    for k in range(4):   # a copy of one image at every batch position
        assert (want[idx == k] == want[idx == k][0]).all() and (tokens[idx == k] == tokens[idx == k][0]).all(), k
    # the device entry against the host entry
    dev, label, prob = device_forward(plain, B.DeviceArray.from_numpy(imgs[:8]), 8)
    assert same_bits(dev, want[:8]) and (label == want[:8].argmax(1)).all() and same_bits(prob, want[:8].max(1))
    try:
        plain.set_lanes(2)
        assert same_bits(plain.forward(imgs), want) and same_bits(plain.features(imgs, "tokens"), tokens)
    finally:
        plain.set_lanes(1)
    graph = engines(name, max_batch=8, dtype=dtype, use_graph=True)
    d8 = B.DeviceArray.from_numpy(imgs[:8])
    first = device_forward(graph, d8, 8)[0]
    second = device_forward(graph, d8, 8)[0]   # the replay
    assert same_bits(first, want[:8]) and same_bits(second, want[:8])
    pruned = engines(name, max_batch=8, dtype=dtype, prune_last_layer=True)
    assert same_bits(pruned.forward(imgs), want)
    assert same_bits(pruned.features(imgs, "cls"), plain.features(imgs, "cls"))
    copy = B.Engine(cfg, max_batch=8, dtype=dtype)
    try:
        copy.copy_weights_from(plain)
        assert same_bits(copy.forward(imgs), want)
    finally:
        copy.close()


def test_the_other_output_calls_run_on_a_swiglu_engine(oracle, engines):
    """Class attention, top-k and a caller's head route through the same layers: finite, of the documented shapes, and consistent with
    the probabilities."""
    cfg = SMALL_SG
    eng = engines("small_sg", max_batch=4)
    imgs, ref_p, _, ref_s = model_run(oracle, "small_sg", 5)
    probs = eng.forward(imgs)
    att = eng.cls_attention(imgs, "heads")
    assert att.shape == eng.attention_shape(5, "heads") and np.isfinite(att).all() and np.allclose(att.sum(-1), 1.0, atol=1e-5)
    labels, scores = B.split_topk(eng.topk_host(imgs, 3))
    assert (labels[:, 0] == probs.argmax(1)).all() and same_bits(np.ascontiguousarray(scores[:, 0]), probs.max(1))
    y = np.stack([oracle.layer_norm(np.ascontiguousarray(st[-1]), weights("small_sg")[-4], weights("small_sg")[-3]) for st in ref_s])
    assert rel_err(eng.features(imgs, "mean"), y[:, 1:].mean(1, dtype=np.float64)) <= LOGIT_REL


# ---- bf16 ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ln_fold", [0, -1], ids=["ln-folded", "ln-kernels"])
@pytest.mark.parametrize("name", ["tiny_sg", "small_sg"])
def test_bf16_probabilities_match_the_model_and_the_gelu_figure_is_printed_beside(oracle, engines, name, ln_fold):
    """u is rounded to bf16 in front of the gate, where GELU is applied to the fp32 accumulator: the GELU model of the same
    dimensions runs beside it (against the oracle) so that the record shows what that costs.  Only the SwiGLU figure is asserted."""
    cfg = CONFIGS[name]
    n = 6
    imgs, ref_p, _, _ = model_run(oracle, name, n)
    eng = engines(name, max_batch=4, dtype="bf16", ln_fold=ln_fold)
    err = check_bf16_probs(eng.forward(imgs), ref_p, f"{name} ln_fold={ln_fold} swiglu")
    twin = dataclasses.replace(cfg, mlp="gelu")
    Wt = synth.make_weights(twin, SEED)
    gelu = B.Engine(twin, max_batch=4, dtype="bf16", ln_fold=ln_fold)
    try:
        gelu.load_weights(Wt)
        gerr = float(np.abs(gelu.forward(imgs) - oracle.forward(oracle_config(twin), imgs, Wt)).max())
    finally:
        gelu.close()
    print(f"bf16 {name} ln_fold={ln_fold}: max |dprob| swiglu {err:.3e}, gelu twin {gerr:.3e}")


# ---- one layer at the full width of ViT-g/14 ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_one_layer_at_vit_g14_width(oracle, dtype):
    """embed 1536, 24 heads, hidden 4096: N = 8192, K = 4096 and D = 1536 through the fold, the split image and both GEMM families."""
    cfg, n = G14_LAYER, 2
    imgs, ref_p, ref_l, ref_s = model_run(oracle, "g14_layer", n)
    eng = B.Engine(cfg, max_batch=n, dtype=dtype)
    try:
        eng.load_weights(weights("g14_layer"))
        probs = eng.forward(imgs)
        if dtype == "bf16":
            check_bf16_probs(probs, ref_p, "g14 layer")
            return
        err, lerr = float(np.abs(probs - ref_p).max()), rel_err(eng.logits(n), ref_l)
        serr = rel_err(eng.intermediate(imgs, [0], "tokens", 0)[:, 0], ref_s[:, 1])
        print(f"fp32 g14 layer: max |dprob| = {err:.3e}, logits {lerr:.3e}, stage {serr:.3e}")
        assert err <= PROB_TOL and (probs.argmax(1) == ref_p.argmax(1)).all()
        assert lerr <= LOGIT_REL and serr <= LOGIT_REL
    finally:
        eng.close()


# ---- isolation -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_nan_image_leaves_the_other_rows_of_its_batch_their_bits(engines, dtype):
    cfg = SMALL_SG
    eng = engines("small_sg", max_batch=4, dtype=dtype)
    imgs = synth.make_images(cfg, 4, 55)
    clean = eng.forward(imgs)
    tokens = eng.features(imgs, "tokens")
    assert np.isfinite(clean).all()
    dirty = imgs.copy()
    dirty[2, 1, 7, 9] = np.nan
    got, got_tokens = eng.forward(dirty), eng.features(dirty, "tokens")
    good = [0, 1, 3]
    assert same_bits(got[good], clean[good]) and same_bits(got_tokens[good], tokens[good])
    assert not np.isfinite(got[2]).all() and not np.isfinite(got_tokens[2]).all()
    assert same_bits(eng.forward(imgs), clean)   # and the call behind it


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def test_mismatched_weights_and_kinds_are_refused_and_the_engine_stays_usable(engines):
    cfg = TINY_SG
    eng = engines("tiny_sg", max_batch=4)
    imgs = synth.make_images(cfg, 3, 9)
    before = eng.forward(imgs)
    W = list(weights("tiny_sg"))
    H, D = cfg.hidden_dim, cfg.embed_dim
    W[12] = np.ascontiguousarray(W[12][:H])   # what a GELU model of these dimensions holds
    with pytest.raises(B.VitError) as err:
        eng.load_weights(W)
    msg = str(err.value)
    assert err.value.code == VIT_ERR_WEIGHTS and "weight 12" in msg and str(H * D) in msg and str(2 * H * D) in msg, msg
    assert same_bits(eng.forward(imgs), before)
    with pytest.raises(B.VitError) as err:
        B.Engine(dataclasses.replace(cfg, mlp=7), max_batch=4)
    assert f"({VIT_ERR_ARG})" in str(err.value) and "MLP kind 7" in str(err.value), str(err.value)
    assert same_bits(eng.forward(imgs), before)
    # a GELU engine of the same eight dimensions refuses the SwiGLU image, and the SwiGLU engine the GELU one
    twin = dataclasses.replace(cfg, mlp="gelu")
    Wt = synth.make_weights(twin, SEED)
    gelu = B.Engine(twin, max_batch=4)
    try:
        gelu.load_weights(Wt)
        gbefore = gelu.forward(imgs)
        with pytest.raises(B.VitError) as err:
            gelu.load_weight_image(B.WeightImage.build(cfg, weights("tiny_sg")))
        assert err.value.code == VIT_ERR_WEIGHTS, str(err.value)
        assert same_bits(gelu.forward(imgs), gbefore)
        with pytest.raises(B.VitError) as err:
            eng.load_weight_image(B.WeightImage.build(twin, Wt))
        assert err.value.code == VIT_ERR_WEIGHTS, str(err.value)
        with pytest.raises(B.VitError) as err:
            eng.copy_weights_from(gelu)
        assert err.value.code == VIT_ERR_ARG, str(err.value)
        assert same_bits(eng.forward(imgs), before)
    finally:
        gelu.close()


# ---- the stage profile -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("lanes", [1, 2])
def test_the_gate_is_a_second_launch_of_the_fc1_stage(lanes, dtype):
    cfg = SMALL_SG
    twin = dataclasses.replace(cfg, mlp="gelu")
    imgs = synth.make_images(cfg, 4, 3)
    counts = {}
    for key, c, W in (("swiglu", cfg, weights("small_sg")), ("gelu", twin, synth.make_weights(twin, SEED))):
        eng = B.Engine(c, max_batch=4, dtype=dtype, lanes=lanes, profile=True)
        try:
            eng.load_weights(W)
            eng.reset_stage_times()
            eng.forward(imgs)
            counts[key] = {s: v["launches"] for s, v in eng.stage_times()["stages"].items()}
        finally:
            eng.close()
    assert set(counts["swiglu"]) == set(B.STAGES) == set(counts["gelu"])   # no new stage
    assert counts["gelu"]["fc1"] == cfg.depth * lanes and counts["swiglu"]["fc1"] == 2 * cfg.depth * lanes
    for s in B.STAGES:
        if s != "fc1":
            assert counts["swiglu"][s] == counts["gelu"][s], s
