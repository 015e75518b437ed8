"""Embedding outputs of the engine (vit_engine_features_*): class token, patch-token mean, all tokens.

References: the live oracle's encoder output through its own LayerNorm (pyoracle.layer_norm(stages[depth], W[-4], W[-3]); row 0
of it is what the oracle's classifier reads, tests/test_features_abi.py), and for ViT-B/16 the class row the reference's own
functions computed (stage_cls[:, 13] of tests/golden/vit_b16_e2e.npz).  Bars: 1e-3 x max |ref| (LOGIT_REL: the logits are a linear
map of these rows) for fp32 engines, the measured-and-doubled figures below for bf16 engines, and bitwise for everything the
engine promises to keep bit-identical.
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import oracle_config
from engine_helpers import CONFIGS, CONSTS, device_features, engines, same_bits, weights  # noqa: F401 (fixtures)
from test_features_abi import l2_normalize_f64
from test_input_u8_model import normalise_u8
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "vit_b16_e2e.npz")
LOGIT_REL = 1e-3
VIT_ERR_ARG = 1
KINDS = ("cls", "mean", "tokens")


def rel_err(got, ref) -> float:
    return float(np.abs(got - ref).max()) / float(np.abs(ref).max())


def oracle_tokens(oracle, cfg, imgs, W):
    """[n][T][D]: the final LayerNorm of the oracle's encoder output."""
    ocfg = oracle_config(cfg)
    return np.stack([oracle.layer_norm(oracle.forward_image(ocfg, im, W, want_stages=True)[2][cfg.depth], W[-4], W[-3]) for im in imgs])


def reference(y, kind):
    """The contract's row for `kind` from the normalised tokens y [n][T][D], float64 mean."""
    return {"cls": y[:, 0], "mean": y[:, 1:].mean(1, dtype=np.float64), "tokens": y}[kind]


# ---- 1, 2: fp32 engines against the oracle and the reference's golden class row ----------------------------------------

# Measured on an MI355X (profiles/r09/README.md): the largest max |d| / max |ref| over both models, all n and the three kinds
# (VIT_SMALL, n = 2, cls; the probabilities of the same path show 3.1e-6 absolute).  It sits far below the logits bar, so ten times
# it is asserted as well: a regression of two orders of magnitude cannot hide under 1e-3.
FP32_MEASURED = 8.5e-7


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_fp32_features_match_the_live_oracle(oracle, engines, weights, name):
    cfg, W = CONFIGS[name], weights(name, 21)
    eng = engines(name, 21, max_batch=4)  # chunk loop and ragged tails, as test_small_models_match_live_oracle
    worst = 0.0
    for n in (1, 2, 5, 11):
        imgs = synth.make_images(cfg, n, 100 + n)
        y = oracle_tokens(oracle, cfg, imgs, W)
        for kind in KINDS:
            got = eng.features(imgs, kind)
            assert got.shape == ((n, cfg.tokens, cfg.embed_dim) if kind == "tokens" else (n, cfg.embed_dim))
            err = rel_err(got, reference(y, kind))
            print(f"fp32 {name} n={n} {kind}: max |d| / max |ref| = {err:.3e}")
            worst = max(worst, err)
            assert err <= LOGIT_REL, (n, kind, err)
    assert worst <= 10 * FP32_MEASURED, worst  # measured: tiny 5.5e-7, small 8.5e-7


B16_CLS_MEASURED = 1.6e-6  # measured max |d| / max |ref| of the fp32 class row against stage_cls[:, 13] (profiles/r09/README.md)


def test_fp32_b16_class_row_matches_the_reference_golden(engines):
    g = np.load(GOLD)
    n = int(g["n_images"])
    assert int(g["weight_seed"]) == 1234
    imgs = synth.make_images(synth.VIT_B16, n, int(g["image_seed"]))
    got = engines("b16", max_batch=256).features(imgs, "cls")
    err = rel_err(got, g["stage_cls"][:, 13])
    print(f"fp32 b16 cls vs stage_cls[:, 13]: max |d| / max |ref| = {err:.3e}")
    assert err <= LOGIT_REL
    assert err <= 10 * B16_CLS_MEASURED  # measured 1.573e-6


# ---- 3: bitwise identities ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name,mb,n", [("tiny", 4, 11), ("b16", 16, 19)])
def test_class_row_of_tokens_is_cls_and_pruning_changes_no_bit(engines, name, mb, n, dtype):
    imgs = synth.make_images(CONFIGS[name], n, 301)
    plain, pruned = engines(name, max_batch=mb, dtype=dtype), engines(name, max_batch=mb, dtype=dtype, prune_last_layer=True)
    got = {k: plain.features(imgs, k) for k in KINDS}
    assert same_bits(got["tokens"][:, 0], got["cls"])
    for k in KINDS:  # CLS through the pruned layer; MEAN and TOKENS make the call run the last layer unpruned
        assert same_bits(pruned.features(imgs, k), got[k]), k
    # and the pruned engine's probabilities are what they were, before and after
    assert same_bits(pruned.forward(imgs), plain.forward(imgs))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["tiny", "b16"])
def test_lanes_change_no_bit(engines, name, dtype):
    imgs = synth.make_images(CONFIGS[name], 37, 302)  # chunks of 16, 16, 5: four lanes, four lanes, two lanes
    eng = engines(name, max_batch=16, dtype=dtype)
    want = {(k, l2): eng.features(imgs, k, l2) for k in KINDS for l2 in ((False,) if k == "tokens" else (False, True))}
    try:
        for lanes in (2, 4):
            eng.set_lanes(lanes)
            for (k, l2), w in want.items():
                assert same_bits(eng.features(imgs, k, l2), w), (lanes, k, l2)
    finally:
        eng.set_lanes(1)


@pytest.mark.parametrize("ln_fold", [0, -1])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name,mb", [("tiny", 16), ("small", 8), ("b16", 16)])
def test_pooling_scratch_of_a_lane_stays_inside_the_lanes_own_rows(engines, name, mb, dtype, ln_fold):
    """Lanes run on independent streams: while one lane pools, another may still be in its last layer, reading its rows of y and
    (bf16 fold) its bf16 copy of x in the upper half of the same allocation.  A timing race does not show in outputs, so the
    layout itself is checked: each lane's scratch lies inside that lane's own y rows, 16-byte aligned, and overlaps no range of
    any other lane, for every lane count and chunk size up to max_batch."""
    eng = engines(name, max_batch=mb, dtype=dtype, ln_fold=ln_fold)
    cfg = eng.cfg
    alloc = mb * cfg.tokens * cfg.embed_dim * 4
    overlap = lambda a, b: a[0] < b[1] and b[0] < a[1]
    seen_xa = False
    try:
        for lanes in (1, 2, 3, 4):
            eng.set_lanes(lanes)
            for nb in sorted({1, 2, 3, 5, 7, mb // 2, mb - 1, mb}):
                lay = eng.pool_scratch_layout(nb)
                assert len(lay) == (lanes if nb >= 2 * lanes else 1)
                for j, a in enumerate(lay):
                    s = a["scratch"]
                    assert s[0] % 16 == 0 and s[0] < s[1] <= alloc, (lanes, nb, j, a)
                    assert a["y"][0] <= s[0] and s[1] <= a["y"][1], (lanes, nb, j, a)
                    seen_xa = seen_xa or a["xa"] is not None
                    for k, b in enumerate(lay):
                        for what in ("scratch", "y", "xa"):
                            if k != j and b[what] is not None:
                                assert not overlap(s, b[what]), (lanes, nb, j, k, what, a, b)
                    if a["xa"] is not None:
                        assert not overlap(s, a["xa"]) and a["xa"][1] <= alloc
    finally:
        eng.set_lanes(1)
    # the bf16 copy of x exists exactly where the bf16 fold is on (embed_dim >= 128: every model here), off with ln_fold = -1
    assert seen_xa == (dtype == "bf16" and ln_fold == 0)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_graph_cache_keeps_forwards_and_feature_calls_apart(engines, dtype):
    """One input buffer and ONE output buffer for every call: only the output descriptor tells the calls apart."""
    plain = engines("tiny", max_batch=8, dtype=dtype)
    graph = engines("tiny", max_batch=8, dtype=dtype, use_graph=True)
    cfg, n = plain.cfg, 6
    d_images = B.DeviceArray.from_numpy(synth.make_images(cfg, n, 303))
    d_out = B.DeviceArray((n, max(cfg.tokens * cfg.embed_dim, cfg.num_classes)))

    def run(eng, what):
        if what == "probs":
            eng.forward_device(d_images.ptr, n, d_out.ptr)
            eng.sync()
            return d_out.numpy().reshape(-1)[:n * cfg.num_classes].copy()
        kind, l2 = what
        return device_features(eng, d_images, n, kind, l2, d_out=d_out)

    calls = [("cls", False), "probs", ("cls", False), ("cls", False), "probs", "probs", ("mean", False), ("mean", True), "probs",
             ("tokens", False), ("cls", True), ("tokens", False), "probs", ("mean", False)]
    want = {w: run(plain, w) for w in set(calls)}
    for w in calls:
        assert same_bits(run(graph, w), want[w]), w
    assert not same_bits(want[("cls", False)], want[("mean", False)])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_host_path_device_path_and_u8_input_agree_bit_for_bit(engines, dtype):
    eng = engines("small", max_batch=4, dtype=dtype)
    cfg, n = eng.cfg, 11
    u8 = np.random.default_rng(304).integers(0, 256, size=(n, cfg.img_size, cfg.img_size, cfg.in_chans), dtype=np.uint8)
    x = B.images_u8_to_f32(u8, *CONSTS)
    assert same_bits(x, normalise_u8(u8, *CONSTS))
    d_x, d_u8 = B.DeviceArray.from_numpy(x), B.DeviceArray.from_numpy(u8)
    for kind in ("tokens", "cls", "mean", "tokens"):  # widest row first: the staging grows once and then serves narrower rows
        for l2 in ((False,) if kind == "tokens" else (False, True)):
            host = eng.features(x, kind, l2)
            assert same_bits(device_features(eng, d_x, n, kind, l2), host), (kind, l2)
            assert same_bits(eng.features_u8(u8, kind, l2, *CONSTS), host), (kind, l2)
            assert same_bits(device_features(eng, d_u8, n, kind, l2, u8=True), host), (kind, l2)
    # the probabilities still come through the (regrown) staging unharmed
    assert same_bits(eng.forward_u8(u8, *CONSTS), eng.forward(x))


@pytest.mark.parametrize("dtype,batch", [("f32", 256), ("bf16", 256)])
def test_b16_copies_of_an_image_give_identical_rows_wherever_they_sit(engines, dtype, batch):
    """16 distinct images x 16 copies, shuffled: copies give identical rows wherever they sit.

    Known record (profiles/r09/README.md, "Seen once, not explained"; ADVICE.md, "bf16 first call"): the bf16 case failed ONCE in
    ten runs, on a new engine's first call (256 images, host path), in CLS -- which with one lane is the head's own LayerNorm launch
    on the same x, i.e. the bits differed in front of the feature code; 400 warm calls and 108 first calls, the previous build's
    forward included, never showed it again.  A failure here with CLS rows of ONE image differing on a first call is that record
    again and belongs to the bf16 first-call path of the forward, not to the pooling."""
    eng = engines("b16", max_batch=256, dtype=dtype)
    base = synth.make_images(synth.VIT_B16, 16, 305)
    idx = (np.arange(batch) % 16)[np.random.default_rng(0).permutation(batch)]
    # TOKENS on 32 of them (memory): the first and the last copy of each image, in the order they have in the shuffled batch
    where = [np.flatnonzero(idx == k) for k in range(16)]
    two_each = np.sort(np.concatenate([[w[0], w[-1]] for w in where]))
    for kind, sel in (("cls", np.arange(batch)), ("mean", np.arange(batch)), ("tokens", two_each)):
        got = eng.features(base[idx[sel]], kind)
        for k in range(16):
            at = np.flatnonzero(idx[sel] == k)
            rows = got[at]
            assert len(rows) == (2 if kind == "tokens" else 16)
            odd = [(int(sel[p]), int((r != rows[0]).sum()), float(np.abs(r - rows[0]).max())) for p, r in zip(at, rows) if not same_bits(r, rows[0])]
            assert not odd, f"{kind}: image {k} (first copy at {int(sel[at[0]])}): (position, differing elements, max |d|) = {odd}"
        assert not same_bits(got[idx[sel] == 0][0], got[idx[sel] == 1][0])


# ---- 4: CLS is the head's operand; feature calls leave no state behind -------------------------------------------------

@pytest.mark.parametrize("name,mb", [("small", 8), ("b16", 16)])
def test_cls_is_the_operand_of_the_head(engines, weights, name, mb):
    eng, W = engines(name, max_batch=mb), weights(name, 1234)
    n = 5
    imgs = synth.make_images(CONFIGS[name], n, 306)
    before = eng.forward(imgs)
    logits = eng.logits(n)
    cls = eng.features(imgs, "cls")
    with pytest.raises(B.VitError):  # nothing wrote logits: an error, not the previous call's
        eng.logits(n)
    head = B.gemm(cls, W[-2], W[-1])
    assert float(np.abs(head - logits).max()) <= LOGIT_REL * float(np.abs(logits).max())
    for kind in ("mean", "tokens"):
        eng.features(imgs, kind)
        with pytest.raises(B.VitError):
            eng.logits(1)
    assert same_bits(eng.forward(imgs), before)
    assert same_bits(eng.logits(n), logits)


# ---- 5: l2_normalize ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name,mb,n", [("small", 4, 11), ("b16", 16, 7)])
def test_l2_normalized_rows(engines, name, mb, n, dtype):
    eng = engines(name, max_batch=mb, dtype=dtype)
    imgs = synth.make_images(CONFIGS[name], n, 307)
    for kind in ("cls", "mean"):
        raw, unit = eng.features(imgs, kind), eng.features(imgs, kind, True)
        norms = np.sqrt((unit.astype(np.float64) ** 2).sum(1))
        assert float(np.abs(norms - 1.0).max()) <= 1e-5, kind
        # elements <= 1, a handful of fp32 roundings over a tree of depth ~12: 1e-5 is a bound with an order to spare
        assert float(np.abs(unit - l2_normalize_f64(raw)).max()) <= 1e-5, kind


# ---- 6: bf16 engines ---------------------------------------------------------------------------------------------------

# No project bar exists for bf16 activations.  Measured on an MI355X (profiles/r09/README.md): max |d| / max |ref| against the
# oracle over the seeds below; the assertion is twice the largest measured value rounded up to one significant digit.
# (bf16 error moves by about that much between seeds: the bf16 probability tests show 2.4e-3 measured under a 2e-2 bar.)
BF16_MEASURED = {"cls": 4.153e-3, "mean": 2.781e-3, "tokens": 3.035e-3, "b16_cls": 5.436e-3}
BF16_BAR = {"cls": 9e-3, "mean": 6e-3, "tokens": 7e-3, "b16_cls": 2e-2}


def bf16_check(kind, err):
    assert err > 1e-5, (kind, err)  # really the bf16 path: fp32 engines sit near 1e-6
    assert err <= BF16_BAR[kind], (kind, err, BF16_MEASURED[kind])  # 2 x measured, rounded up to one significant digit


def test_bf16_features_against_the_live_oracle(oracle, engines, weights):
    cfg, W = synth.VIT_SMALL, weights("small", 21)
    eng = engines("small", 21, max_batch=4, dtype="bf16")
    worst = dict.fromkeys(KINDS, 0.0)
    for n in (1, 3, 8):
        imgs = synth.make_images(cfg, n, 100 + n)
        y = oracle_tokens(oracle, cfg, imgs, W)
        for kind in KINDS:
            err = rel_err(eng.features(imgs, kind), reference(y, kind))
            print(f"bf16 small n={n} {kind}: max |d| / max |ref| = {err:.3e}")
            worst[kind] = max(worst[kind], err)
    for kind in KINDS:
        bf16_check(kind, worst[kind])


def test_bf16_b16_class_row_against_the_reference_golden(engines):
    g = np.load(GOLD)
    n = int(g["n_images"])
    imgs = synth.make_images(synth.VIT_B16, n, int(g["image_seed"]))
    err = rel_err(engines("b16", max_batch=256, dtype="bf16").features(imgs, "cls"), g["stage_cls"][:, 13])
    print(f"bf16 b16 cls vs stage_cls[:, 13]: max |d| / max |ref| = {err:.3e}")
    bf16_check("b16_cls", err)


# ---- profile -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", [1, 2])
def test_profile_accounts_feature_launches_to_the_layernorm_stage(engines, lanes):
    eng = engines("tiny", max_batch=4, lanes=lanes, profile=True, ln_fold=-1)
    n = 4
    imgs = synth.make_images(eng.cfg, n, 308)

    def launches(fn):
        eng.reset_stage_times()
        fn()
        t = eng.stage_times()
        assert t["images"] == n
        return {s: v["launches"] for s, v in t["stages"].items()}

    probs = launches(lambda: eng.forward(imgs))
    assert probs["head"] == lanes and probs["softmax"] == lanes
    for kind, l2 in (("cls", False), ("cls", True), ("mean", False), ("mean", True), ("tokens", False)):
        got = launches(lambda: eng.features(imgs, kind, l2))
        assert got["head"] == 0 and got["softmax"] == 0, (kind, got)
        assert got["ln"] == probs["ln"], (kind, got)  # one bracket per lane in place of the head's LayerNorm bracket
        assert {s: k for s, k in got.items() if s not in ("ln", "head", "softmax")} == \
               {s: k for s, k in probs.items() if s not in ("ln", "head", "softmax")}


# ---- 7: errors ---------------------------------------------------------------------------------------------------------

def test_invalid_arguments_return_vit_err_arg_and_leave_the_engine_usable(engines):
    L = B.lib()
    eng = engines("tiny", max_batch=4)
    cfg, n = eng.cfg, 3
    imgs = synth.make_images(cfg, n, 309)
    u8 = np.random.default_rng(310).integers(0, 256, size=(n, cfg.img_size, cfg.img_size, cfg.in_chans), dtype=np.uint8)
    ref, ref_cls = eng.forward(imgs), eng.features(imgs, "cls")
    d_x, d_u8 = B.DeviceArray.from_numpy(imgs), B.DeviceArray.from_numpy(u8)
    d_out = B.DeviceArray((n, cfg.tokens, cfg.embed_dim))
    spec = lambda k, l2=0: C.byref(B.CFeatureSpec(k, l2))
    mean, std = (C.c_float * 3)(*B.IMAGENET_MEAN), (C.c_float * 3)(*B.IMAGENET_STD)
    zero_std = (C.c_float * 3)(0.229, 0.0, 0.225)

    def still_fine():
        assert L.vit_engine_last_error(eng._h)
        assert same_bits(eng.forward(imgs), ref)
        assert same_bits(eng.features(imgs, "cls"), ref_cls)

    for d_images, nn, sp, out in [(None, n, spec(0), d_out.ptr), (d_x.ptr, n, spec(0), None), (d_x.ptr, n, None, d_out.ptr),
                                  (d_x.ptr, 0, spec(0), d_out.ptr), (d_x.ptr, -1, spec(1), d_out.ptr), (d_x.ptr, n, spec(3), d_out.ptr),
                                  (d_x.ptr, n, spec(-1), d_out.ptr), (d_x.ptr, n, spec(2, 1), d_out.ptr), (d_x.ptr, n, spec(0, 2), d_out.ptr),
                                  (d_x.ptr, n, spec(1, -1), d_out.ptr)]:
        assert L.vit_engine_features_device(eng._h, d_images, nn, sp, out, None) == VIT_ERR_ARG
        still_fine()
    for d_images, nn, m, s, sp in [(d_u8.ptr, n, None, std, spec(0)), (d_u8.ptr, n, mean, zero_std, spec(1)), (d_u8.ptr + 1, n, mean, std, spec(0)),
                                   (d_u8.ptr, n, mean, std, spec(7)), (d_u8.ptr, n, mean, std, spec(2, 1)), (d_u8.ptr, 0, mean, std, spec(0))]:
        assert L.vit_engine_features_device_u8(eng._h, d_images, nn, m, s, sp, d_out.ptr, None) == VIT_ERR_ARG
        still_fine()
    out = np.empty((n, cfg.tokens, cfg.embed_dim), np.float32)
    rows = (B.f32p * n)(*[out[i].ctypes.data_as(B.f32p) for i in range(n)])
    holes = (B.f32p * n)(*[out[i].ctypes.data_as(B.f32p) if i != 1 else None for i in range(n)])
    in_f32 = (B.f32p * n)(*[imgs[i].ctypes.data_as(B.f32p) for i in range(n)])
    in_u8 = (C.c_void_p * n)(*[u8[i].ctypes.data for i in range(n)])
    for ptrs, nn, sp, r in [(None, n, spec(0), rows), (in_f32, n, spec(0), None), (in_f32, 0, spec(0), rows), (in_f32, n, None, rows),
                            (in_f32, n, spec(5), rows), (in_f32, n, spec(2, 1), rows), (in_f32, n, spec(1), holes)]:
        assert L.vit_engine_features_host(eng._h, ptrs, nn, sp, r) == VIT_ERR_ARG
        still_fine()
    for ptrs, nn, m, s, sp, r in [(in_u8, n, mean, None, spec(0), rows), (in_u8, n, mean, zero_std, spec(0), rows),
                                  (in_u8, n, mean, std, spec(2, 1), rows), (None, n, mean, std, spec(0), rows)]:
        assert L.vit_engine_features_host_u8(eng._h, ptrs, nn, m, s, sp, r) == VIT_ERR_ARG
        still_fine()
    assert L.vit_engine_feature_row_elems(eng._h, spec(0)) == L.vit_engine_feature_row_elems(eng._h, spec(1, 1)) == cfg.embed_dim
    assert L.vit_engine_feature_row_elems(eng._h, spec(2)) == cfg.tokens * cfg.embed_dim
    assert L.vit_engine_feature_row_elems(eng._h, spec(2, 1)) == 0 and L.vit_engine_feature_row_elems(eng._h, spec(3)) == 0
    assert L.vit_engine_feature_row_elems(eng._h, None) == 0
    with pytest.raises(B.VitError):
        eng.features(imgs, "tokens", True)
    still_fine()
