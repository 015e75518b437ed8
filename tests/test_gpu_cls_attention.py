"""The class token's attention over the tokens in the last layer (vithip_cls_attention_*, vit_engine_cls_attention_*).

The reference is always the float64 restatement cls_attention_ref (tests/test_cls_attention_abi.py, held there against the oracle's
attention_core): on the kernel's own input for the kernel tests, on the live oracle's last-layer q and k for the engine tests --
never an output of the engine.  Bars: the project's probability bars against ViT_seq.c, 1e-4 absolute for fp32 and 2e-2 for bf16, as
caps; and twice the largest error measured on an MI355X per dtype and level (profiles/r11/README.md), which is what catches a
regression that stays under a cap.  Rows sum to one within T * 2^-23.  Everything the engine promises to keep bit-identical is
compared bitwise.
"""
import ctypes as C

import numpy as np
import pytest

import preproc_model as M
from engine_helpers import CONFIGS, CONSTS, device_attention, engines, same_bits, weights  # noqa: F401 (fixtures)
from test_cls_attention_abi import cls_attention_ref, head_mean_ref, oracle_cls_attention
from test_gpu_preproc import DeviceImages, random_images
from test_input_u8_model import normalise_u8
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

VIT_ERR_ARG = 1
HIP_INVALID = 1  # hipErrorInvalidValue
KINDS = ("heads", "head_mean")
RESIZE = {"tiny": 36, "small": 72}

CAP = {"f32": 1e-4, "bf16": 2e-2}  # the project's probability bars against ViT_seq.c: caps, never loosened
# Largest max |p - ref| measured on an MI355X, per dtype and level (profiles/r11/README.md, "Accuracy"); 2 x each is asserted beside
# the cap.  op: the kernel against the restatement on its own (for bf16: rounded) input, the peaked and the long rows included;
# engine: against the restatement on the live oracle's q and k.
MEASURED = {("f32", "op"): 5.979e-8,      # T = 2, heads = 3: half an ulp of a p near 1
            ("bf16", "op"): 8.091e-8,     # T = 2, heads = 2
            ("f32", "engine"): 7.787e-8,  # ViT-B/16, one image, HEADS (VIT_SMALL, lanes = 2, n = 11: 6.230e-8)
            ("bf16", "engine"): 3.074e-4}  # VIT_TINY, ln_fold = 0, n = 11, HEADS


def check_rows(p, T):
    """fp32 rows [..., T]: finite, and |sum_t p - 1| <= T * 2^-23 in float64 (twice the worst-case fp32 accumulation plus division
    rounding)."""
    assert p.dtype == np.float32 and p.shape[-1] == T and np.isfinite(p).all()
    off = float(np.abs(p.astype(np.float64).sum(-1) - 1.0).max())
    assert off <= T * 2.0 ** -23, (T, off)


def check_error(got, ref, dtype, level, what):
    """max |p - ref| under the cap; returns it for the caller's 2 x measured assertion on the worst case."""
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{dtype} {level} {what}: max |p - ref| = {err:.3e}")
    assert err <= CAP[dtype], (what, err)
    return err


def check_measured(worst, dtype, level):
    assert worst <= 2 * MEASURED[(dtype, level)], (dtype, level, worst, MEASURED[(dtype, level)])


def numpy_head_mean(p):
    """[n][heads][T] fp32 -> [n][T]: the heads added in order in fp32, then / (float)heads: what HEAD_MEAN must be, bit for bit."""
    acc = p[:, 0].copy()
    for h in range(1, p.shape[1]):
        acc = acc + p[:, h]
    return (acc / np.float32(p.shape[1])).astype(np.float32)


# ---- 1, 2: the kernel against the restatement --------------------------------------------------------------------------

def op_inputs(n, T, heads, seed):
    return np.random.default_rng(seed).standard_normal((n * T, 3 * heads * 64)).astype(np.float32)


def run_op(dtype, qkv, n, T, heads, head_mean=False, q_scaled=False, **kw):
    """-> (kernel output, the float64 reference on what the kernel read)"""
    if dtype == "f32":
        return B.cls_attention(qkv, n, T, heads, head_mean, **kw), cls_attention_ref(qkv, T, heads)
    bits = B.to_bf16_bits(qkv)
    got = B.cls_attention_bf16(bits, n, T, heads, head_mean, q_scaled, **kw)
    return got, cls_attention_ref(B.from_bf16_bits(bits), T, heads, q_scaled)


# one key, fewer keys than lanes, the wave boundary either side, the engine's sizes, both thresholds of the other attention kernels;
# 4099: past the kernel's LDS score cache (4096 keys), where pass 2 and 3 recompute
TOKENS = (1, 2, 5, 17, 50, 64, 65, 197, 225, 577, 705)


@pytest.fixture(scope="module")
def op_worst():
    return {"f32": 0.0, "bf16": 0.0}


@pytest.mark.parametrize("T", TOKENS + (4099,))
def test_kernel_matches_the_restatement(T, op_worst):
    n = 3
    for dtype in ("f32", "bf16"):
        for heads in ((1, 2, 3) if T <= 705 else (1, 2)):
            qkv = op_inputs(n, T, heads, 1000 * T + heads)
            got, ref = run_op(dtype, qkv, n, T, heads)
            assert got.shape == (n, heads, T)
            check_rows(got, T)
            op_worst[dtype] = max(op_worst[dtype], check_error(got, ref, dtype, "op", f"T={T} heads={heads}"))
            mean, _ = run_op(dtype, qkv, n, T, heads, head_mean=True)
            assert mean.shape == (n, T) and same_bits(mean, numpy_head_mean(got)), (dtype, T, heads)
            check_rows(mean, T)
        check_measured(op_worst[dtype], dtype, "op")


def test_kernel_q_scaled_reads_prescaled_queries(op_worst):
    n, heads = 3, 3
    for T in (5, 197, 577):
        qkv = op_inputs(n, T, heads, 77 + T)
        qkv[:, :heads * 64] *= np.float32(B.QSCALE)  # rounded to bf16 by run_op before the reference reads it
        got, ref = run_op("bf16", qkv, n, T, heads, q_scaled=True)
        check_rows(got, T)
        op_worst["bf16"] = max(op_worst["bf16"], check_error(got, ref, "bf16", "op", f"q_scaled T={T}"))
        mean, _ = run_op("bf16", qkv, n, T, heads, head_mean=True, q_scaled=True)
        assert same_bits(mean, numpy_head_mean(got))
        # and the flag matters: the plain exponent on the same bits is another distribution
        plain, _ = run_op("bf16", qkv, n, T, heads)
        assert not same_bits(plain, got)
    check_measured(op_worst["bf16"], "bf16", "op")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_kernel_peaked_rows_give_one_and_zeros(dtype, op_worst):
    """One key per (image, head) scaled so that its score is about 200 above the rest: p = 1 there, exact zeros or denormals
    elsewhere, no NaN."""
    n, T, heads = 3, 197, 3
    qkv = op_inputs(n, T, heads, 5)
    r = qkv.reshape(n, T, 3, heads, 64)  # a view
    peak = np.array([[(7 * i + 50 * h + 3) % T for h in range(heads)] for i in range(n)])
    for i in range(n):
        for h in range(heads):
            q = r[i, 0, 0, h]
            r[i, peak[i, h], 1, h] = q * np.float32(1600.0 / float(q.astype(np.float64) @ q.astype(np.float64)))  # q . k = 1600: score 200
    for q_scaled in ((False,) if dtype == "f32" else (False, True)):
        x = qkv.copy()
        if q_scaled:
            x[:, :heads * 64] *= np.float32(B.QSCALE)
        got, ref = run_op(dtype, x, n, T, heads, q_scaled=q_scaled)
        check_rows(got, T)
        op_worst[dtype] = max(op_worst[dtype], check_error(got, ref, dtype, "op", f"peaked q_scaled={q_scaled}"))
        for i in range(n):
            for h in range(heads):
                assert got[i, h, peak[i, h]] == np.float32(1.0)
                rest = np.delete(got[i, h], peak[i, h])
                assert (rest >= 0).all() and float(rest.max()) < 2.0 ** -126  # zeros or denormals
    check_measured(op_worst[dtype], dtype, "op")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_kernel_writes_only_its_rows(dtype):
    n, T, heads = 3, 65, 3
    qkv = op_inputs(n, T, heads, 9)
    for head_mean in (False, True):
        row = T if head_mean else heads * T
        want, _ = run_op(dtype, qkv, n, T, heads, head_mean)
        raw, _ = run_op(dtype, qkv, n, T, heads, head_mean, ld_out=row + 5, fill=np.nan)
        assert raw.shape == (n, row + 5)
        assert same_bits(raw[:, :row], want.reshape(n, row))
        assert np.isnan(raw[:, row:]).all()


def test_kernel_refuses_bad_arguments():
    L = B.lib()
    n, T, heads = 2, 5, 2
    w = 3 * heads * 64
    dq, do = B.DeviceArray((n * T, w)), B.DeviceArray.from_numpy(np.full((n, heads * T), 7.0, np.float32))
    f32 = lambda *a: L.vithip_cls_attention_f32(None, *a)
    b16 = lambda *a: L.vithip_cls_attention_bf16(None, *a)
    for args in [(None, w, do.ptr, heads * T, n, T, heads, 0), (dq.ptr, w, None, heads * T, n, T, heads, 0),
                 (dq.ptr, w, do.ptr, heads * T, 0, T, heads, 0), (dq.ptr, w, do.ptr, heads * T, n, 0, heads, 0),
                 (dq.ptr, w, do.ptr, heads * T, n, T, 0, 0), (dq.ptr, w, do.ptr, heads * T, n, T, heads, 2),
                 (dq.ptr, w - 4, do.ptr, heads * T, n, T, heads, 0), (dq.ptr, w + 2, do.ptr, heads * T, n, T, heads, 0),
                 (dq.ptr, w, do.ptr, heads * T - 1, n, T, heads, 0), (dq.ptr, w, do.ptr, T - 1, n, T, heads, 1),
                 (dq.ptr + 4, w, do.ptr, heads * T, n, T, heads, 0), (dq.ptr, w, do.ptr + 2, heads * T, n, T, heads, 0)]:
        assert f32(*args) == HIP_INVALID, args
        assert b16(*args, 0) == HIP_INVALID, args
    assert b16(dq.ptr, w + 4, do.ptr, heads * T, n, T, heads, 0, 0) == HIP_INVALID  # bf16 rows step in 16 bytes = 8 elements
    assert b16(dq.ptr, w, do.ptr, heads * T, n, T, heads, 0, 2) == HIP_INVALID
    assert (do.numpy() == 7.0).all()


# ---- engines -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def oracle_maps(oracle, weights):
    """(name, n) -> (images, [n][heads][T] float64): the restatement on the live oracle's last-layer q and k, weight seed 21;
    computed once and shared."""
    cache = {}

    def get(name, n):
        if (name, n) not in cache:
            imgs = synth.make_images(CONFIGS[name], n, 100 + n)
            cache[(name, n)] = (imgs, oracle_cls_attention(oracle, CONFIGS[name], imgs, weights(name, 21)))
        return cache[(name, n)]

    return get


def against_oracle(eng, oracle_maps, name, ns, dtype, what):
    """Both kinds for every n: shapes, row sums, the cap; HEAD_MEAN = the HEADS bits reduced.  Returns the worst error."""
    cfg, worst = CONFIGS[name], 0.0
    for n in ns:
        imgs, ref = oracle_maps(name, n)
        heads = eng.cls_attention(imgs, "heads")
        assert heads.shape == (n, cfg.num_heads, cfg.tokens)
        check_rows(heads, cfg.tokens)
        worst = max(worst, check_error(heads, ref, dtype, "engine", f"{name} {what} n={n} heads"))
        mean = eng.cls_attention(imgs, "head_mean")
        assert mean.shape == (n, cfg.tokens)
        check_rows(mean, cfg.tokens)
        worst = max(worst, check_error(mean, head_mean_ref(ref), dtype, "engine", f"{name} {what} n={n} head_mean"))
        assert same_bits(mean, numpy_head_mean(heads)), (name, what, n)
    return worst


F32_OPTIONS = {"default": {}, "ln_fold_off": {"ln_fold": -1}, "fp32_split_off": {"fp32_split": -1}, "pruned": {"prune_last_layer": True},
               "lanes2": {"lanes": 2}}


@pytest.mark.parametrize("opt", list(F32_OPTIONS))
@pytest.mark.parametrize("name", ["tiny", "small"])
def test_fp32_engines_match_the_live_oracle(engines, oracle_maps, name, opt):
    eng = engines(name, 21, max_batch=4, **F32_OPTIONS[opt])  # chunk loop and ragged tails
    check_measured(against_oracle(eng, oracle_maps, name, (1, 2, 5, 11), "f32", opt), "f32", "engine")


def test_fp32_b16_image_matches_the_live_oracle(engines, oracle_maps):
    eng = engines("b16", 21, max_batch=2)
    check_measured(against_oracle(eng, oracle_maps, "b16", (1,), "f32", "default"), "f32", "engine")


@pytest.mark.parametrize("ln_fold", [0, -1])  # the fold keeps QSCALE * q in the Q columns: q_scaled on and off
@pytest.mark.parametrize("name", ["tiny", "small"])
def test_bf16_engines_match_the_live_oracle(engines, oracle_maps, name, ln_fold):
    eng = engines(name, 21, max_batch=4, dtype="bf16", ln_fold=ln_fold)
    worst = against_oracle(eng, oracle_maps, name, (1, 2, 5, 11), "bf16", f"ln_fold={ln_fold}")
    assert worst > 1e-6, worst  # really the bf16 path: fp32 engines sit orders below
    check_measured(worst, "bf16", "engine")


# ---- 5: bit identities -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["tiny", "small"])
def test_pruning_and_lanes_change_no_bit(engines, name, dtype):
    imgs = synth.make_images(CONFIGS[name], 37, 401)  # chunks of 16, 16, 5: four lanes, four lanes, two lanes
    eng = engines(name, max_batch=16, dtype=dtype)
    pruned = engines(name, max_batch=16, dtype=dtype, prune_last_layer=True)
    want = {k: eng.cls_attention(imgs, k) for k in KINDS}
    probs = eng.forward(imgs)
    for k in KINDS:
        assert same_bits(pruned.cls_attention(imgs, k), want[k]), k
    assert same_bits(pruned.forward(imgs), probs)  # and the pruned engine's probabilities are what they were
    for e in (eng, pruned):
        try:
            for lanes in (2, 4):
                e.set_lanes(lanes)
                for k in KINDS:
                    assert same_bits(e.cls_attention(imgs, k), want[k]), (lanes, k)
        finally:
            e.set_lanes(1)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["tiny", "small"])
def test_host_path_device_path_and_u8_input_agree_bit_for_bit(engines, name, dtype):
    eng = engines(name, max_batch=4, dtype=dtype)
    cfg, n = eng.cfg, 11
    u8 = np.random.default_rng(402).integers(0, 256, size=(n, cfg.img_size, cfg.img_size, cfg.in_chans), dtype=np.uint8)
    x = normalise_u8(u8, *CONSTS)
    d_x, d_u8 = B.DeviceArray.from_numpy(x), B.DeviceArray.from_numpy(u8)
    before = eng.forward(x)
    for kind in KINDS:
        host = eng.cls_attention(x, kind)
        assert same_bits(device_attention(eng, d_x, n, kind), host), kind
        assert same_bits(eng.cls_attention_u8(u8, kind, *CONSTS), host), kind
        assert same_bits(device_attention(eng, d_u8, n, kind, u8=True), host), kind
    assert same_bits(eng.forward_u8(u8, *CONSTS), before)  # the probabilities come through the shared staging unharmed


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["tiny", "small"])
def test_images_calls_equal_u8_calls_on_the_restatements_bytes(engines, name, dtype):
    eng = engines(name, max_batch=4, dtype=dtype)
    cfg, R, n = eng.cfg, RESIZE[name], 7
    sizes = [(R, R), (R + R // 2, 2 * R - 1), (2 * R + 1, R + 3), (R // 2, R // 2 + 5), (R + 1, R + 1), (3 * R, R), (cfg.img_size, cfg.img_size)]
    imgs = random_images(sizes, cfg.in_chans, 403)
    u8 = np.stack([M.resize_crop(im, R, cfg.img_size) for im in imgs])
    dev = DeviceImages(imgs)
    for kind in KINDS:
        want = eng.cls_attention_u8(u8, kind, *CONSTS)
        assert same_bits(eng.cls_attention_images(imgs, R, kind, *CONSTS), want), kind
        d_out = B.DeviceArray(eng.attention_shape(n, kind))
        eng.cls_attention_device_images(dev.triples, d_out.ptr, R, kind, *CONSTS)
        eng.sync()
        assert same_bits(d_out.numpy(), want), kind


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["tiny", "small"])
def test_copies_of_an_image_give_identical_rows_wherever_they_sit(engines, name, dtype):
    """4 distinct images x 16 copies, shuffled through a batch of 64 (chunks of 16): the copies' rows are identical."""
    eng = engines(name, max_batch=16, dtype=dtype)
    base = synth.make_images(CONFIGS[name], 4, 404)
    idx = (np.arange(64) % 4)[np.random.default_rng(0).permutation(64)]
    for kind in KINDS:
        got = eng.cls_attention(base[idx], kind)
        for k in range(4):
            rows = got[idx == k]
            assert len(rows) == 16 and all(same_bits(r, rows[0]) for r in rows), (kind, k)
        assert not same_bits(got[idx == 0][0], got[idx == 1][0])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["tiny", "small"])
def test_graph_engine_returns_the_eager_bits_and_keeps_the_calls_apart(engines, name, dtype):
    """One input buffer and ONE output buffer for every call: only the output descriptor tells the calls apart."""
    plain = engines(name, max_batch=8, dtype=dtype)
    graph = engines(name, max_batch=8, dtype=dtype, use_graph=True)
    cfg, n = plain.cfg, 6
    d_images = B.DeviceArray.from_numpy(synth.make_images(cfg, n, 405))
    d_out = B.DeviceArray((n, max(cfg.num_heads * cfg.tokens, cfg.embed_dim, cfg.num_classes)))

    def run(eng, what):
        if what == "probs":
            eng.forward_device(d_images.ptr, n, d_out.ptr)
            eng.sync()
            return d_out.numpy().reshape(-1)[:n * cfg.num_classes].copy()
        if what == "cls":
            eng.features_device(d_images.ptr, n, d_out.ptr, "cls")
            eng.sync()
            return d_out.numpy().reshape(-1)[:n * cfg.embed_dim].copy()
        return device_attention(eng, d_images, n, what, d_out=d_out)

    calls = ["probs", "cls", "heads", "head_mean"] * 2 + ["heads", "heads", "probs", "head_mean", "cls", "head_mean"]
    want = {w: run(plain, w) for w in set(calls)}
    for w in calls:
        assert same_bits(run(graph, w), want[w]), w
    assert not same_bits(want["heads"].reshape(-1)[:n * cfg.tokens], want["head_mean"].reshape(-1))


# ---- 6: launch accounting ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", [1, 2])
def test_profile_shows_the_last_layer_stopping_behind_in_proj(engines, lanes):
    eng = engines("small", max_batch=4, lanes=lanes, profile=True, ln_fold=-1)
    n, depth = 4, eng.cfg.depth
    imgs = synth.make_images(eng.cfg, n, 406)

    def launches(fn):
        eng.reset_stage_times()
        fn()
        t = eng.stage_times()
        assert t["images"] == n
        return {s: v["launches"] for s, v in t["stages"].items()}

    probs = launches(lambda: eng.forward(imgs))
    for kind in KINDS:
        got = launches(lambda: eng.cls_attention(imgs, kind))
        assert got["outproj"] == got["fc1"] == got["fc2"] == (depth - 1) * lanes, (kind, got)
        assert got["head"] == 0 and got["softmax"] == 0, (kind, got)
        assert got["attn"] == depth * lanes, (kind, got)  # depth - 1 attention launches and the new kernel
        assert got["qkv"] == probs["qkv"] and got["embed"] == probs["embed"], (kind, got)
        assert got["ln"] == probs["ln"] - 2 * lanes, (kind, got)  # without the fold: no LN2 of the last layer, no final LayerNorm
    after = launches(lambda: eng.forward(imgs))
    assert after == probs
    assert probs["outproj"] == probs["fc1"] == probs["fc2"] == probs["attn"] == depth * lanes
    assert probs["head"] == probs["softmax"] == lanes


# ---- 8: errors ---------------------------------------------------------------------------------------------------------

def test_invalid_arguments_return_vit_err_arg_and_leave_the_engine_usable(engines):
    L = B.lib()
    eng = engines("tiny", max_batch=4)
    cfg, n = eng.cfg, 3
    imgs = synth.make_images(cfg, n, 407)
    u8 = np.random.default_rng(408).integers(0, 256, size=(n, cfg.img_size, cfg.img_size, cfg.in_chans), dtype=np.uint8)
    ref, ref_cls, ref_attn = eng.forward(imgs), eng.features(imgs, "cls"), eng.cls_attention(imgs, "heads")
    d_x, d_u8 = B.DeviceArray.from_numpy(imgs), B.DeviceArray.from_numpy(u8)
    d_out = B.DeviceArray((n, cfg.num_heads, cfg.tokens))
    spec = lambda k, r=0: C.byref(B.CAttentionSpec(k, r))
    mean, std = (C.c_float * 3)(*B.IMAGENET_MEAN), (C.c_float * 3)(*B.IMAGENET_STD)
    zero_std = (C.c_float * 3)(0.229, 0.0, 0.225)
    nan_mean = (C.c_float * 3)(0.485, float("nan"), 0.406)

    def still_fine():
        assert L.vit_engine_last_error(eng._h)
        assert same_bits(eng.forward(imgs), ref)
        assert same_bits(eng.features(imgs, "cls"), ref_cls)
        assert same_bits(eng.cls_attention(imgs, "heads"), ref_attn)

    for d_images, nn, sp, out in [(None, n, spec(0), d_out.ptr), (d_x.ptr, n, spec(0), None), (d_x.ptr, n, None, d_out.ptr),
                                  (d_x.ptr, 0, spec(0), d_out.ptr), (d_x.ptr, -1, spec(1), d_out.ptr), (d_x.ptr, n, spec(2), d_out.ptr),
                                  (d_x.ptr, n, spec(-1), d_out.ptr), (d_x.ptr, n, spec(0, 1), d_out.ptr), (d_x.ptr, n, spec(1, -1), d_out.ptr)]:
        assert L.vit_engine_cls_attention_device(eng._h, d_images, nn, sp, out, None) == VIT_ERR_ARG
        still_fine()
    for d_images, nn, m, s, sp, out in [(d_u8.ptr, n, None, std, spec(0), d_out.ptr), (d_u8.ptr, n, mean, None, spec(0), d_out.ptr),
                                        (d_u8.ptr, n, mean, zero_std, spec(1), d_out.ptr), (d_u8.ptr, n, nan_mean, std, spec(0), d_out.ptr),
                                        (d_u8.ptr + 1, n, mean, std, spec(0), d_out.ptr), (d_u8.ptr, n, mean, std, spec(7), d_out.ptr),
                                        (d_u8.ptr, n, mean, std, spec(0, 3), d_out.ptr), (d_u8.ptr, 0, mean, std, spec(0), d_out.ptr),
                                        (None, n, mean, std, spec(0), d_out.ptr), (d_u8.ptr, n, mean, std, None, d_out.ptr),
                                        (d_u8.ptr, n, mean, std, spec(0), None)]:
        assert L.vit_engine_cls_attention_device_u8(eng._h, d_images, nn, m, s, sp, out, None) == VIT_ERR_ARG
        still_fine()
    out = np.empty((n, cfg.num_heads, cfg.tokens), np.float32)
    rows = (B.f32p * n)(*[out[i].ctypes.data_as(B.f32p) for i in range(n)])
    holes = (B.f32p * n)(*[out[i].ctypes.data_as(B.f32p) if i != 1 else None for i in range(n)])
    in_f32 = (B.f32p * n)(*[imgs[i].ctypes.data_as(B.f32p) for i in range(n)])
    in_holes = (B.f32p * n)(*[imgs[i].ctypes.data_as(B.f32p) if i != 2 else None for i in range(n)])
    in_u8 = (C.c_void_p * n)(*[u8[i].ctypes.data for i in range(n)])
    for ptrs, nn, sp, r in [(None, n, spec(0), rows), (in_f32, n, spec(0), None), (in_f32, 0, spec(0), rows), (in_f32, n, None, rows),
                            (in_f32, n, spec(5), rows), (in_f32, n, spec(1, 1), rows), (in_f32, n, spec(1), holes),
                            (in_holes, n, spec(0), rows)]:
        assert L.vit_engine_cls_attention_host(eng._h, ptrs, nn, sp, r) == VIT_ERR_ARG
        still_fine()
    for ptrs, nn, m, s, sp, r in [(in_u8, n, mean, None, spec(0), rows), (in_u8, n, mean, zero_std, spec(0), rows),
                                  (in_u8, n, mean, std, spec(2), rows), (in_u8, n, mean, std, spec(0, 1), rows),
                                  (None, n, mean, std, spec(0), rows), (in_u8, n, mean, std, spec(0), None)]:
        assert L.vit_engine_cls_attention_host_u8(eng._h, ptrs, nn, m, s, sp, r) == VIT_ERR_ARG
        still_fine()
    # decoded images: what the matching forward refuses, and the spec
    R = RESIZE["tiny"]
    srcs = random_images([(R, R + 3), (2 * R, R), (R + 1, R + 1)], cfg.in_chans, 409)
    dev = DeviceImages(srcs)
    keep, host_recs = B.host_image_records(srcs, cfg.in_chans)
    pp = lambda r=R, m=B.IMAGENET_MEAN, s=B.IMAGENET_STD: C.byref(B.preproc_params(r, m, s, cfg.in_chans))
    null_pixels = B.image_records([(0, R, R)] + dev.triples[1:])
    huge = B.image_records([(dev.triples[0][0], 20000, R)] + dev.triples[1:])
    for recs, nn, p, sp, o in [(None, n, pp(), spec(0), d_out.ptr), (dev.records, 0, pp(), spec(0), d_out.ptr), (dev.records, n, None, spec(0), d_out.ptr),
                               (dev.records, n, pp(), None, d_out.ptr), (dev.records, n, pp(), spec(0), None), (dev.records, n, pp(), spec(2), d_out.ptr),
                               (dev.records, n, pp(), spec(0, 1), d_out.ptr), (dev.records, n, pp(cfg.img_size - 1), spec(0), d_out.ptr),
                               (dev.records, n, pp(4097), spec(0), d_out.ptr), (dev.records, n, pp(R, B.IMAGENET_MEAN, (0.2, 0.0, 0.2)), spec(0), d_out.ptr),
                               (null_pixels, n, pp(), spec(0), d_out.ptr), (huge, n, pp(), spec(1), d_out.ptr)]:
        assert L.vit_engine_cls_attention_device_images(eng._h, recs, nn, p, sp, o, None) == VIT_ERR_ARG
        still_fine()
    for recs, nn, p, sp, r in [(None, n, pp(), spec(0), rows), (host_recs, 0, pp(), spec(0), rows), (host_recs, n, None, spec(0), rows),
                               (host_recs, n, pp(), None, rows), (host_recs, n, pp(), spec(0), None), (host_recs, n, pp(), spec(3), rows),
                               (host_recs, n, pp(), spec(1, 2), rows), (host_recs, n, pp(cfg.img_size - 1), spec(0), rows),
                               (host_recs, n, pp(), spec(0), holes)]:
        assert L.vit_engine_cls_attention_host_images(eng._h, recs, nn, p, sp, r) == VIT_ERR_ARG
        still_fine()
    assert L.vit_engine_attention_row_elems(eng._h, spec(0)) == cfg.num_heads * cfg.tokens
    assert L.vit_engine_attention_row_elems(eng._h, spec(1)) == cfg.tokens
    assert L.vit_engine_attention_row_elems(eng._h, spec(2)) == 0 and L.vit_engine_attention_row_elems(eng._h, spec(-1)) == 0
    assert L.vit_engine_attention_row_elems(eng._h, spec(0, 1)) == 0 and L.vit_engine_attention_row_elems(eng._h, None) == 0
    assert L.vit_engine_attention_row_elems(None, spec(0)) == 0
    assert eng.attention_shape(n, "heads") == (n, cfg.num_heads, cfg.tokens) and eng.attention_shape(n, "head_mean") == (n, cfg.tokens)
    with pytest.raises(B.VitError):
        eng.attention_shape(n, 2)
    with pytest.raises(B.VitError):
        eng.cls_attention(imgs, 9)
    still_fine()


def test_read_logits_after_an_attention_call_is_an_error(engines):
    eng = engines("tiny", max_batch=4)
    n = 3
    imgs = synth.make_images(eng.cfg, n, 410)
    before = eng.forward(imgs)
    logits = eng.logits(n)
    for kind in KINDS:
        eng.cls_attention(imgs, kind)
        with pytest.raises(B.VitError):  # nothing wrote logits: an error, not the previous call's
            eng.logits(1)
    assert same_bits(eng.forward(imgs), before)
    assert same_bits(eng.logits(n), logits)
