"""A non-finite image changes only its own outputs: every other image of the batch keeps the bits it has in a clean batch.

Every other module feeds the kernels finite, well-scaled data, and on such data two assumptions cannot fail: (i) a masked key has
probability exactly 0, so whatever its K/V row holds in LDS does not matter -- true only while that row is finite, 0 * Inf and
0 * NaN being NaN on the matrix pipe; (ii) an LDS-DMA whose source lies past the descriptor's range writes zeros.  A kernel that
walks several (image, head) items per workgroup, or that meets LDS another launch filled, can then carry one image's NaN into
another image's rows.

The method is the same everywhere (isolation() below): launch on a clean seeded batch (Y), overwrite ALL the data of a seeded random
half of the images (rows, for the row-wise kernels) with the poison, launch again (Y'), launch on the clean batch once more.  Y is
finite; every clean image has the bits of Y in Y'; every poisoned image's block of Y' holds a non-finite value (the poison was
read); the third launch equals Y (the poisoned launch left nothing behind).  Poisoning half the images needs no knowledge of how a
kernel maps items to workgroups: for any static walk a quarter of the consecutive item pairs of a workgroup are (poisoned, clean)
-- provided workgroups do take several items, which every walking case asserts from the device's CU count (items >= 1.5 x the
largest grid the kernel uses).

The clean data is one pool of 2^24 seeded values U(-1.5, 1.5), repeated to the size a case needs (no image's length divides the
pool's, so no two images are equal); the Q columns are not pre-scaled for the q_scaled entries -- the scores stay within +-40 in
the exponent, finite either way.
"""
import math

import numpy as np
import pytest

from engine_helpers import device_forward
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

BF16_POISONS = [pytest.param(0x7FC0, id="nan"), pytest.param(0x7F80, id="inf")]
F32_POISONS = [pytest.param(float("nan"), id="nan"), pytest.param(float("inf"), id="inf"), pytest.param(3e38, id="3e38")]

_pool = {}
_clean = {}   # the clean launch's output of the latest case, shared by its poisons: {"key": ..., "Y": ...}


def cus() -> int:
    if "cus" not in _pool:
        _pool["cus"] = int(B.device_info(0)["compute_units"])
    return _pool["cus"]


def pool(dtype, count, seed=0):
    """`count` clean values: fp32 U(-1.5, 1.5), or their bf16 bit patterns (truncated: it is input data)."""
    if "f32" not in _pool:
        _pool["f32"] = np.random.default_rng(2024).uniform(-1.5, 1.5, 1 << 24).astype(np.float32)
        _pool["bf16"] = (_pool["f32"].view(np.uint32) >> 16).astype(np.uint16)
    src = _pool["bf16" if np.dtype(dtype) == np.uint16 else "f32"]
    return np.resize(np.roll(src, -977 * seed) if seed else src, count)


def floats(a):
    a = np.asarray(a)
    return B.from_bf16_bits(a) if a.dtype == np.uint16 else a.astype(np.float64)


def raw(a, n):
    return np.ascontiguousarray(a).reshape(n, -1).view(np.uint8)


def walk_items(heads, per_cu=1):
    """Images for a launch of at least 1.5 items per workgroup of the largest grid (per_cu x CUs)."""
    return math.ceil(1.5 * per_cu * cus() / heads)


def assert_walks(n, heads, per_cu=1):
    assert n * heads >= 1.5 * per_cu * cus(), f"{n * heads} items on {per_cu * cus()} workgroups: nobody walks from one image to the next"


def isolation(key, run, data, n, poison, seed=1):
    """run(data) -> an array whose leading n blocks are the n images' (rows') outputs; data's leading n blocks are their inputs."""
    if _clean.get("key") != key:
        _clean.clear()
        _clean.update(key=key, Y=run(data))
    Y = _clean["Y"]
    assert np.isfinite(floats(Y)).all(), "the clean launch is not finite"
    bad = np.sort(np.random.default_rng(seed).permutation(n)[:n // 2])
    good = np.setdiff1d(np.arange(n), bad)
    assert bad.size and good.size
    dirty = np.array(data, copy=True)
    dirty.reshape(n, -1)[bad] = poison
    Y2 = run(dirty)
    differ = np.flatnonzero((raw(Y2, n)[good] != raw(Y, n)[good]).any(axis=1))
    assert differ.size == 0, f"{differ.size} of {good.size} clean blocks changed, first: block {good[differ[0]]}"
    finite_in = np.isfinite(np.asarray(floats(np.array([poison], dirty.dtype)))).all()
    if not finite_in:   # (3e38 goes in finite and overflows inside, or does not: nothing is promised about its own block)
        dead = ~np.isfinite(floats(Y2)).reshape(n, -1)
        assert dead[bad].any(axis=1).all(), "a poisoned block came out finite: the poison was not read"
    assert np.array_equal(raw(run(data), n), raw(Y, n)), "the launch after the poisoned one differs from the first"


# ---- (a) attention entries --------------------------------------------------------------------------------------------

def bf16_attention(n, T, heads, **kw):
    return lambda bits: B.attention_bf16io(bits.reshape(n * T, 3 * heads * 64), n, T, heads, **kw)


STREAM_TOKENS = [225, 257, 300, 330, 370, 400, 448, 470, 500, 540, 560, 577, 620, 650, 690, 704]   # 8..22 key tiles: every chunk plan


@pytest.mark.parametrize("poison", BF16_POISONS)
@pytest.mark.parametrize("qs", [False, True], ids=["plain-q", "qscaled"])
@pytest.mark.parametrize("T,heads", [(T, 1) for T in STREAM_TOKENS] + [(300, 3), (577, 2)])
def test_streamed_attention(T, heads, qs, poison):
    """attention_bf16_stream_kernel (225..704 tokens): one workgroup per CU walks (image, head) items and streams K/V through a ring
    of two 128-key slots.  A chunk of three 32-key tiles leaves the slot's fourth tile as the last four-tile chunk wrote it -- with
    an odd chunk count (10 key tiles = 4 + 3 + 3) that is another item's rows -- and the second sub-chunk's P.V reads it."""
    n = walk_items(heads)
    assert_walks(n, heads)
    isolation(("stream", T, heads, qs), bf16_attention(n, T, heads, q_scaled=qs), pool(np.uint16, n * T * 3 * heads * 64), n, poison)


def test_streamed_token_counts_cover_every_key_tile_count():
    assert sorted({(t + 31) // 32 for t in STREAM_TOKENS}) == list(range(8, 23))


@pytest.mark.parametrize("poison", BF16_POISONS)
@pytest.mark.parametrize("qs", [False, True], ids=["plain-q", "qscaled"])
@pytest.mark.parametrize("T,heads", [(33, 1), (50, 2), (197, 1), (197, 3), (224, 1)])
def test_resident_bf16_attention_item_walk(T, heads, qs, poison):
    """attention_bf16_kernel: the next item's K/V arrive by LDS-DMA in a second LDS image; up to 96 tokens two workgroups per CU."""
    per_cu = 2 if T <= 96 else 1
    n = walk_items(heads, per_cu)
    assert_walks(n, heads, per_cu)
    isolation(("resident16", T, heads, qs), bf16_attention(n, T, heads, q_scaled=qs), pool(np.uint16, n * T * 3 * heads * 64), n, poison)


@pytest.mark.parametrize("poison", BF16_POISONS)
@pytest.mark.parametrize("qs", [False, True], ids=["plain-q", "qscaled"])
def test_chunked_bf16_attention(qs, poison):
    """Beyond 704 tokens: one workgroup per (head, image, query blocks); nothing walks, LDS is per workgroup."""
    n, T, heads = 6, 740, 2
    isolation(("chunked16", qs), bf16_attention(n, T, heads, q_scaled=qs), pool(np.uint16, n * T * 3 * heads * 64), n, poison)


@pytest.mark.parametrize("poison", BF16_POISONS)
@pytest.mark.parametrize("T", [197, 300])
def test_bf16_attention_with_fp32_arithmetic(T, poison):
    n, heads = 8, 2
    isolation(("f32math", T), bf16_attention(n, T, heads, f32math=True), pool(np.uint16, n * T * 3 * heads * 64), n, poison)


@pytest.mark.parametrize("poison", F32_POISONS)
@pytest.mark.parametrize("T,heads,small", [(5, 1, False), (130, 1, False), (197, 1, False), (197, 2, False), (224, 1, False),
                                           (130, 2, True), (197, 2, True), (224, 2, True), (300, 2, True), (577, 2, True)])
def test_fp32_attention(T, heads, small, poison):
    """attention_f32_resident_kernel up to 224 tokens: the item walk on a full device, and with a small batch the instantiation that
    cuts a head's query blocks over up to four workgroups (the tail block is cut in four by keys either way); the chunked kernel
    beyond (one workgroup per head, image and query blocks)."""
    n = 4 if small else walk_items(heads)
    if not small:
        assert_walks(n, heads)
    run = lambda q: B.attention(q.reshape(n * T, 3 * heads * 64), n, T, heads)
    isolation(("f32", T, heads, small), run, pool(np.float32, n * T * 3 * heads * 64), n, poison)


@pytest.mark.parametrize("poison", F32_POISONS)
def test_fp32_attention_class_rows_only(poison):
    n, T, heads = walk_items(1), 197, 1
    assert_walks(n, heads)
    run = lambda q: B.attention_rows(q.reshape(n * T, 3 * heads * 64), n, T, heads, 1)
    isolation(("f32rows",), run, pool(np.float32, n * T * 3 * heads * 64), n, poison)


@pytest.mark.parametrize("poison", BF16_POISONS)
def test_bf16_attention_class_rows_only(poison):
    n, T, heads = walk_items(1), 197, 1
    assert_walks(n, heads)
    run = lambda q: B.attention_bf16io_rows(q.reshape(n * T, 3 * heads * 64), n, T, heads, 1)
    isolation(("bf16rows",), run, pool(np.uint16, n * T * 3 * heads * 64), n, poison)


@pytest.mark.parametrize("poison", F32_POISONS)
@pytest.mark.parametrize("head_mean", [False, True], ids=["heads", "mean"])
@pytest.mark.parametrize("T", [197, 577])
def test_cls_attention_f32(T, head_mean, poison):
    n, heads = 12, 3
    run = lambda q: B.cls_attention(q.reshape(n * T, 3 * heads * 64), n, T, heads, head_mean)
    isolation(("cls32", T, head_mean), run, pool(np.float32, n * T * 3 * heads * 64), n, poison)


@pytest.mark.parametrize("poison", BF16_POISONS)
@pytest.mark.parametrize("head_mean", [False, True], ids=["heads", "mean"])
@pytest.mark.parametrize("T", [197, 577])
def test_cls_attention_bf16(T, head_mean, poison):
    n, heads = 12, 3
    run = lambda q: B.cls_attention_bf16(q.reshape(n * T, 3 * heads * 64), n, T, heads, head_mean)
    isolation(("cls16", T, head_mean), run, pool(np.uint16, n * T * 3 * heads * 64), n, poison)


# ---- (b) what another launch left in LDS ----------------------------------------------------------------------------------

def test_resident_bf16_attention_after_a_launch_of_nans():
    """The resident kernels stage a ragged last key tile by LDS-DMA whose rows past the image's last lie outside the descriptor's
    range, expect zeros in LDS for them, and multiply those rows by P = 0.  Should the hardware skip the LDS write instead, the rows
    hold what the previous item -- or the previous KERNEL on that CU -- left there.  So: the clean ragged launch (197 tokens) in a
    fresh state, a launch of the same instantiation at the full tile count (224) whose every value is NaN, the clean launch again:
    the same bits.  Both launches fill every CU twice.  A detector, not a proof: which CU runs which workgroup, and what else ran
    in between, is not ours to fix."""
    heads, n = 1, 2 * cus()
    clean = pool(np.uint16, n * 197 * 3 * 64).reshape(n * 197, 3 * 64)
    fresh = B.attention_bf16io(clean, n, 197, heads, q_scaled=True)
    assert np.isfinite(floats(fresh)).all()
    nans = np.full((n * 224, 3 * 64), 0x7FC0, np.uint16)
    assert np.isnan(floats(B.attention_bf16io(nans, n, 224, heads, q_scaled=True))).all()
    assert np.array_equal(B.attention_bf16io(clean, n, 197, heads, q_scaled=True), fresh)


@pytest.mark.parametrize("T_full", [208, 224])
def test_resident_fp32_attention_after_a_launch_of_nans(T_full):
    """As above for attention_f32_resident_kernel (16-key tiles: 197 tokens are 13 of them, 208 the same instantiation full; 224 the
    next one, whose LDS image reaches further)."""
    heads, n = 1, 2 * cus()
    clean = pool(np.float32, n * 197 * 3 * 64).reshape(n * 197, 3 * 64)
    fresh = B.attention(clean, n, 197, heads)
    assert np.isfinite(fresh).all()
    nans = np.full((n * T_full, 3 * 64), np.nan, np.float32)
    assert np.isnan(B.attention(nans, n, T_full, heads)).all()
    assert np.array_equal(B.attention(clean, n, 197, heads).view(np.uint32), fresh.view(np.uint32))


# ---- (c) kernels whose rows are independent ---------------------------------------------------------------------------------

GM, GN, GK = 300, 200, 128   # ragged in M and N for every tile shape, K a whole step of every kernel (tile 12: 128)


def gemm_operands(N=GN, K=GK, M=GM):
    return pool(np.float32, N * K, 1).reshape(N, K) * np.float32(0.05), pool(np.float32, N, 2) * np.float32(0.1), pool(np.float32, M * N, 3).reshape(M, N)


@pytest.mark.parametrize("poison", F32_POISONS)
@pytest.mark.parametrize("tile,arith,w_split", [(0, 0, False), (9, 0, False), (10, 0, False), (11, 0, False), (12, 0, False),
                                                (9, 1, False), (10, 1, False), (9, 1, True), (10, 1, True)])
def test_gemm_f32_rows(tile, arith, w_split, poison):
    W, b, _ = gemm_operands()
    run = lambda A: B.gemm(A, W, b, tile=tile, arith=arith, w_split=w_split)
    isolation(("gemm", tile, arith, w_split), run, pool(np.float32, GM * GK).reshape(GM, GK), GM, poison)


@pytest.mark.parametrize("poison", F32_POISONS)
@pytest.mark.parametrize("epi", ["bias", "gelu", "residual", "fold"])
def test_gemm_f32_epilogues_and_fold_consumer(epi, poison):
    """The three epilogues, and the consumer side of the LayerNorm fold (the rows' statistics come from vithip_rowstats_f32 on the
    same, possibly poisoned, rows)."""
    W, b, R = gemm_operands()
    if epi == "fold":
        gamma, beta = 1.0 + pool(np.float32, GK, 4) * np.float32(0.3), pool(np.float32, GK, 5) * np.float32(0.3)
        Wf, colsum, bias_f = B.ln_fold_weights_f32(W, b, gamma, beta)
        run = lambda A: B.gemm(A, Wf, bias_f, ln=(B.rowstats_f32(A), colsum))
    elif epi == "residual":
        run = lambda A: B.gemm(A, W, b, residual=R, epilogue=B.EPI_BIAS_RESIDUAL)
    else:
        run = lambda A: B.gemm(A, W, b, epilogue=B.EPI_BIAS_GELU if epi == "gelu" else B.EPI_BIAS)
    isolation(("gemm-epi", epi), run, pool(np.float32, GM * GK).reshape(GM, GK), GM, poison)


@pytest.mark.parametrize("poison", F32_POISONS)
def test_gemm_f32_persistent_walk_with_late_helpers(poison):
    """The persistent walk with a workspace: tiles of the partial last round start on a helper workgroup and their accumulators
    travel to the owner (handover_test = 1: the helpers run late, owners withdraw and recompute) -- pieces of poisoned and clean
    row blocks pass through the same workspace.  The shape of test_gemm_helper_pieces_are_bit_identical_and_reusable."""
    M, N, K = 128 * 100, 768, 768
    W, b, _ = gemm_operands(N, K, 1)
    st = {}
    run = lambda A: B.gemm(A, W, b, tile=9, workspace=True, handover_test=1, stats=st)
    isolation(("gemm-walk",), run, pool(np.float32, M * K).reshape(M, K), M, poison)
    assert st["taken"] + st["recomputed"] > 0, st


@pytest.mark.parametrize("poison", BF16_POISONS)
@pytest.mark.parametrize("variant,role", [(v, r) for v in (1, 2) for r in ("plain", "gelu", "producer", "consumer") if v == 2 or r in ("plain", "gelu")])
def test_gemm_bf16_rows(variant, role, poison):
    """Both kernels (1 two-stage, 2 ping-pong), with and without GELU; the ping-pong kernel also as the producer and the consumer of
    the LayerNorm fold (the two-stage kernel has neither side).  The GELU of the ping-pong kernel is built on v_min / v_max, which
    drop a NaN: it has to carry the NaN of a poisoned row into the output itself (relu_keep_nan, csrc/vit_gemm_common.hpp)."""
    W, b, R = gemm_operands()
    Wb = B.to_bf16_bits(W)
    if role == "producer":     # C (fp32), bf16(C) and the rows' partial sums [strips][M][2]
        def run(A):
            Cf, x16, part = B.gemm_bf16(A, Wb, b, residual=R, epilogue=B.BF16_EPI_F32_RESIDUAL, variant=variant, ln_producer=True)
            return np.concatenate([Cf, B.from_bf16_bits(x16), part.transpose(1, 0, 2).reshape(GM, -1)], axis=1)
    elif role == "consumer":   # the rows' pairs come from vithip_rowstats_bf16 on the same, possibly poisoned, rows
        gamma, beta = 1.0 + pool(np.float32, GK, 4) * np.float32(0.3), pool(np.float32, GK, 5) * np.float32(0.3)
        Wf, colsum, bias_f = B.ln_fold_weights(W, b, gamma, beta)

        def run(A):
            x16, rows = B.rowstats_bf16(B.from_bf16_bits(A))
            return B.gemm_bf16(x16, Wf, bias_f, epilogue=B.BF16_EPI_BF16, variant=variant, ln_rows=rows, ln_colsum=colsum)
    else:
        run = lambda A: B.gemm_bf16(A, Wb, b, epilogue=B.BF16_EPI_BF16_GELU if role == "gelu" else B.BF16_EPI_BF16, variant=variant)
    isolation(("gemm16", variant, role), run, pool(np.uint16, GM * GK).reshape(GM, GK), GM, poison)


@pytest.mark.parametrize("poison", F32_POISONS)
@pytest.mark.parametrize("op", ["layernorm", "layernorm_bf16out", "rowstats_f32", "rowstats_bf16", "softmax_top1"])
def test_row_kernels(op, poison):
    rows, dim = 301, 192
    gamma, beta = 1.0 + pool(np.float32, dim, 4) * np.float32(0.3), pool(np.float32, dim, 5) * np.float32(0.3)
    if op == "rowstats_bf16":
        def run(x):
            x16, rs = B.rowstats_bf16(x)
            return np.concatenate([B.from_bf16_bits(x16), rs], axis=1)
    elif op == "softmax_top1":
        def run(x):
            probs, label, prob = B.softmax_top1(x)
            return np.concatenate([probs, label.astype(np.float32)[:, None], prob[:, None]], axis=1)
    else:
        run = {"layernorm": lambda x: B.layernorm(x, gamma, beta), "layernorm_bf16out": lambda x: B.layernorm_bf16out(x, gamma, beta),
               "rowstats_f32": B.rowstats_f32}[op]
    isolation(("row", op), run, pool(np.float32, rows * dim).reshape(rows, dim), rows, poison)


@pytest.mark.parametrize("poison", F32_POISONS)
@pytest.mark.parametrize("norm", [True, False], ids=["norm", "copy"])
@pytest.mark.parametrize("layout", ["cls", "tokens", "patches", "map"])
def test_tap(layout, norm, poison):
    images, tokens, dim = 6, 10, 192    # 9 patches: the map's channel runs are unaligned
    gamma, beta = 1.0 + pool(np.float32, dim, 4) * np.float32(0.3), pool(np.float32, dim, 5) * np.float32(0.3)
    run = lambda x: B.tap(x.reshape(images * tokens, dim), gamma if norm else None, beta if norm else None, images, tokens, layout)
    isolation(("tap", layout, norm), run, pool(np.float32, images * tokens * dim), images, poison)


GENERAL = synth.ModelConfig(img_size=42, patch_size=14, in_chans=1, num_classes=10, embed_dim=64, depth=1, num_heads=1, hidden_dim=64)


@pytest.mark.parametrize("poison", F32_POISONS)
@pytest.mark.parametrize("kernel", ["f32", "general", "bf16", "bf16_implicit"])
def test_patch_embed(kernel, poison):
    cfg, n = (GENERAL, 6) if kernel == "general" else (synth.VIT_SMALL, 6)
    W = [synth.make_weight(cfg, i, 5) for i in range(4)]
    run = {"f32": lambda im: B.patch_embed(cfg, im, W[1], W[2], W[0], W[3]),
           "general": lambda im: B.patch_embed_general(cfg, im, W[1], W[2], W[0], W[3]),
           "bf16": lambda im: B.patch_embed_bf16(cfg, im, W[1], W[2], W[0], W[3]),
           "bf16_implicit": lambda im: B.patch_embed_bf16(cfg, im, W[1], W[2], W[0], W[3], implicit=True)}[kernel]
    images = pool(np.float32, n * cfg.in_chans * cfg.img_size ** 2).reshape(n, cfg.in_chans, cfg.img_size, cfg.img_size)
    isolation(("embed", kernel), run, images, n, poison)


# ---- (d) engines ------------------------------------------------------------------------------------------------------------

STREAMED = synth.ModelConfig(img_size=272, num_classes=10, embed_dim=128, depth=2, num_heads=2, hidden_dim=256)   # 290 tokens: 4 + 3 + 3
B16_NARROW = synth.ModelConfig(img_size=224, num_classes=10, embed_dim=128, depth=2, num_heads=2, hidden_dim=256)  # 197 tokens
OUTPUTS = ["forward", "features-cls", "features-mean", "cls_attention", "intermediate"]
_weights = {}


def engine_outputs(eng, images, which):
    """The output `which` of one call on `images`, [n][...]: the forward through the device entry with its top-1 label and
    probability in two more columns, everything else through the host entries."""
    n = images.shape[0]
    if which == "forward":
        d = B.DeviceArray.from_numpy(images)
        probs, label, prob = device_forward(eng, d, n)
        d.free()
        return np.concatenate([probs, label.astype(np.float32)[:, None], prob[:, None]], axis=1)
    if which.startswith("features"):
        return eng.features(images, which.split("-")[1])
    if which == "cls_attention":
        return eng.cls_attention(images, "heads")
    return eng.intermediate(images, [eng.cfg.depth - 1], "tokens")


def engine_case(cfg, per_cu, poison, dtype, ln_fold=0, lanes=1, use_graph=False):
    """One pixel of every poisoned image is poisoned; every output kind in turn.  A lane's attention launch holds n / lanes images
    (the engine cuts a chunk evenly) of cfg.num_heads items each: n is sized so that this is 1.5 items per workgroup."""
    n = lanes * walk_items(cfg.num_heads, per_cu)
    assert_walks(n // lanes, cfg.num_heads, per_cu)
    if cfg not in _weights:
        _weights.clear()
        _weights[cfg] = synth.make_weights(cfg, 1234)
    per = cfg.in_chans * cfg.img_size ** 2
    images = pool(np.float32, n * per).reshape(n, cfg.in_chans, cfg.img_size, cfg.img_size)
    bad = np.sort(np.random.default_rng(3).permutation(n)[:n // 2])
    good = np.setdiff1d(np.arange(n), bad)
    dirty = images.copy()
    dirty.reshape(n, per)[bad, per // 3] = poison
    eng = B.Engine(cfg, max_batch=n, dtype=dtype, ln_fold=ln_fold, lanes=lanes, use_graph=use_graph)
    try:
        eng.load_weights(_weights[cfg])
        for which in OUTPUTS:
            Y = engine_outputs(eng, images, which)
            assert np.isfinite(Y).all(), which
            Y2 = engine_outputs(eng, dirty, which)
            differ = np.flatnonzero((raw(Y2, n)[good] != raw(Y, n)[good]).any(axis=1))
            assert differ.size == 0, f"{which}: {differ.size} of {good.size} clean images changed, first: image {good[differ[0]]}"
            if not np.isfinite(poison):
                assert (~np.isfinite(Y2)).reshape(n, -1)[bad].any(axis=1).all(), f"{which}: a poisoned image came out finite"
            assert np.array_equal(raw(engine_outputs(eng, images, which), n), raw(Y, n)), f"{which}: the call after the poisoned one differs"
    finally:
        eng.close()


@pytest.mark.parametrize("poison", F32_POISONS)
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("ln_fold", [0, -1], ids=["ln-folded", "ln-kernels"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_engine_at_290_tokens(dtype, ln_fold, lanes, use_graph, poison):
    """The bf16 engine's attention is the streamed kernel with the 4 + 3 + 3 chunk plan here (the fp32 engine's the chunked one)."""
    engine_case(STREAMED, 1, poison, dtype, ln_fold, lanes, use_graph)


@pytest.mark.parametrize("poison", F32_POISONS)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("cfg,per_cu", [(synth.VIT_TINY, 2), (B16_NARROW, 1)], ids=["17-tokens", "197-tokens"])
def test_engine_on_the_resident_paths(cfg, per_cu, dtype, poison):
    engine_case(cfg, per_cu, poison, dtype)
