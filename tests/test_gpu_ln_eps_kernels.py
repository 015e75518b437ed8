"""The `_eps` siblings of every LayerNorm entry point (include/vit_hip_kernels.h, VITHIP_LN_EPS): at eps 1e-5 (CLIP) and 1e-12 (HF
ViTModel) against a float64 model, at dims 64, 768 and 2048, on rows that include some of variance 1e-5 .. 1e-7 -- where the three
epsilons give results more than 10 % apart, which is asserted.  With the double 1e-6 each sibling gives the BITS of its old entry
point (the old one is a call of the sibling), and the in-place LayerNorm gives the bits of the out-of-place one.

Bars: 2e-5 of max |ref| for normalised rows, the bar of every fp32 row op here (tests/test_gpu_ops.py REL); 2e-6 relative for the
(rstd, mean) pairs, the bar of tests/test_gpu_ops.py's row-statistics test; one bf16 rounding (2^-8 relative) on top for bf16 stores.
The small-variance rows are centred (|mean| << spread), so E[x^2] - mean^2 cancels nothing and fp32 sums of <= 2048 terms stay within
those bars (relative error of a sum ~ sqrt(dim) * 2^-24 = 2.7e-6, of rstd half that).
"""
import numpy as np
import pytest

import strided as S
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

REL, PAIR_REL = 2e-5, 2e-6
DIMS = [64, 768, 2048]
EPSES = [1e-5, 1e-12]
IMAGES, TOKENS = 3, 21          # pooled kernels and taps: 63 rows; 20 patch tokens = a full segment of 16 and a ragged one
ROWS = IMAGES * TOKENS


def u(k, shape, a, seed=911):
    return synth.uniform(seed, k, int(np.prod(shape)), -a, a).reshape(shape)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint16)


_cache = {}


def operands(dim):
    """x [ROWS][dim]: ordinary rows (spread 3, offset 0.5) with every third row scaled down to a variance of 1e-5, 1e-6 or 1e-7."""
    if dim not in _cache:
        x = u(1, (ROWS, dim), 3.0) + 0.5
        small = np.arange(ROWS) % 3 == 1
        target = np.array([1e-5, 1e-6, 1e-7])[(np.arange(ROWS) // 3) % 3]
        c = u(2, (ROWS, dim), 1.0)
        c = c - c.mean(1, keepdims=True)
        c = c / c.std(1, keepdims=True) * np.sqrt(target)[:, None]
        x[small] = c[small]
        gamma, beta = (1.0 + u(3, (dim,), 0.5)).astype(np.float32), u(4, (dim,), 0.5)
        _cache[dim] = (np.ascontiguousarray(x, np.float32), gamma, beta, small)
    return _cache[dim]


def stats64(x, eps):
    x = x.astype(np.float64)
    mean = x.mean(1)
    var = (x * x).mean(1) - mean * mean
    return mean, 1.0 / np.sqrt(var + eps)


def ln64(x, gamma, beta, eps):
    mean, rstd = stats64(x, eps)
    return (x.astype(np.float64) - mean[:, None]) * rstd[:, None] * gamma + beta


def close(got, ref, rel=REL):
    err, scale = float(np.abs(got.astype(np.float64) - ref).max()), float(np.abs(ref).max())
    assert err <= rel * scale, f"max err {err:.3e} > {rel} * {scale:.3e}"


@pytest.mark.parametrize("dim", DIMS)
def test_the_three_epsilons_are_more_than_ten_percent_apart_on_the_small_rows(dim):
    x, gamma, beta, small = operands(dim)
    r = {eps: stats64(x[small], eps)[1] for eps in (1e-5, 1e-6, 1e-12)}
    assert (r[1e-6] / r[1e-5] > 1.1).any() and (r[1e-12] / r[1e-6] > 1.1).any()
    assert (r[1e-12] / r[1e-5] > 1.1).all()
    got = {eps: B.layernorm(x, gamma, beta, eps=eps)[small] for eps in (1e-5, 1e-6, 1e-12)}
    d56 = np.abs(got[1e-5] - got[1e-6]).max() / np.abs(got[1e-6] - beta).max()
    d612 = np.abs(got[1e-6] - got[1e-12]).max() / np.abs(got[1e-12] - beta).max()
    assert d56 > 0.1 and d612 > 0.1, (d56, d612)


@pytest.mark.parametrize("eps", EPSES)
@pytest.mark.parametrize("dim", DIMS)
def test_layernorm_siblings(dim, eps):
    x, gamma, beta, _ = operands(dim)
    ref = ln64(x, gamma, beta, eps)
    close(B.layernorm(x, gamma, beta, eps=eps), ref)
    got16 = B.from_bf16_bits(B.layernorm_bf16out(x, gamma, beta, eps=eps)).astype(np.float64)
    assert (np.abs(got16 - ref) <= 2.0 ** -8 * np.abs(ref) + REL * np.abs(ref).max()).all()
    # the default: the bits of the old entry points
    assert np.array_equal(bits(B.layernorm(x, gamma, beta, eps=1e-6)), bits(B.layernorm(x, gamma, beta)))
    assert np.array_equal(B.layernorm_bf16out(x, gamma, beta, eps=1e-6), B.layernorm_bf16out(x, gamma, beta))
    assert not np.array_equal(bits(B.layernorm(x, gamma, beta, eps=eps)), bits(B.layernorm(x, gamma, beta)))


@pytest.mark.parametrize("eps", EPSES + [None])
@pytest.mark.parametrize("dim", DIMS)
def test_layernorm_in_place_gives_the_bits_of_out_of_place(dim, eps):
    """y == x, ldy == ldx, also with ldx > dim and a sentinel in the gap and around the frame."""
    x, gamma, beta, _ = operands(dim)
    want = B.layernorm(x, gamma, beta, eps=eps)
    assert np.array_equal(bits(B.layernorm(x, gamma, beta, eps=eps, in_place=True)), bits(want))
    out = {}
    got = B.layernorm(x, gamma, beta, eps=eps, in_place=True, ldx=dim + 12, frames=S, out=out)
    out["y"].check()
    assert np.array_equal(bits(got), bits(want))


def test_layernorm_refuses_overlap_that_is_not_in_place_and_bad_epsilons():
    dim = 64
    x, gamma, beta, _ = operands(dim)
    L = B.lib()
    dx, dg, db = B.DeviceArray.from_numpy(np.concatenate([x, x])), B.DeviceArray.from_numpy(gamma), B.DeviceArray.from_numpy(beta)
    fn, _ = B._ln_fn("vithip_layernorm_f32", 1e-5)
    INVALID = 1
    assert fn(None, dx.ptr, dim, dx.ptr + 4 * dim, dim, dg.ptr, db.ptr, ROWS, dim, 1e-5) == INVALID          # shifted by one row
    assert fn(None, dx.ptr, dim, dx.ptr, 2 * dim, dg.ptr, db.ptr, ROWS, dim, 1e-5) == INVALID               # same base, another stride
    assert L.vithip_layernorm_f32(None, dx.ptr, dim, dx.ptr + 4 * dim, dim, dg.ptr, db.ptr, ROWS, dim) == INVALID
    for bad in (0.0, -1e-6, float("nan"), float("inf")):
        assert fn(None, dx.ptr, dim, dx.ptr + 4 * ROWS * dim, dim, dg.ptr, db.ptr, ROWS, dim, bad) == INVALID, bad
        with pytest.raises(B.VitError):
            B.rowstats_f32(x, eps=bad)
        with pytest.raises(B.VitError):
            B.rowstats_bf16(x, eps=bad)
        with pytest.raises(B.VitError):
            B.tap(x, gamma, beta, IMAGES, TOKENS, "cls", eps=bad)
        with pytest.raises(B.VitError):
            B.layernorm_pool(x, gamma, beta, IMAGES, TOKENS, eps=bad)
        with pytest.raises(B.VitError):
            B.pool_layernorm(x, gamma, beta, IMAGES, TOKENS, eps=bad)
    assert fn(None, dx.ptr, dim, dx.ptr + 4 * ROWS * dim, dim, dg.ptr, db.ptr, ROWS, dim, 1e-5) == 0     # disjoint: fine
    B.hip_check(L.vithip_device_sync(), "sync")


@pytest.mark.parametrize("eps", EPSES)
@pytest.mark.parametrize("dim", DIMS)
def test_row_statistics_siblings_and_their_finalisers(dim, eps):
    x, gamma, beta, _ = operands(dim)
    mean, rstd = stats64(x, eps)
    got = B.rowstats_f32(x, eps=eps)                                    # (rstd, mean)
    assert np.abs(got[:, 0] - rstd).max() <= PAIR_REL * rstd.max() and np.abs(got[:, 1] - mean).max() <= PAIR_REL * np.abs(mean).max() + 1e-6
    assert np.abs(got[:, 0] / rstd - 1).max() <= 1e-5
    x16, got16 = B.rowstats_bf16(x, eps=eps)                            # (rstd, mean * rstd)
    assert np.abs(got16[:, 0] / rstd - 1).max() <= 1e-5 and np.abs(got16[:, 1] - mean * rstd).max() <= 1e-5 * np.abs(mean * rstd).max() + 1e-6
    assert np.array_equal(x16, B.to_bf16_bits(x))
    assert np.array_equal(bits(B.rowstats_f32(x, eps=1e-6)), bits(B.rowstats_f32(x)))
    d16, dflt = B.rowstats_bf16(x, eps=1e-6), B.rowstats_bf16(x)
    assert np.array_equal(bits(d16[1]), bits(dflt[1])) and np.array_equal(d16[0], dflt[0])
    # the finalisers, on partial sums made here in the strips' layouts: [dim / 64][rows][2] (fp32 fold), [ln_strips][rows][2] (bf16)
    x64 = x.astype(np.float64)
    for f32, strips in ((True, dim // 64), (False, B.ln_strips(dim))):
        part = np.zeros((strips, ROWS, 2), np.float32)
        width = 64
        for k in range(dim // width):
            seg = x64[:, k * width:(k + 1) * width]
            part[k % strips, :, 0] += seg.sum(1).astype(np.float32)
            part[k % strips, :, 1] += (seg * seg).sum(1).astype(np.float32)
        fin = B.rowstats_finalize(part, dim, eps=eps, f32=f32)
        want_second = mean if f32 else mean * rstd
        assert np.abs(fin[:, 0] / rstd - 1).max() <= 1e-5
        assert np.abs(fin[:, 1] - want_second).max() <= 1e-5 * np.abs(want_second).max() + 1e-6
        assert np.array_equal(bits(B.rowstats_finalize(part, dim, eps=1e-6, f32=f32)), bits(B.rowstats_finalize(part, dim, f32=f32)))


@pytest.mark.parametrize("eps", EPSES)
def test_the_residual_gemm_hands_its_epsilon_to_the_statistics_behind_it(eps):
    """vithip_gemm_args.stats_eps: the pairs of the stored rows are vithip_rowstats_f32_eps of them, bit for bit, whether the
    persistent walk takes the sums in its epilogue (tile 9) or a pass behind the GEMM does (tile 10); 0 is the default 1e-6."""
    M, N, K = 300, 128, 128
    A, W, b, R = u(5, (M, K), 0.01), u(6, (N, K), 0.05), np.zeros(N, np.float32), u(7, (M, N), 0.003)
    for tile in (9, 10):
        rs = {}
        Cm = B.gemm(A, W, b, residual=R, epilogue=B.EPI_BIAS_RESIDUAL, tile=tile, row_stats=rs, stats_eps=eps)
        assert rs["in_epilogue"] == (tile == 9)
        assert np.array_equal(bits(rs["rows"]), bits(B.rowstats_f32(Cm, eps=eps))), tile
        rs0 = {}
        B.gemm(A, W, b, residual=R, epilogue=B.EPI_BIAS_RESIDUAL, tile=tile, row_stats=rs0)
        assert np.array_equal(bits(rs0["rows"]), bits(B.rowstats_f32(Cm))) and not np.array_equal(bits(rs0["rows"]), bits(rs["rows"]))
    with pytest.raises(B.VitError):
        B.gemm(A, W, b, residual=R, epilogue=B.EPI_BIAS_RESIDUAL, row_stats={}, stats_eps=-1.0)


@pytest.mark.parametrize("eps", EPSES)
@pytest.mark.parametrize("dim", DIMS)
def test_pooled_blocks_and_taps(dim, eps):
    x, gamma, beta, _ = operands(dim)
    y = ln64(x, gamma, beta, eps).reshape(IMAGES, TOKENS, dim)
    close(B.layernorm_pool(x, gamma, beta, IMAGES, TOKENS, eps=eps), y[:, 1:].mean(1))
    unit = y[:, 1:].mean(1)
    unit = unit / np.linalg.norm(unit, axis=1, keepdims=True)
    close(B.layernorm_pool(x, gamma, beta, IMAGES, TOKENS, l2_normalize=True, eps=eps), unit)
    pooled = x.astype(np.float64).reshape(IMAGES, TOKENS, dim)[:, 1:].mean(1)
    close(B.pool_layernorm(x, gamma, beta, IMAGES, TOKENS, eps=eps), ln64(pooled, gamma, beta, eps))
    for layout, ref in (("cls", y[:, 0]), ("tokens", y), ("patches", y[:, 1:]), ("map", y[:, 1:].transpose(0, 2, 1))):
        close(B.tap(x, gamma, beta, IMAGES, TOKENS, layout, eps=eps), ref)
        # the tap is the LayerNorm kernel's arithmetic: the same bits as the rows of vithip_layernorm_f32_eps
    assert np.array_equal(bits(B.tap(x, gamma, beta, IMAGES, TOKENS, "tokens", eps=eps).reshape(ROWS, dim)), bits(B.layernorm(x, gamma, beta, eps=eps)))
    # the default: the bits of the old entry points
    assert np.array_equal(bits(B.layernorm_pool(x, gamma, beta, IMAGES, TOKENS, eps=1e-6)), bits(B.layernorm_pool(x, gamma, beta, IMAGES, TOKENS)))
    assert np.array_equal(bits(B.pool_layernorm(x, gamma, beta, IMAGES, TOKENS, eps=1e-6)), bits(B.pool_layernorm(x, gamma, beta, IMAGES, TOKENS)))
    for layout in ("cls", "map"):
        assert np.array_equal(bits(B.tap(x, gamma, beta, IMAGES, TOKENS, layout, eps=1e-6)), bits(B.tap(x, gamma, beta, IMAGES, TOKENS, layout)))
