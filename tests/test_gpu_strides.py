"""Leading dimensions, aliasing and write footprints of the kernels, in the memory shapes the engine calls them with.

Every operand sits in a frame (tests/strided.py): 256 guard rows either side and the pad columns hold a NaN sentinel.  Each case
asserts (a) the window equals, bit for bit, what the same entry point returns for the same values in dense layout with the same
tuning fields, (b) the window meets the bar the op already has against a reference that is not the library (float64, or the
oracle), and (c) nothing outside the window of any output frame changed and the result holds no NaN.  Every access a correct or
an incorrect kernel can make here stays inside a frame: no size passed to a kernel exceeds what its frames hold.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import strided as S
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

INVALID = 1  # hipErrorInvalidValue


def u(k, shape, a, seed=4242):
    n = int(np.prod(shape))
    return synth.uniform(seed, k, n, -a, a).reshape(shape)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(S.as_bits(a), S.as_bits(b))


def checked(out):
    """(c): every output frame of a call untouched outside its window, its window written and NaN-free."""
    for name, f in out.items():
        w = f.check()
        if f.dtype != np.int32:
            assert not S.has_nan(w), f"{name}: a NaN in the result"


def close_f32(got, ref64):
    err = float(np.abs(got.astype(np.float64) - ref64).max())
    assert err <= 2e-5 * float(np.abs(ref64).max()), err       # the fp32 GEMM bar of test_gpu_ops.py


def close_bf16(got_bits, ref64):
    err = np.abs(B.from_bf16_bits(got_bits).astype(np.float64) - ref64)
    assert (err <= 2.0 ** -8 * np.abs(ref64) + 1e-5).all(), float(err.max())   # the bf16 bar of test_gpu_bf16.py


def gelu64(x):
    from scipy.special import erf
    return 0.5 * x * (1.0 + erf(x / np.sqrt(2.0)))


def refused(call, *frames):
    """The call answers hipErrorInvalidValue and leaves every listed output frame as it was (window included)."""
    with pytest.raises(B.VitError) as e:
        call()
    assert e.value.code == INVALID, e.value
    for f in [g for f in frames for g in (f.values() if isinstance(f, dict) else [f])]:   # (a dict: the wrapper's `out`, filled by the call)
        arr = f.download()
        f.assert_untouched(arr)
        assert (S.as_bits(f.window(arr)) == S.SENTINEL[f.dtype]).all(), "a refused call wrote its output"


# ---- the frame on the device: what .ptr addresses is the window ---------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.uint16, np.int32])
def test_frame_pointer_addresses_the_window(dtype):
    """A device-to-device copy of one window row through .ptr lands in, and comes from, window coordinates (offset base)."""
    data = (np.arange(5 * 6).reshape(5, 6) + 1).astype(dtype)
    src, dst = S.framed(data, ld=9, offset=3), S.out_frame(5, 6, ld=11, dtype=dtype, offset=1)
    item = np.dtype(dtype).itemsize
    for r in range(5):
        B.hip_check(B.lib().vithip_memcpy_d2d(dst.ptr + r * dst.ld * item, src.ptr + r * src.ld * item, 6 * item, None), "d2d")
    assert bits_equal(dst.check(), data)
    src.assert_untouched()


# ---- vithip_gemm_f32 ----------------------------------------------------------------------------------------------------------

SHAPES = [(313, 200, 128), (5, 10, 128)]
TILES = [(t, B.ARITH_F32, False) for t in (0, 6, 7, 8, 9, 10, 11, 12)] + [(t, B.ARITH_SPLIT3, False) for t in (0, 9, 10, 11)] + \
        [(t, B.ARITH_SPLIT3, True) for t in (0, 9, 10, 11)]


def layout(name, N, K):
    if name == "padded":
        return dict(lda=K + 4, ldw=K + 8, ldc=N + 4, ldr=N + 12)
    if name == "row subset":   # the pruned last layer: class rows of [n][T][K] in, of [n][T][N] out
        return dict(lda=7 * K, ldc=5 * N, ldr=5 * N)
    return dict(ldc=N + 1, ldr=N + 3, offset=1)   # "odd": the 10-class head's store, bases one float off a 16-byte boundary


@functools.lru_cache(maxsize=None)
def gemm_operands(M, N, K):
    A, W, b, R = u(1, (M, K), 1.0), u(2, (N, K), 0.05), u(3, (N,), 0.1), u(4, (M, N), 2.0)
    lin = A.astype(np.float64) @ W.astype(np.float64).T + b
    return A, W, b, R, {B.EPI_BIAS: lin, B.EPI_BIAS_GELU: gelu64(lin), B.EPI_BIAS_RESIDUAL: lin + R}


@functools.lru_cache(maxsize=None)
def gemm_dense(M, N, K, epi, tile, arith, w_split):
    A, W, b, R, _ = gemm_operands(M, N, K)
    return B.gemm(A, W, b, residual=R if epi == B.EPI_BIAS_RESIDUAL else None, epilogue=epi, tile=tile, arith=arith, w_split=w_split)


@pytest.mark.parametrize("lay", ["padded", "row subset", "odd"])
@pytest.mark.parametrize("tile,arith,w_split", TILES)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_f32_layouts(M, N, K, tile, arith, w_split, lay):
    """Every tile code, both arithmetics and the pre-split image (made from the W with ldw > K), every epilogue, the residual in
    a buffer of its own (ldr != ldc where the layout has one) and in place.  W's frame holds NaN behind row N - 1: no tile may
    use what it finds there."""
    A, W, b, R, ref = gemm_operands(M, N, K)
    kw = dict(tile=tile, arith=arith, w_split=w_split, frames=S, **layout(lay, N, K))
    for epi, in_place in ((B.EPI_BIAS, False), (B.EPI_BIAS_GELU, False), (B.EPI_BIAS_RESIDUAL, False), (B.EPI_BIAS_RESIDUAL, True)):
        out = {}
        k = dict(kw)
        if in_place:
            k.pop("ldr")
        got = B.gemm(A, W, b, residual=R if epi == B.EPI_BIAS_RESIDUAL else None, epilogue=epi, in_place=in_place, out=out, **k)
        checked(out)
        assert bits_equal(got, gemm_dense(M, N, K, epi, tile, arith, w_split)), (epi, in_place)
        close_f32(got, ref[epi])


@pytest.mark.parametrize("lay", ["padded", "row subset", "odd"])
@pytest.mark.parametrize("tile,arith", [(0, 0), (9, 0), (10, 0), (11, 0), (12, 0), (9, 1), (10, 1)])
def test_gemm_f32_fold_consumer_with_gathered_rows(tile, arith, lay):
    """The consumer side of the LayerNorm fold as the engine builds it: the (rstd, mean) pairs of the class rows gathered out of a
    [M][T][2] buffer by vithip_gather_rows_f32, with the column sums and with the centred weight."""
    M, N, K, T = 313, 200, 128, 5
    x = (u(5, (M, 1), 2.0) + u(6, (M, K), 1.0)).astype(np.float32)
    gamma, beta = (1.0 + u(7, (K,), 0.5)).astype(np.float32), u(8, (K,), 0.5)
    W, b = u(9, (N, K), 0.05), u(10, (N,), 0.1)
    stats = B.rowstats_f32(x)
    out = {}
    rows = B.gather_rows(stats, src_stride=2 * T, dst_stride=2, frames=S, out=out)
    checked(out)
    assert bits_equal(rows, stats)
    x64, r64 = x.astype(np.float64), rows.astype(np.float64)
    ref = ((x64 - r64[:, 1:]) * r64[:, :1] * gamma + beta) @ W.astype(np.float64).T + b
    for fold in (B.ln_fold_weights_f32, B.ln_fold_weights_f32_centered):
        Wf, cs, bf = fold(W, b, gamma, beta)
        ln = (rows, cs if fold is B.ln_fold_weights_f32 else None)
        for epi in (B.EPI_BIAS, B.EPI_BIAS_GELU):
            out = {}
            got = B.gemm(x, Wf, bf, epilogue=epi, tile=tile, arith=arith, ln=ln, frames=S, out=out, **layout(lay, N, K))
            checked(out)
            assert bits_equal(got, B.gemm(x, Wf, bf, epilogue=epi, tile=tile, arith=arith, ln=ln))
            if epi == B.EPI_BIAS:   # the bar of test_gpu_lnfold.py: the product chain's rounding, amplified by rstd, + 2e-5
                amp = r64[:, :1] * (np.abs(x64) @ np.abs(Wf.astype(np.float64)).T)
                err = np.abs(got - ref)
                assert (err <= 8 * 2.0 ** -24 * amp + 2e-5).all(), float((err - 8 * 2.0 ** -24 * amp).max())


@pytest.mark.parametrize("tile,scratch,in_place", [(9, True, False), (9, True, True), (10, False, False), (10, True, True)])
def test_gemm_f32_row_statistics_producer_with_ldc(tile, scratch, in_place):
    """stats_out of a C with ldc = 5 * N: from the epilogue (tile 9 with scratch) and from the trailing vithip_rowstats_f32(C, ldc)."""
    M, N, K = 313, 256, 128
    A, W, b, R = u(11, (M, K), 1.0), u(12, (N, K), 0.05), u(13, (N,), 0.1), u(14, (M, N), 2.0)
    dense = B.gemm(A, W, b, residual=R, epilogue=B.EPI_BIAS_RESIDUAL, tile=tile)
    rs, out = {"scratch": scratch}, {}
    got = B.gemm(A, W, b, residual=R, epilogue=B.EPI_BIAS_RESIDUAL, tile=tile, row_stats=rs, ldc=5 * N, in_place=in_place,
                 lda=7 * K, frames=S, out=out)
    assert rs["in_epilogue"] == int(tile == 9 and scratch)
    stats = out["stats"].check()
    out["C"].check()
    for f in out.values():
        f.assert_untouched()
    assert not S.has_nan(got) and not S.has_nan(stats)
    assert bits_equal(got, dense)
    assert bits_equal(stats, B.rowstats_f32(dense))
    close_f32(got, A.astype(np.float64) @ W.astype(np.float64).T + b + R)


def test_gemm_f32_hand_over_in_padded_frames_in_place():
    """Tile 9 with a workspace on a shape whose last round is partial, so that owners take helper pieces (and, with
    handover_test = 1, withdraw and recompute): padded layout, residual in place.  K = 512: the walk hands pieces over from 16
    K-steps on (persistent_piece_steps), at K = 128 there are none to test."""
    cu = B.device_info(0)["compute_units"]
    K, N = 512, 768
    M = 128 * ((2 * cu + 88 + 5) // 6)
    owners = (M // 128) * (N // 128) - 2 * cu
    assert 0 < owners < 2 * cu - owners
    A, W, b, R = u(15, (M, K), 1.0), u(16, (N, K), 0.05), u(17, (N,), 0.1), u(18, (M, N), 2.0)
    dense = B.gemm(A, W, b, residual=R, epilogue=B.EPI_BIAS_RESIDUAL, tile=10)
    close_f32(dense, A.astype(np.float64) @ W.astype(np.float64).T + b + R)
    for late in (0, 1):
        out, st = {}, {}
        got = B.gemm(A, W, b, residual=R, epilogue=B.EPI_BIAS_RESIDUAL, tile=9, workspace=True, handover_test=late, stats=st,
                     in_place=True, lda=K + 4, ldw=K + 8, ldc=N + 4, frames=S, out=out)
        checked(out)
        assert bits_equal(got, dense), late
        assert st["taken"] + st["recomputed"] == owners, (st, late)
        if late:
            assert st["recomputed"] > 0, st


def _gemm_args(fA, fW, fb, fR, fC, M, N, K, epi, over):
    v = dict(A=fA.ptr, lda=fA.ld, W=fW.ptr, ldw=fW.ld, bias=fb.ptr, residual=fR.ptr if fR else None, ldr=fR.ld if fR else N,
             C=fC.ptr, ldc=fC.ld, M=M, N=N, K=K, epilogue=epi)
    v.update(over)
    return v


def test_gemm_f32_refusals():
    """Each ld below its width, lda / ldw off their multiple of 4 and A / W off their 16 bytes are refused with the output
    untouched.  (ldc, ldr, C, residual and bias have no multiple or alignment beyond a float's: see test_gemm_f32_layouts, odd.)"""
    M, N, K = 37, 40, 64
    A, W, b, R, _ = gemm_operands(M, N, K)
    fA, fW, fb, fR = S.framed(A, K + 4), S.framed(W, K + 4), S.framed(b), S.framed(R, N + 4)
    fC = S.out_frame(M, N, N + 4)
    L = B.lib()
    bad = [dict(lda=K - 4), dict(ldw=K - 4), dict(ldc=N - 1), dict(ldr=N - 1), dict(lda=K + 2), dict(ldw=K + 2),
           dict(A=fA.ptr + 4), dict(W=fW.ptr + 4), dict(A=None), dict(W=None), dict(bias=None), dict(C=None), dict(residual=None),
           dict(M=0), dict(N=0), dict(K=0)]
    for over in bad:
        args = B.CGemmArgs(**_gemm_args(fA, fW, fb, fR, fC, M, N, K, B.EPI_BIAS_RESIDUAL, over))
        refused(lambda: B.hip_check(L.vithip_gemm_f32(None, C.byref(args)), str(over)), fC)
    args = B.CGemmArgs(**_gemm_args(fA, fW, fb, fR, fC, M, N, K, B.EPI_BIAS_RESIDUAL, {}))   # and the frames themselves are fine
    B.hip_check(L.vithip_gemm_f32(None, C.byref(args)), "vithip_gemm_f32")
    assert bits_equal(fC.check(), B.gemm(A, W, b, residual=R, epilogue=B.EPI_BIAS_RESIDUAL))


# ---- vithip_gemm_bf16 ---------------------------------------------------------------------------------------------------------

def bf16_layout(name, N, K):   # lda, ldw % 8 and ldc, ldr % 4 are the header's multiples
    if name == "padded":
        return dict(lda=K + 8, ldw=K + 16, ldc=N + 4, ldr=N + 12)
    return dict(lda=5 * K, ldc=3 * N, ldr=3 * N)


@functools.lru_cache(maxsize=None)
def bf16_operands(M, N, K):
    Ab, Wb = B.to_bf16_bits(u(21, (M, K), 1.0)), B.to_bf16_bits(u(22, (N, K), 0.08))
    b, R = u(23, (N,), 0.1), u(24, (M, N), 2.0)
    lin = B.from_bf16_bits(Ab).astype(np.float64) @ B.from_bf16_bits(Wb).astype(np.float64).T + b
    return Ab, Wb, b, R, lin


@pytest.mark.parametrize("lay", ["padded", "row subset"])
@pytest.mark.parametrize("K", [192, 128])
@pytest.mark.parametrize("variant", [1, 2])
def test_gemm_bf16_layouts(variant, K, lay):
    M, N = 531, 260
    Ab, Wb, b, R, lin = bf16_operands(M, N, K)
    kw = dict(variant=variant, frames=S, **bf16_layout(lay, N, K))
    for epi in (B.BF16_EPI_BF16, B.BF16_EPI_BF16_GELU):
        out = {}
        k = dict(kw)
        k.pop("ldr")
        got = B.gemm_bf16(Ab, Wb, b, epilogue=epi, out=out, **k)
        checked(out)
        assert bits_equal(got, B.gemm_bf16(Ab, Wb, b, epilogue=epi, variant=variant))
        close_bf16(got, lin if epi == B.BF16_EPI_BF16 else gelu64(lin))
    dense = B.gemm_bf16(Ab, Wb, b, residual=R, epilogue=B.BF16_EPI_F32_RESIDUAL, variant=variant)
    for in_place in (False, True):
        out = {}
        k = dict(kw)
        if in_place:
            k.pop("ldr")
        got = B.gemm_bf16(Ab, Wb, b, residual=R, epilogue=B.BF16_EPI_F32_RESIDUAL, in_place=in_place, out=out, **k)
        checked(out)
        assert bits_equal(got, dense), in_place
        close_f32(got, lin + R)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("K", [192, 128])
def test_gemm_bf16_producer_frames(K, in_place):
    """Variant 2 as the producer of the LayerNorm fold: C, x16 and the row partials, each in a frame (ldx16 = N + 12: the header
    wants ldx16 % 8 == 0, and N % 8 == 4 -- so the reference layout is not dense either: exact buffers with the smallest legal
    ldx16 = N + 4)."""
    M, N = 531, 260
    Ab, Wb, b, R, lin = bf16_operands(M, N, K)
    dC, d16, dP = B.gemm_bf16(Ab, Wb, b, residual=R, epilogue=B.BF16_EPI_F32_RESIDUAL, variant=2, ln_producer=True, ldx16=N + 4)
    out = {}
    gC, g16, gP = B.gemm_bf16(Ab, Wb, b, residual=R, epilogue=B.BF16_EPI_F32_RESIDUAL, variant=2, ln_producer=True, in_place=in_place,
                              lda=K + 8, ldw=K + 16, ldc=N + 4, ldx16=N + 12, frames=S, out=out)
    for name in ("C", "x16", "partials"):
        out[name].assert_untouched()
    assert not S.has_nan(gC) and not S.has_nan(g16) and not S.has_sentinel(gC) and not S.has_sentinel(g16)
    assert bits_equal(gC, dC) and bits_equal(g16, d16)
    assert bits_equal(B.rowstats_finalize(gP, N), B.rowstats_finalize(dP, N))
    close_f32(gC, lin + R)
    close_bf16(g16, gC.astype(np.float64))


@pytest.mark.parametrize("lay", ["padded", "row subset"])
def test_gemm_bf16_fold_consumer_with_gathered_rows(lay):
    M, N, K, T = 531, 260, 192, 3
    x = (u(25, (M, 1), 2.0) + u(26, (M, K), 1.0)).astype(np.float32)
    gamma, beta = (1.0 + u(27, (K,), 0.5)).astype(np.float32), u(28, (K,), 0.5)
    W, b = u(29, (N, K), 0.05), u(30, (N,), 0.1)
    x16, stats = B.rowstats_bf16(x)
    out = {}
    rows = B.gather_rows(stats, src_stride=2 * T, dst_stride=2, frames=S, out=out)
    checked(out)
    assert bits_equal(rows, stats)
    Wf, cs, bf = B.ln_fold_weights(W, b, gamma, beta)
    k = bf16_layout(lay, N, K)
    k.pop("ldr")
    for epi in (B.BF16_EPI_BF16, B.BF16_EPI_BF16_GELU):
        out = {}
        got = B.gemm_bf16(x16, Wf, bf, epilogue=epi, variant=2, ln_rows=rows, ln_colsum=cs, frames=S, out=out, **k)
        checked(out)
        assert bits_equal(got, B.gemm_bf16(x16, Wf, bf, epilogue=epi, variant=2, ln_rows=stats, ln_colsum=cs))


def test_gemm_bf16_refusals():
    M, N, K = 37, 40, 128
    Ab, Wb, b, R, _ = bf16_operands(M, N, K)
    fA, fW, fb, fR = S.framed(Ab, K + 8), S.framed(Wb, K + 8), S.framed(b), S.framed(R, N + 4)
    fC = S.out_frame(M, N, N + 4)
    L = B.lib()
    L.vithip_gemm_bf16.argtypes = [C.c_void_p, C.POINTER(B.CGemmBf16Args)]
    bad = [dict(lda=K - 8), dict(ldw=K - 8), dict(ldc=N - 4), dict(ldr=N - 4), dict(lda=K + 4), dict(ldw=K + 4), dict(ldc=N + 2),
           dict(ldr=N + 2), dict(A=fA.ptr + 8), dict(W=fW.ptr + 8), dict(bias=fb.ptr + 4), dict(C=fC.ptr + 4),
           dict(residual=fR.ptr + 4), dict(A=None), dict(C=None), dict(residual=None), dict(M=0)]
    for over in bad:
        args = B.CGemmBf16Args(**_gemm_args(fA, fW, fb, fR, fC, M, N, K, B.BF16_EPI_F32_RESIDUAL, over))
        refused(lambda: B.hip_check(L.vithip_gemm_bf16(None, C.byref(args)), str(over)), fC)


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------

LN_SHAPES = [(5, 4), (37, 192), (9, 1280), (3, 1984), (2, 2048), (16389, 64)]   # the last: the grid-stride loop wraps


@functools.lru_cache(maxsize=None)
def ln_operands(rows, dim):
    x = u(31, (rows, dim), 3.0) + 0.5
    return x.astype(np.float32), synth.uniform(4242, 32, dim, 0.5, 1.5), u(33, (dim,), 0.5)


@pytest.mark.parametrize("ldx_of", [lambda d: d + 4, lambda d: 6 * d], ids=["ldx=dim+4", "ldx=6*dim"])
@pytest.mark.parametrize("rows,dim", LN_SHAPES)
def test_layernorm_f32_frames(oracle, rows, dim, ldx_of):
    x, g, b = ln_operands(rows, dim)
    out = {}
    got = B.layernorm(x, g, b, ldx=ldx_of(dim), ldy=dim + 8, frames=S, out=out)
    checked(out)
    assert bits_equal(got, B.layernorm(x, g, b))
    ref = oracle.layer_norm(x, g, b)
    err = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())
    assert err <= 2e-5 * float(np.abs(ref).max()), err       # the bar of test_layernorm


@pytest.mark.parametrize("ldx_of", [lambda d: d + 4, lambda d: 6 * d], ids=["ldx=dim+4", "ldx=6*dim"])
@pytest.mark.parametrize("rows,dim", LN_SHAPES)
def test_layernorm_bf16out_frames(oracle, rows, dim, ldx_of):
    x, g, b = ln_operands(rows, dim)
    out = {}
    got = B.layernorm_bf16out(x, g, b, ldx=ldx_of(dim), ldy=dim + 8, frames=S, out=out)
    checked(out)
    assert bits_equal(got, B.layernorm_bf16out(x, g, b))
    close_bf16(got, oracle.layer_norm(x, g, b).astype(np.float64))


@pytest.mark.parametrize("entry", ["vithip_layernorm_f32", "vithip_layernorm_f32_bf16out"])
def test_layernorm_refusals(entry):
    rows, dim = 5, 64
    x, g, b = ln_operands(rows, dim)
    fx, fg, fb = S.framed(x, dim + 4), S.framed(g), S.framed(b)
    fy = S.out_frame(rows, dim, dim + 8, np.float32 if entry == "vithip_layernorm_f32" else np.uint16)
    fn = getattr(B.lib(), entry)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    good = [fx.ptr, fx.ld, fy.ptr, fy.ld, fg.ptr, fb.ptr, rows, dim]
    for i, v in ((1, dim - 4), (3, dim - 4), (1, dim + 2), (3, dim + 2), (0, fx.ptr + 4), (2, fy.ptr + 4), (4, fg.ptr + 4), (5, fb.ptr + 4),
                 (0, None), (2, None), (4, None), (5, None), (6, 0), (7, 0), (7, 2052)):
        a = list(good)
        a[i] = v
        refused(lambda: B.hip_check(fn(None, *a), f"{entry} argument {i} = {v}"), fy)


# ---- row statistics -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ldx_of", [lambda d: d + 4, lambda d: 6 * d], ids=["ldx=dim+4", "ldx=6*dim"])
@pytest.mark.parametrize("rows,dim", [(37, 192), (9, 1280), (3, 1984), (2, 2048), (16389, 64)])
def test_rowstats_f32_frames(rows, dim, ldx_of):
    x, _, _ = ln_operands(rows, dim)
    out = {}
    got = B.rowstats_f32(x, ldx=ldx_of(dim), frames=S, out=out)
    checked(out)
    assert bits_equal(got, B.rowstats_f32(x))
    x64 = x.astype(np.float64)
    mean = x64.mean(1)
    assert np.allclose(got[:, 1], mean, rtol=0, atol=2e-5 * float(np.abs(x64).max()))
    assert np.allclose(got[:, 0], 1.0 / np.sqrt(x64.var(1) + 1e-6), rtol=2e-5, atol=0)


@pytest.mark.parametrize("ldx_of", [lambda d: d + 4, lambda d: 6 * d], ids=["ldx=dim+4", "ldx=6*dim"])
@pytest.mark.parametrize("rows,dim", LN_SHAPES)
def test_rowstats_bf16_frames(rows, dim, ldx_of):
    x, _, _ = ln_operands(rows, dim)
    out = {}
    g16, grows = B.rowstats_bf16(x, ldx=ldx_of(dim), ldx16=dim + 8, frames=S, out=out)
    checked(out)
    d16, drows = B.rowstats_bf16(x)
    assert bits_equal(g16, d16) and bits_equal(grows, drows)
    assert bits_equal(g16, B.to_bf16_bits(x))          # round to nearest even: the host model is exact
    x64 = x.astype(np.float64)
    rstd = 1.0 / np.sqrt(x64.var(1) + 1e-6)
    assert np.allclose(grows[:, 0], rstd, rtol=2e-5, atol=0)
    assert np.allclose(grows[:, 1], x64.mean(1) * rstd, rtol=0, atol=2e-5 * float(np.abs(x64).max() * rstd.max()))


def test_rowstats_refusals():
    rows, dim = 5, 64
    x, _, _ = ln_operands(rows, dim)
    L = B.lib()
    fx, f16, fr = S.framed(x, dim + 4), S.out_frame(rows, dim, dim + 8, np.uint16), S.out_frame(rows, 2)
    L.vithip_rowstats_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int]
    good = [fx.ptr, fx.ld, fr.ptr, rows, dim]
    for i, v in ((1, dim - 4), (0, fx.ptr + 2), (2, fr.ptr + 4), (0, None), (2, None), (3, 0), (4, 0), (4, 32), (4, 2112)):
        a = list(good)
        a[i] = v
        refused(lambda: B.hip_check(L.vithip_rowstats_f32(None, *a), f"vithip_rowstats_f32 argument {i} = {v}"), fr)
    L.vithip_rowstats_bf16.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int]
    good = [fx.ptr, fx.ld, f16.ptr, f16.ld, fr.ptr, rows, dim]
    for i, v in ((1, dim - 4), (3, dim - 4), (1, dim + 2), (3, dim + 2), (0, fx.ptr + 4), (2, f16.ptr + 4), (4, fr.ptr + 4),
                 (0, None), (2, None), (4, None), (5, 0), (6, 0)):
        a = list(good)
        a[i] = v
        refused(lambda: B.hip_check(L.vithip_rowstats_bf16(None, *a), f"vithip_rowstats_bf16 argument {i} = {v}"), f16, fr)


# ---- vithip_gather_rows_f32 ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows,width,src_stride,dst_stride", [(1, 2, 2, 2), (11, 2, 2 * 197, 2), (300, 7, 19, 9), (5, 256, 300, 256)])
def test_gather_rows(rows, width, src_stride, dst_stride):
    """Exact against numpy slicing of a [rows][src_stride] buffer whose other columns hold values of their own."""
    full = u(41, (rows, src_stride), 5.0)
    f_src, f_dst = S.framed(full), S.out_frame(rows, width, dst_stride)
    L = B.lib()
    L.vithip_gather_rows_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int]
    B.hip_check(L.vithip_gather_rows_f32(None, f_src.ptr, src_stride, f_dst.ptr, dst_stride, rows, width), "vithip_gather_rows_f32")
    assert bits_equal(f_dst.check(), full[:, :width])
    f_src.assert_untouched()
    out = {}   # and through the wrapper, the source's other columns being NaN padding
    got = B.gather_rows(full[:, :width], src_stride=src_stride, dst_stride=dst_stride, frames=S, out=out)
    checked(out)
    assert bits_equal(got, full[:, :width])


def test_gather_rows_refusals():
    src = u(42, (6, 4), 1.0)
    for kw in (dict(src_stride=3), dict(dst_stride=3), dict(null="src"), dict(null="dst"), dict(rows=0), dict(width=0)):
        out = {}
        refused(lambda: B.gather_rows(src, frames=S, out=out, **kw), out)
        assert "dst" in out


# ---- vithip_softmax_top1_f32 --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("classes", [1, 2, 63, 64, 65, 255, 256, 257, 1000, 1025])
@pytest.mark.parametrize("rows", [1, 37])
def test_softmax_top1_frames(oracle, rows, classes):
    logits = u(51, (rows, classes), 6.0)
    dprobs, dlabel, dprob = B.softmax_top1(logits)
    for want_label, want_prob in ((True, True), (False, True), (True, False), (False, False)):
        out = {}
        probs, label, prob = B.softmax_top1(logits, ld_logits=classes + 3, ld_probs=classes + 5, want_label=want_label,
                                            want_prob=want_prob, frames=S, out=out)
        out["probs"].check()
        for name, want in (("label", want_label), ("prob", want_prob)):
            arr = out[name].download()
            out[name].assert_untouched(arr)
            assert S.has_sentinel(out[name].window(arr)) == (not want), (name, want)   # a NULL output is not written anywhere
        assert not S.has_nan(probs) and bits_equal(probs, dprobs)
        if want_label:
            assert np.array_equal(label, dlabel)
        if want_prob:
            assert bits_equal(prob, dprob)
    for r in range(rows):
        ref = oracle.softmax(logits[r])
        assert float(np.abs(dprobs[r] - ref).max()) <= 1e-6
        assert dlabel[r] == int(ref.argmax())
        assert dprob[r] == dprobs[r, dlabel[r]]


def test_softmax_top1_huge_logits_in_frames():
    logits = u(52, (4, 300), 1.0)
    logits[0, 7], logits[1, 299], logits[2, :] = 3e4, 3e4, -3e4
    logits[2, 258], logits[3, :] = 3e4, 3e4
    logits[3, 100] = -3e4
    out = {}
    probs, label, prob = B.softmax_top1(logits, ld_logits=303, ld_probs=305, frames=S, out=out)
    checked(out)
    assert np.isfinite(probs).all()
    assert list(label[:3]) == [7, 299, 258] and list(prob[:3]) == [1.0, 1.0, 1.0]
    assert [int((probs[r] == 1.0).sum()) for r in range(3)] == [1, 1, 1]
    assert label[3] == 0 and probs[3, 100] == 0.0


@pytest.mark.parametrize("first,second", [(1, 33), (5, 70), (3, 259), (255, 256)])
def test_softmax_top1_ties_take_the_first_index(first, second):
    """Two lanes of one wave, two waves, two iterations of one thread, either side of the 256-thread boundary."""
    logits = u(53, (3, 300), 1.0)
    logits[:, first] = logits[:, second] = 2.5
    out = {}
    _, label, _ = B.softmax_top1(logits, ld_logits=303, ld_probs=305, frames=S, out=out)
    checked(out)
    assert list(label) == [first] * 3


def test_softmax_top1_refusals():
    logits = u(54, (3, 10), 1.0)
    fl, fp, flab, fpr = S.framed(logits, 13), S.out_frame(3, 10, 15), S.out_frame(3, 1, dtype=np.int32), S.out_frame(3, 1)
    fn = B.lib().vithip_softmax_top1_f32
    good = [fl.ptr, fl.ld, fp.ptr, fp.ld, flab.ptr, fpr.ptr, 3, 10]
    for i, v in ((1, 9), (3, 9), (0, None), (2, None), (6, 0), (7, 0)):
        a = list(good)
        a[i] = v
        refused(lambda: B.hip_check(fn(None, *a), f"vithip_softmax_top1_f32 argument {i} = {v}"), fp, flab, fpr)


# ---- partial-row attention ----------------------------------------------------------------------------------------------------

ATT_SHAPES = [(2, 197, 3), (3, 33, 1), (1, 224, 2), (2, 5, 2)]


@functools.lru_cache(maxsize=None)
def attention_full(kind, n, T, heads):
    qkv = u(61, (n * T, 3 * heads * 64), 1.5)
    if kind == "f32":
        return qkv, B.attention(qkv, n, T, heads)
    bits = B.to_bf16_bits(qkv)
    return bits, B.attention_bf16io(bits, n, T, heads, q_scaled=kind == "qscaled")


@pytest.mark.parametrize("n,T,heads", ATT_SHAPES)
@pytest.mark.parametrize("kind", ["f32", "bf16io", "qscaled"])
def test_attention_partial_rows_footprint(oracle, kind, n, T, heads):
    """Rows 0..q_rows-1 of every image equal the full call's bit for bit; rows q_rows..T-1 of every image, and everything
    around the buffer, keep the sentinel."""
    D = heads * 64
    qkv, full = attention_full(kind, n, T, heads)
    if kind == "f32":      # (b): the full call against the oracle, at the bar of test_attention; the partial rows equal it bitwise
        for i in range(n):
            blk = qkv[i * T:(i + 1) * T]
            q, k, v = (np.ascontiguousarray(blk[:, j * D:(j + 1) * D]) for j in range(3))
            ref = oracle.attention_core(q, k, v, heads)
            assert float(np.abs(full[i * T:(i + 1) * T] - ref).max()) <= 1e-5 * max(1.0, float(np.abs(ref).max()))
    for q_rows in (1, 2, 31, 32, 33, T - 1):
        if not 1 <= q_rows < T:
            continue
        out = {}
        if kind == "f32":
            got = B.attention_rows(qkv, n, T, heads, q_rows, frames=S, out=out)
        else:
            got = B.attention_bf16io_rows(qkv, n, T, heads, q_rows, q_scaled=kind == "qscaled", frames=S, out=out)
        out["out"].assert_untouched()
        got, want = got.reshape(n, T, D), full.reshape(n, T, D)
        assert bits_equal(got[:, :q_rows], want[:, :q_rows]), q_rows
        assert not S.has_nan(got[:, :q_rows])
        assert (S.as_bits(got[:, q_rows:]) == S.SENTINEL[got.dtype]).all(), f"q_rows {q_rows}: rows behind it were written"


@pytest.mark.parametrize("kind", ["f32", "bf16io", "qscaled"])
def test_attention_partial_rows_refusals(kind):
    n, T, heads = 1, 5, 1
    qkv, _ = attention_full(kind, 2, 5, 2)
    qkv = np.ascontiguousarray(qkv[:T, :3 * 64])
    for q_rows in (0, -1, T + 1):
        out = {}
        call = (lambda: B.attention_rows(qkv, n, T, heads, q_rows, frames=S, out=out)) if kind == "f32" else \
            (lambda: B.attention_bf16io_rows(qkv, n, T, heads, q_rows, q_scaled=kind == "qscaled", frames=S, out=out))
        refused(call, out)
        assert "out" in out
