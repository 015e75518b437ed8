"""The QuickGELU epilogue (VITHIP_EPI_BIAS_QGELU, VITHIP_BF16_EPI_BF16_QGELU: q(y) = y / (1 + exp(-1.702 y))) through every GEMM kernel
that carries it: the 16x16x4 latency tile, the generic tiles in both arithmetics, the persistent walk with and without the pre-split
weight image and with the hand-over, the LayerNorm fold's consumer form, the two-stage bf16 kernel and the ping-pong one.  Shapes are
the smallest that reach each kernel by the dispatcher's rules (csrc/vit_gemm.hip dispatch(), vithip_gemm_bf16); M is ragged, N ends in
a partial tile, ldc > N and the columns beyond N keep their sentinel (tests/strided.py).  Reference: float64 GEMM + bias, then the
float64 function.  The GEMM part takes the bars of the GELU twins (tests/test_gpu_ops.py close(), tests/test_gpu_bf16.py)."""
import numpy as np
import pytest

import strided as S
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

SPLIT = B.ARITH_SPLIT3


def u(k, shape, a, seed=4242):
    return synth.uniform(seed, k, int(np.prod(shape)), -a, a).reshape(shape)


def q64(y):
    """float64 model: y * sigmoid(1.702 y), written so that neither tail overflows into a NaN."""
    y = np.asarray(y, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return y / (1.0 + np.exp(-1.702 * y))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint16)


def run_f32(A, W, b, **kw):
    """One launch into a padded, sentinel-filled frame (ldc = N + 8): the window, after the footprint check."""
    out = {}
    got = B.gemm(A, W, b, epilogue=B.EPI_BIAS_QGELU, ldc=W.shape[0] + 8, frames=S, out=out, **kw)
    out["C"].check()
    return got


def close_f32(got, A, W, b):
    ref = q64(A.astype(np.float64) @ W.astype(np.float64).T + b)
    err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    print(f"{A.shape} x {W.shape}: max err {err:.3g} of {scale:.3g}")
    assert err <= 2e-5 * scale


# ---- fp32 ------------------------------------------------------------------------------------------------------------------------

def test_latency_kernel():
    """A handful of rows, K % 128 == 0, fewer than 160 tiles of 64 x 64: auto takes vit_gemm_latency.hip; tile 12 names it."""
    M, N, K = 5, 200, 128
    A, W, b = u(1, (M, K), 1.0), u(2, (N, K), 0.2), u(3, (N,), 0.1)
    got = run_f32(A, W, b)
    close_f32(got, A, W, b)
    assert np.array_equal(bits(got), bits(run_f32(A, W, b, tile=12)))
    assert np.array_equal(bits(got), bits(run_f32(A, W, b, tile=11)))   # the 32x32x2 kernels give the same bits


@pytest.mark.parametrize("arith", [B.ARITH_F32, SPLIT], ids=["f32", "split3"])
def test_generic_tiles_and_the_small_persistent_walk(arith):
    """394 x 200 x 96: auto is the 64x64 tile (K % 128 != 0 keeps it off the latency kernel); every tile code of the arithmetic --
    tile 9 is the persistent walk without pieces, with w_split on the pre-split image -- gives the same bits."""
    M, N, K = 394, 200, 96
    A, W, b = u(4, (M, K), 1.0), u(5, (N, K), 0.2), u(6, (N,), 0.1)
    ref = run_f32(A, W, b, arith=arith)
    close_f32(ref, A, W, b)
    for tile in ((6, 7, 8, 9, 10, 11) if arith == B.ARITH_F32 else (9, 10, 11)):
        assert np.array_equal(bits(run_f32(A, W, b, tile=tile, arith=arith)), bits(ref)), tile
    if arith == SPLIT:
        assert np.array_equal(bits(run_f32(A, W, b, tile=9, arith=arith, w_split=True)), bits(ref))
        assert not np.array_equal(bits(ref), bits(run_f32(A, W, b)))   # the split really ran


@pytest.mark.parametrize("arith,w_split", [(B.ARITH_F32, False), (SPLIT, False), (SPLIT, True)], ids=["f32", "split3", "split3-image"])
def test_persistent_walk_by_the_dispatchers_own_threshold(arith, w_split):
    """40 x 32 = 1,280 tiles of 128 x 128 is where auto starts the walk; K = 128 is its minimum.  Same bits as one tile per workgroup."""
    M, N, K = 128 * 40 - 37, 128 * 32 - 96, 128
    A, W, b = u(7, (M, K), 1.0), u(8, (N, K), 0.2), u(9, (N,), 0.1)
    got = run_f32(A, W, b, arith=arith, w_split=w_split)
    close_f32(got, A, W, b)
    assert np.array_equal(bits(got), bits(B.gemm(A, W, b, epilogue=B.EPI_BIAS_QGELU, tile=10, arith=arith)))


@pytest.mark.parametrize("arith", [B.ARITH_F32, SPLIT], ids=["f32", "split3"])
def test_persistent_walk_with_the_hand_over(arith):
    """600 tiles on 512 workgroups with a workspace: the instantiations with helper pieces, helpers on time and late."""
    M, N, K = 128 * 100 - 57, 768, 768
    A, W, b = u(10, (M, K), 1.0), u(11, (N, K), 0.05), u(12, (N,), 0.1)
    ref = B.gemm(A, W, b, epilogue=B.EPI_BIAS_QGELU, tile=10, arith=arith)
    for late in (0, 1):
        st = {}
        got = run_f32(A, W, b, tile=9, workspace=True, handover_test=late, stats=st, arith=arith)
        assert np.array_equal(bits(got), bits(ref)), late
        assert st["taken"] + st["recomputed"] > 0, st
    close_f32(ref[:300], A[:300], W, b)


@pytest.mark.parametrize("arith", [B.ARITH_F32, SPLIT], ids=["f32", "split3"])
@pytest.mark.parametrize("centred", [True, False], ids=["centred", "colsum"])
def test_fold_consumer_form(arith, centred):
    """LayerNorm folded into the GEMM with the QuickGELU behind it (the library's own epilogue code 7), on rows whose mean is as large
    as their spread; against LayerNorm-then-GEMM in float64, bar of tests/test_gpu_ops.py::test_gemm_layernorm_fold_with_centred_weights
    (2e-5 on values of order one; q's slope is at most 1.1, the bar is taken against the larger of 1 and max |ref|)."""
    M, N, K = 394, 200, 128
    x = (u(13, (M, K), 2.0) + u(14, (M, 1), 2.0)).astype(np.float32)
    gamma, beta = (1.0 + u(15, (K,), 0.5)).astype(np.float32), u(16, (K,), 0.5)
    W, b = u(17, (N, K), 0.05), u(18, (N,), 0.1)
    rows = B.rowstats_f32(x)
    if centred:
        Wf, _, bf = B.ln_fold_weights_f32_centered(W, b, gamma, beta)
        ln = (rows, None)
    else:
        Wf, cs, bf = B.ln_fold_weights_f32(W, b, gamma, beta)
        ln = (rows, cs)
    x64 = x.astype(np.float64)
    mean, var = x64.mean(1, keepdims=True), x64.var(1, keepdims=True)
    y64 = (x64 - mean) / np.sqrt(var + 1e-6) * gamma + beta
    ref = q64(y64 @ W.astype(np.float64).T + b)
    outs = {}
    for tile in ((0, 9, 10, 11, 12) if arith == B.ARITH_F32 else (0, 9, 10, 11)):
        outs[tile] = run_f32(x, Wf, bf, tile=tile, arith=arith, ln=ln)
        assert np.array_equal(bits(outs[tile]), bits(outs[0])), tile
    err = float(np.abs(outs[0] - ref).max())
    print(f"fold consumer, arith {arith}, centred {centred}: max err {err:.3g} of {float(np.abs(ref).max()):.3g}")
    assert err <= 2e-5 * max(1.0, float(np.abs(ref).max()))
    # the plain epilogue on the normalised rows is the same function of (nearly) the same accumulator
    plain = B.gemm(B.layernorm(x, gamma, beta), W, b, epilogue=B.EPI_BIAS_QGELU, tile=10, arith=arith)
    assert float(np.abs(plain - outs[0]).max()) <= 4e-5 * max(1.0, float(np.abs(ref).max()))


def test_refusals_stay_refusals():
    A, W, b = u(19, (8, 64), 1.0), u(20, (16, 64), 0.1), u(21, (16,), 0.1)
    for epi in (3, 4, 5, 7, 8):          # the fold forms are the library's own; 8 does not exist
        with pytest.raises(B.VitError):
            B.gemm(A, W, b, epilogue=epi)
    with pytest.raises(B.VitError):      # the fold takes the bias, GELU and QuickGELU roles only
        B.gemm(A, W, b, residual=np.zeros((8, 16), np.float32), epilogue=B.EPI_BIAS_RESIDUAL, ln=(np.ones((8, 2), np.float32), None))
    Ab, Wb = B.to_bf16_bits(A), B.to_bf16_bits(W)
    for epi in (3, 5):
        with pytest.raises(B.VitError):
            B.gemm_bf16(Ab, Wb, b, epilogue=epi)


# ---- bf16 ------------------------------------------------------------------------------------------------------------------------

def run_bf16(Ab, Wb, b, **kw):
    out = {}
    got = B.gemm_bf16(Ab, Wb, b, epilogue=B.BF16_EPI_BF16_QGELU, ldc=Wb.shape[0] + 8, frames=S, out=out, **kw)
    out["C"].check()
    return got


@pytest.mark.parametrize("variant,K", [(1, 64), (1, 192), (2, 192), (0, 192), (0, 64)],
                         ids=["two-stage-K64", "two-stage", "ping-pong", "auto", "auto-K64"])
def test_bf16_kernels(variant, K):
    """531 x 260: three tile rows with a ragged last one, a second tile column of four columns.  K = 64 is the two-stage kernel's own
    range (auto sends it there); K = 192 reaches the ping-pong kernel (auto, variant 2) with an odd number of K steps."""
    M, N = 531, 260
    Ab, Wb, b = B.to_bf16_bits(u(22, (M, K), 1.0)), B.to_bf16_bits(u(23, (N, K), 0.2)), u(24, (N,), 0.1)
    ref = q64(B.from_bf16_bits(Ab).astype(np.float64) @ B.from_bf16_bits(Wb).astype(np.float64).T + b)
    got = B.from_bf16_bits(run_bf16(Ab, Wb, b, variant=variant))
    err = np.abs(got - ref)
    assert (err <= 2.0 ** -8 * np.abs(ref) + 1e-5).all(), float(err.max())       # one bf16 rounding of the result
    if variant == 0:
        assert np.array_equal(run_bf16(Ab, Wb, b, variant=0), run_bf16(Ab, Wb, b, variant=2 if K >= 128 else 1))


def test_bf16_many_tiles_and_fold_consumer():
    """More tiles than workgroups on the ping-pong kernel (the persistent loop crosses tile boundaries), then the same kernel as the
    LayerNorm fold's consumer."""
    M, N, K = 256 * 37 + 19, 2048 + 4, 128
    Ab, Wb, b = B.to_bf16_bits(u(25, (M, K), 1.0)), B.to_bf16_bits(u(26, (N, K), 0.2)), u(27, (N,), 0.1)
    ref = q64(B.from_bf16_bits(Ab).astype(np.float64) @ B.from_bf16_bits(Wb).astype(np.float64).T + b)
    err = np.abs(B.from_bf16_bits(run_bf16(Ab, Wb, b)) - ref)
    assert (err <= 2.0 ** -8 * np.abs(ref) + 1e-5).all(), float(err.max())
    M, N, K = 531, 260, 192
    x = (u(28, (M, 1), 2.0) + u(29, (M, K), 1.0)).astype(np.float32)
    gamma, beta = (1.0 + u(30, (K,), 0.5)).astype(np.float32), u(31, (K,), 0.5)
    W, b = u(32, (N, K), 0.05), u(33, (N,), 0.1)
    x16, stats = B.rowstats_bf16(x)
    Wf, cs, bf = B.ln_fold_weights(W, b, gamma, beta)
    got = B.from_bf16_bits(run_bf16(x16, Wf, bf, variant=2, ln_rows=stats, ln_colsum=cs))
    # the twin: the same launch with the bias role, then the function in float64 on what it stored (bf16 of the accumulator)
    lin = B.from_bf16_bits(B.gemm_bf16(x16, Wf, bf, epilogue=B.BF16_EPI_BF16, variant=2, ln_rows=stats, ln_colsum=cs)).astype(np.float64)
    err = np.abs(got - q64(lin))
    # two bf16 roundings apart (the twin's accumulator was rounded before the function, slope <= 1.1)
    assert (err <= 2.2 * 2.0 ** -8 * np.maximum(np.abs(lin), np.abs(got)) + 1e-5).all(), float(err.max())


# ---- the function itself -----------------------------------------------------------------------------------------------------------

def ulp_err(got, x):
    """|got - q64(x)| in units of (ulp of the float32 result + 2^-126), finite inputs."""
    ref = q64(x)
    unit = np.spacing(np.abs(ref.astype(np.float32))).astype(np.float64) + 2.0 ** -126
    return np.abs(got.astype(np.float64) - ref) / unit


def sweep():
    xs = np.concatenate([np.linspace(-100.0, 100.0, 1 << 17), u(34, (1 << 15,), 100.0), u(35, (1 << 14,), 8.0), u(36, (1 << 12,), 0.01)])
    return np.sort(xs.astype(np.float32))


def through_gemm(xs, N=64, bf16=False, **kw):
    """One GEMM with K = 32 (bf16: 64, that kernel's K step) whose single non-zero product passes the value through: the accumulator
    is exactly the input."""
    K = 64 if bf16 else 32
    A = np.zeros((xs.size, K), np.float32)
    A[:, 0] = xs
    W = np.zeros((N, K), np.float32)
    W[:, 0] = 1.0
    if bf16:
        return B.gemm_bf16(B.to_bf16_bits(A), B.to_bf16_bits(W), np.zeros(N, np.float32), epilogue=B.BF16_EPI_BF16_QGELU, **kw)
    return B.gemm(A, W, np.zeros(N, np.float32), epilogue=B.EPI_BIAS_QGELU, **kw)


def test_quickgelu_epilogue_over_its_range_against_pytorch():
    """Dense over [-100, 100] (2^17 evenly spaced, 2^15 + 2^14 + 2^12 random values at three scales).  No bar fixed in advance: the
    error is in units of (ulp of the result + 2^-126) against the float64 model, PyTorch's CPU fp32 x * torch.sigmoid(1.702 * x) is
    measured the same way on the same inputs, and the kernel may exceed PyTorch's maximum by at most 2 x (v_exp_f32 and v_rcp_f32 are
    1-ulp instructions where libm rounds to half an ulp; both carry the argument's relative error, which grows with |1.702 y| -- the
    deep negative tail is tens of units for both).  Interior tiles evaluate the packed lock-step form, the ragged last tile and
    N = 32 the scalar one: the same bits.
    Measured on an MI355X (profiles/r19/clip.md): kernel max 56.30 units (at y = -37.98), PyTorch CPU max 75.34 (at y = -40.87); on
    [-8, 8] kernel 14.01, PyTorch 11.73."""
    import torch

    xs = sweep()
    got = through_gemm(xs)                        # 64 columns: whole 64x64 tiles take the lock-step form
    assert all(np.array_equal(bits(got[:, 0]), bits(got[:, n])) for n in range(1, 64))
    edge = through_gemm(xs, N=32)                 # a partial tile column: the scalar form, value by value
    assert np.array_equal(bits(edge[:, 0]), bits(got[:, 0]))
    lat = through_gemm(np.concatenate([xs[:4096:64], xs[-4096::64]]), N=32, tile=11)
    assert np.array_equal(bits(lat[:, 0]), bits(np.concatenate([got[:4096:64, 0], got[-4096::64, 0]])))
    t = torch.from_numpy(xs)
    pt = (t * torch.sigmoid(1.702 * t)).numpy()
    e_kernel, e_torch = ulp_err(got[:, 0], xs), ulp_err(pt, xs)
    k, p = int(e_kernel.argmax()), int(e_torch.argmax())
    print(f"quickgelu fp32: kernel max {e_kernel[k]:.2f} units at y = {xs[k]!r}, PyTorch CPU max {e_torch[p]:.2f} at y = {xs[p]!r}; "
          f"on [-8, 8]: kernel {e_kernel[np.abs(xs) <= 8].max():.2f}, PyTorch {e_torch[np.abs(xs) <= 8].max():.2f}")
    assert e_kernel.max() <= 2.0 * e_torch.max()
    # bf16: the fp32 sequence on the fp32 accumulator, rounded once -- half a bf16 ulp of the model plus the fp32 form's error
    xb = B.from_bf16_bits(B.to_bf16_bits(xs))     # what a bf16 operand can carry through the GEMM
    gotb = through_gemm(xb, bf16=True)
    assert all(np.array_equal(gotb[:, 0], gotb[:, n]) for n in range(1, 64))
    f32 = through_gemm(xb)[:, 0]
    assert np.array_equal(gotb[:, 0], B.to_bf16_bits(f32))                       # exactly: one rounding of the fp32 value
    ref = q64(xb)
    half_ulp16 = np.spacing(np.abs(ref.astype(np.float32))).astype(np.float64) * 2.0 ** 15
    slack = e_kernel.max() * (np.spacing(np.abs(ref.astype(np.float32))).astype(np.float64) + 2.0 ** -126)
    assert (np.abs(B.from_bf16_bits(gotb[:, 0]).astype(np.float64) - ref) <= half_ulp16 + slack + 2.0 ** -133).all()
    assert np.array_equal(through_gemm(xb, bf16=True, variant=1)[:, 0], gotb[:, 0])     # K = 64: auto was the two-stage kernel already


def test_special_values_and_row_confinement():
    """+Inf -> +Inf; -Inf and NaN -> NaN; a large negative finite y -> a tiny negative value or -0, never NaN; 0 -> 0; the fp32
    extremes; and a non-finite row stays in its own row: every other row keeps the bits of the clean launch."""
    fmax, tiny, den = np.float32(3.4028235e38), np.float32(1.17549435e-38), np.float32(1e-45)
    specials = np.array([np.inf, -np.inf, np.nan, fmax, -fmax, -100.0, -60.0, -52.0, -51.0, 0.0, -0.0, tiny, -tiny, den, -den, 100.0],
                        np.float32)
    clean = np.linspace(-6.0, 6.0, 128).astype(np.float32)
    for N, kw in ((64, {}), (32, {}), (32, dict(tile=10))):
        xs = np.concatenate([clean[:64], specials, clean[64:]])
        got = through_gemm(xs, N=N, **kw)[:, 0]
        s = got[64:64 + specials.size]
        assert s[0] == np.inf and np.isnan(s[1]) and np.isnan(s[2]) and s[3] == fmax
        for v in s[4:9]:
            assert not np.isnan(v) and v <= 0.0 and v > -1e-20, s
        assert s[9] == 0.0 and s[10] == 0.0 and abs(float(s[11])) <= float(tiny) and abs(float(s[12])) <= float(tiny)
        assert s[13] == 0.0 or s[13] == den
        assert s[15] == np.float32(100.0)
        ref = through_gemm(clean, N=N, **kw)[:, 0]
        assert np.array_equal(bits(np.concatenate([got[:64], got[64 + specials.size:]])), bits(ref))
    # a poisoned ROW of a real product: the other rows' bits do not move (fp32 tiles and both bf16 kernels)
    M, Nn, K = 200, 96, 128
    A, W, b = u(37, (M, K), 1.0), u(38, (Nn, K), 0.2), u(39, (Nn,), 0.1)
    for poison in (np.nan, np.inf, -np.inf):
        P = A.copy()
        P[77, 5] = poison
        for kw in (dict(), dict(tile=10), dict(tile=9), dict(tile=11, arith=SPLIT)):
            c, p = B.gemm(A, W, b, epilogue=B.EPI_BIAS_QGELU, **kw), B.gemm(P, W, b, epilogue=B.EPI_BIAS_QGELU, **kw)
            keep = np.arange(M) != 77
            assert np.array_equal(bits(c[keep]), bits(p[keep])) and not np.isfinite(p[77]).all(), (poison, kw)
        for variant in (1, 2):
            Ab, Pb, Wb = B.to_bf16_bits(A), B.to_bf16_bits(P), B.to_bf16_bits(W)
            c = B.gemm_bf16(Ab, Wb, b, epilogue=B.BF16_EPI_BF16_QGELU, variant=variant)
            p = B.gemm_bf16(Pb, Wb, b, epilogue=B.BF16_EPI_BF16_QGELU, variant=variant)
            assert np.array_equal(c[keep], p[keep]) and not np.isfinite(B.from_bf16_bits(p[77])).all(), (poison, variant)
