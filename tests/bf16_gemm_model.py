"""Host models of the bf16 GEMM path (vithip_gemm_bf16: csrc/vit_gemm_bf16_pp.hip, csrc/vit_gemm_bf16.hip; the patch embeddings on
the same pipe) for tests/test_bf16_gemm_model.py and tests/test_gpu_bf16_gemm_accuracy.py.  numpy only, no GPU.

Two operand families:

  integer   A in {-1, 0, 1}, W in {-2 .. 2} (bf16-exact).  Every product and every partial sum is an integer far below 2^24, so the fp32
            accumulator of ANY matrix instruction in ANY order is the exact integer A . W^T (exact_acc asserts it), and each epilogue is
            a short chain of fp32 operations on it that numpy reproduces bit for bit.  No model of v_mfma_f32_16x16x32_bf16 is needed.
  random    bf16-rounded uniform operands against float64, with e_seq -- the error of a plain sequential fp32 evaluation (an FMA chain
            over k ascending, then the epilogue's fp32 operations) -- as the yardstick:
                fp32 outputs   |x - ref| <= 4 e_seq + 2^-23 |ref|max
                bf16 outputs   rne_bf16(ref - bar) <= x <= rne_bf16(ref + bar) as ordered bf16 values, the same bar: a store that
                               truncates instead of rounding fails it on about half of all outputs
                fold consumer  the same with norm = rstd (|A| . |W|^T) + |mean*rstd * colsum| + |bias| per element in the place of
                               |ref|max (the terms cancel), in the normalised form  max e / norm <= 4 max e_seq / norm + 2^-23.
            e_seq and the normalisers come from the reference and the inputs, never from a kernel's output.

The epilogues, read from the kernels (acc is the fp32 accumulator, every operation below rounds once, to fp32):

  BF16            rne_bf16(acc + bias)                                       both kernels
  F32_RESIDUAL    (acc + bias) + R                                           both kernels: the ping-pong kernel's put_blk adds the bias
                                                                             before the transpose and R behind it; the two-stage kernel
                                                                             (vit_gemm_bf16.hip: y = acc + b4, then y + res) has the same order
  F32_EMBED       (acc + conv_b) + pos[1 + patch]; class row cls + pos[0]    both patch embeddings (vit_patch_embed_bf16.hip: acc + bn + add)
  fold consumer   c = fma(-mean*rstd, colsum, bias); t = fma(acc, rstd, c); rne_bf16(t)
                  THE CONTRACTION FORM: `b4 - m4 * s4` (vit_gemm_bf16_pp.hip, pack()) is ONE fused operation.  The gfx950 assembly of
                  the shipped flags (-O3, no -ffp-contract: hipcc's default is fast) holds 768 v_pk_fma_f32 and not one v_pk_mul_f32
                  or v_pk_add_f32 in gemm_bf16_pp_kernel<BF16, 0, 0, LNF = true>: two fused operations per pair of values, the
                  first with neg_lo / neg_hi on one factor.
  fold producer   C as F32_RESIDUAL, x16 = rne_bf16(C), partials [ln_strips(N)][M][2] = (sum, sum of squares) of C over each 64-column
                  strip; strips (or parts of strips) behind N add nothing.  Order-free only while the sums are exact: producer_case
                  asserts |C| <= 256 on the reference (squares <= 2^16, 64 of them <= 2^22).

The two activations for a bf16 destination, step by step in fp32 (v_exp_f32 is float64 exp2 rounded to fp32, v_rcp_f32 float64 1/x
rounded to fp32; the device's are within 1 ulp, so these serve the CPU test of the stated error figures and are no bar for the GPU):
gelu_bf16 (gelu_bf16_lockstep: both kernels), quick_gelu (the five steps of every kernel), and gelu_erf_f32 (erf_fp32 in the
reference's formula, the fp32 GEMMs' form: what a bf16 epilogue must not use, tests/test_bf16_gemm_model.py shows why).
"""
import math

import numpy as np

from split_gemm_model import _add_round_to_odd
from vit_amd import binding as B
from vit_amd import synth

SEED = 3301           # the one draw the CPU test and the GPU tests share
TILE = 256            # the ping-pong kernel's tile is 256 x 256, K steps are 64 deep
STRIP = 64
CLAMP = 4.0 * math.sqrt(2.0)          # gelu_bf16_lockstep clamps |y| at fp32(4 sqrt 2)
CLAMP_F32 = np.float32(5.656854249492381)

# (M, N, K) of tests/test_gpu_bf16_gemm_accuracy.py.  2 x 3 tiles of which two are interior, ragged M, N % 8 == 4 (the half-chunk store)
# at the shortest K the ping-pong kernel takes; odd K-step counts; the model's own K; less than one tile (K = 64: two-stage only).
SHAPES = [(275, 516, 128), (275, 516, 192), (275, 516, 448), (300, 260, 768), (64, 256, 3072), (5, 12, 64), (5, 12, 128)]
PERSISTENT = (256 * 37 + 19, 2048 + 4, 192)   # 38 x 9 = 342 tiles: more than the 256 workgroups of an MI355X
PRODUCER_SHAPES = [s for s in SHAPES if 128 <= s[2] <= 768]   # the fold needs the ping-pong kernel; |C| <= 256 holds up to K = 768
RANDOM_SHAPES = SHAPES[:4]
MUTANT_SHAPE = SHAPES[0]
PADS = dict(lda=8, ldw=16, ldc=4, ldr=12, ldx16=12)   # elements above the minimum leading dimension (the forms test_gpu_strides.py uses)


def f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def rne_bf16(x):
    """fp32 -> the nearest bf16 value (ties to even), as fp32."""
    return B.from_bf16_bits(B.to_bf16_bits(np.asarray(x, np.float32))).reshape(np.shape(x))


def bits16(x):
    return B.to_bf16_bits(np.asarray(x, np.float32)).reshape(np.shape(x))


def trunc_bf16_bits(x):
    """The mutant store: the upper 16 bits, no rounding."""
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def fma32(a, b, c):
    """fma(a, b, c) of fp32 arrays with ONE rounding: the product is exact in float64, the sum is rounded to odd there."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    p, c = np.broadcast_arrays(a * b, c)
    return _add_round_to_odd(np.ascontiguousarray(c), np.ascontiguousarray(p)).astype(np.float32)


# ---- operands ------------------------------------------------------------------------------------------------------------------------

def u(index, shape, lo, hi, seed=SEED):
    return synth.uniform(seed, index, int(np.prod(shape)), lo, hi).reshape(shape)


def ints(index, shape, lo, hi, seed=SEED):
    """Integers lo .. hi, uniformly, as fp32."""
    return np.clip(np.floor(u(index, shape, lo, hi + 1, seed)), lo, hi).astype(np.float32)


def integer_operands(M, N, K):
    """A in {-1, 0, 1} [M][K], W in {-2 .. 2} [N][K]."""
    return ints(0, (M, K), -1, 1), ints(1, (N, K), -2, 2)


def bias_residual(M, N, integer):
    """bias [N] and residual [M][N] in +-16: integer-valued, or fractional fp32."""
    if integer:
        return ints(2, (N,), -16, 16), ints(3, (M, N), -16, 16)
    return u(4, (N,), -16.0, 16.0), u(5, (M, N), -16.0, 16.0)


def exact_acc(A, W):
    """A . W^T as float64; asserted integral and below 2^24: the fp32 accumulator of any summation order holds exactly this."""
    acc = np.asarray(A, np.float64) @ np.asarray(W, np.float64).T
    assert np.array_equal(acc, np.rint(acc)) and float(np.abs(acc).max()) < 2.0 ** 24
    bound = np.abs(np.asarray(A, np.float64)) @ np.abs(np.asarray(W, np.float64)).T   # no partial sum of any order is larger
    assert float(bound.max()) < 2.0 ** 24
    return acc


def random_operands(M, N, K, a=1.0, w=0.08):
    """bf16-exact uniform operands (the ranges of tests/test_gpu_bf16.py)."""
    return rne_bf16(u(6, (M, K), -a, a)), rne_bf16(u(7, (N, K), -w, w))


def fold_inputs(M, N, K):
    """The random family's fold consumer as the engine runs it: fp32 rows whose mean is as large as their spread, an unfolded weight
    and bias, gamma and beta.  The device (vithip_rowstats_bf16, vithip_ln_fold_weights) or fold_on_host turns them into the GEMM's operands."""
    x = u(10, (M, K), -1.5, 1.5) + u(11, (M, 1), -1.5, 1.5)
    return x, u(12, (N, K), -0.05, 0.05), u(13, (N,), -0.1, 0.1), np.float32(1.0) + u(14, (K,), -0.5, 0.5), u(15, (K,), -0.2, 0.2)


def fold_on_host(x, W, b, g, beta):
    """Host stand-ins of the two device helpers (the CPU test only): x16 bits, rows, Wf bits, colsum, bias_f."""
    rows = rows_f32_seq(*seq_sums(x), x.shape[1])
    Wf = rne_bf16(g[None, :] * W)
    cs = f32(Wf.astype(np.float64).sum(axis=1))
    bf = f32(b.astype(np.float64) + W.astype(np.float64) @ beta.astype(np.float64))
    return bits16(x), rows, bits16(Wf), cs, bf


def consumer_rows(M):
    """(rstd, mean*rstd) per row: rstd log-spaced from 0.05 to 1e3 (= 1 / sqrt(eps)), mean*rstd of alternating sign, the rows shuffled, so
    that neighbouring rows -- and rows 8 apart -- have nothing in common."""
    rstd = 0.05 * 2e4 ** np.linspace(0.0, 1.0, M)
    m = np.where(np.arange(M) % 2 == 0, 1.0, -1.0) * u(9, (M,), 0.1, 3.0)
    order = np.argsort(u(8, (M,), 0.0, 1.0), kind="stable")
    return np.stack([rstd, m], axis=1)[order].astype(np.float32)


# ---- epilogue models (acc: float64 or fp32 holding fp32 values) -----------------------------------------------------------------------

def epi_bf16(acc, bias):
    return bits16(f32(acc) + np.asarray(bias, np.float32)[None, :])


def epi_f32_residual(acc, bias, R):
    return (f32(acc) + np.asarray(bias, np.float32)[None, :]) + np.asarray(R, np.float32)


def consumer_f32(acc, rows, colsum, bias):
    """t of the fold consumer before the store (or the activation)."""
    rows = np.asarray(rows, np.float32)
    c = fma32(-rows[:, 1:2], np.asarray(colsum, np.float32)[None, :], np.asarray(bias, np.float32)[None, :])
    return fma32(f32(acc), rows[:, 0:1], c)


def epi_consumer(acc, rows, colsum, bias):
    return bits16(consumer_f32(acc, rows, colsum, bias))


def ln_strips(N):
    return 4 * ((N + TILE - 1) // TILE)   # vithip_ln_strips


def strip_partials(C):
    """[ln_strips(N)][M][2] (sum, sum of squares) of every 64-column strip in float64; absent columns add nothing."""
    C = np.asarray(C, np.float64)
    M, N = C.shape
    strips = ln_strips(N)
    padded = np.zeros((M, strips * STRIP))
    padded[:, :N] = C
    s = padded.reshape(M, strips, STRIP)
    return np.stack([s.sum(axis=2), (s * s).sum(axis=2)], axis=2).transpose(1, 0, 2)


def producer_case(M, N, K):
    """Integer operands, bias and residual; C, x16 bits and strip partials of the fold producer; |C| <= 256 asserted on the reference."""
    A, W = integer_operands(M, N, K)
    bias, R = bias_residual(M, N, integer=True)
    acc = exact_acc(A, W)
    C64 = acc + bias[None, :].astype(np.float64) + R.astype(np.float64)
    assert float(np.abs(C64).max()) <= 256.0, (M, N, K, float(np.abs(C64).max()))
    C = epi_f32_residual(acc, bias, R)
    assert np.array_equal(C.astype(np.float64), C64)
    part = strip_partials(C64)
    assert float(part.max()) <= 2.0 ** 22
    return dict(A=A, W=W, bias=bias, R=R, C=C, x16=bits16(C), partials=part.astype(np.float32))


def embed_patches(images, patch):
    """[n][C][S][S] -> [n * G * G][C * p * p], k = (c * p + kh) * p + kw (ViT_seq.c:52-101)."""
    n, C, S, _ = images.shape
    G = S // patch
    return images.reshape(n, C, G, patch, G, patch).transpose(0, 2, 4, 1, 3, 5).reshape(n * G * G, C * patch * patch)


def embed_case(cfg, n):
    """Integer pixels in +-4 and conv weights in +-2, fractional conv_b, cls and pos; x [n][tokens][D] of F32_EMBED bit for bit."""
    D = cfg.embed_dim
    imgs = ints(20, (n, cfg.in_chans, cfg.img_size, cfg.img_size), -4, 4)
    conv_w = ints(21, (D, cfg.patch_dim), -2, 2)
    conv_b, cls, pos = u(22, (D,), -1.0, 1.0), u(23, (D,), -1.0, 1.0), u(24, (cfg.patches + 1, D), -1.0, 1.0)
    acc = exact_acc(embed_patches(imgs, cfg.patch_size), conv_w).reshape(n, cfg.patches, D)
    x = np.empty((n, cfg.patches + 1, D), np.float32)
    x[:, 0] = cls + pos[0]
    x[:, 1:] = (f32(acc) + conv_b[None, None, :]) + pos[None, 1:, :]
    return dict(images=imgs, conv_w=conv_w, conv_b=conv_b, cls=cls, pos=pos, x=x)


# ---- row statistics --------------------------------------------------------------------------------------------------------------------

LN_EPS = 1e-6   # VITHIP_LN_EPS


def rows_f64(s, ss, dim, eps=None):
    """(rstd, mean*rstd) from the sums of a row, float64: var = E[x^2] - mean^2, 1 / sqrt(var + eps)."""
    s, ss = np.asarray(s, np.float64), np.asarray(ss, np.float64)
    mean = s / dim
    rstd = 1.0 / np.sqrt(ss / dim - mean * mean + (LN_EPS if eps is None else eps))
    return np.stack([rstd, mean * rstd], axis=1)


def rows_f32_seq(s, ss, dim, eps=None):
    """The same from the same sums, every operation rounded to fp32 on its own (the epsilon is added in double: ViT_seq.c:113-116)."""
    s, ss, d = np.asarray(s, np.float32), np.asarray(ss, np.float32), np.float32(dim)
    mean = s / d
    var = ss / d - mean * mean
    rstd = np.float32(1.0) / np.sqrt((var.astype(np.float64) + (LN_EPS if eps is None else eps)).astype(np.float32))
    return np.stack([rstd, mean * rstd], axis=1)


def seq_sums(x):
    """(sum, sum of squares) of every row, sequential fp32: an add chain and an FMA chain over the columns ascending."""
    x = np.asarray(x, np.float32)
    s, ss = np.zeros(x.shape[0], np.float32), np.zeros(x.shape[0], np.float32)
    for k in range(x.shape[1]):
        s = s + x[:, k]
        ss = fma32(x[:, k], x[:, k], ss)
    return s, ss


def rows_bar(seq, ref):
    """4 e_seq + 2^-23 |ref| per row and column of the pair; e_seq is the sequential evaluation's largest error in that column."""
    e_seq = np.abs(np.asarray(seq, np.float64) - ref).max(axis=0)
    return 4.0 * e_seq[None, :] + 2.0 ** -23 * np.abs(ref)


def layernorm_f64(x, g, b, eps=None):
    x = np.asarray(x, np.float64)
    mean = x.mean(axis=1, keepdims=True)
    var = (x * x).mean(axis=1, keepdims=True) - mean * mean
    return (x - mean) / np.sqrt(var + (LN_EPS if eps is None else eps)) * np.asarray(g, np.float64) + np.asarray(b, np.float64)


def layernorm_f32_seq(x, g, b, eps=None):
    """csrc/vit_rowops.hip's formula one fp32 operation after the other: y = (x - mean) * inv_std * gamma + beta."""
    x = np.asarray(x, np.float32)
    s, ss = seq_sums(x)
    d = np.float32(x.shape[1])
    mean = s / d
    var = ss / d - mean * mean
    rstd = np.float32(1.0) / np.sqrt((var.astype(np.float64) + (LN_EPS if eps is None else eps)).astype(np.float32))
    return (x - mean[:, None]) * rstd[:, None] * np.asarray(g, np.float32) + np.asarray(b, np.float32)


# ---- the float64 side of the random family ----------------------------------------------------------------------------------------------

def fma_chain(A, W):
    """acc = fma(a_k, w_k, acc) from zero, k ascending, one rounding per step."""
    acc = np.zeros((A.shape[0], W.shape[0]), np.float64)
    A64, W64 = np.asarray(A, np.float64), np.asarray(W, np.float64)
    for k in range(A.shape[1]):
        acc = _add_round_to_odd(acc, np.outer(A64[:, k], W64[:, k])).astype(np.float32).astype(np.float64)
    return acc.astype(np.float32)


def ref64(A, W, bias, R=None):
    ref = np.asarray(A, np.float64) @ np.asarray(W, np.float64).T + np.asarray(bias, np.float64)[None, :]
    return ref if R is None else ref + np.asarray(R, np.float64)


def seq_f32(A, W, bias, R=None):
    """The sequential fp32 evaluation of BF16 (before the store) or F32_RESIDUAL."""
    y = fma_chain(A, W) + np.asarray(bias, np.float32)[None, :]
    return y if R is None else y + np.asarray(R, np.float32)


def bar_f32(seq, ref):
    """4 e_seq + 2^-23 |ref|max, e_seq = max |seq - ref|."""
    return 4.0 * float(np.abs(np.asarray(seq, np.float64) - ref).max()) + 2.0 ** -23 * float(np.abs(ref).max())


def consumer_ref64(A, W, rows, colsum, bias):
    rows = np.asarray(rows, np.float64)
    acc = np.asarray(A, np.float64) @ np.asarray(W, np.float64).T
    return rows[:, 0:1] * acc - rows[:, 1:2] * np.asarray(colsum, np.float64)[None, :] + np.asarray(bias, np.float64)[None, :]


def consumer_norm(A, W, rows, colsum, bias):
    """rstd (|A| . |W|^T) + |mean*rstd * colsum| + |bias| per element: the scale of the terms that cancel in the consumer's output."""
    rows = np.asarray(rows, np.float64)
    mag = np.abs(np.asarray(A, np.float64)) @ np.abs(np.asarray(W, np.float64)).T
    return rows[:, 0:1] * mag + np.abs(rows[:, 1:2] * np.asarray(colsum, np.float64)[None, :]) + np.abs(np.asarray(bias, np.float64))[None, :]


def consumer_seq(A, W, rows, colsum, bias):
    return consumer_f32(fma_chain(A, W), rows, colsum, bias)


def consumer_share(seq, ref, norm):
    """4 max e_seq / norm + 2^-23: the consumer's bar as a share of the normaliser."""
    return 4.0 * float((np.abs(np.asarray(seq, np.float64) - ref) / norm).max()) + 2.0 ** -23


def consumer_bar(seq, ref, norm):
    return consumer_share(seq, ref, norm) * norm


def sample_rows(M, count=48):
    """Rows on which e_seq of a large case is taken: a sample's maximum is at most the whole's, so the bar only tightens."""
    return np.unique(np.linspace(0, M - 1, count).astype(np.int64))


def bf16_interval(ref, bar):
    """(lo, hi) bf16 values, as fp32, between which a bf16 output must lie, ends included."""
    ref = np.asarray(ref, np.float64)
    return rne_bf16(f32(ref - bar)), rne_bf16(f32(ref + bar))


def in_interval(got_bits, ref, bar):
    """Elementwise: the bf16 output lies in [rne_bf16(ref - bar), rne_bf16(ref + bar)] as ordered values."""
    lo, hi = bf16_interval(ref, bar)
    got = B.from_bf16_bits(np.asarray(got_bits, np.uint16)).reshape(np.shape(got_bits))
    return (got >= lo) & (got <= hi)


def differ_share(got_bits, ref):
    """Share of bf16 outputs that are not rne_bf16(ref) (a zero of either sign counts as the same value)."""
    got = B.from_bf16_bits(np.asarray(got_bits, np.uint16)).reshape(np.shape(got_bits))
    return float((got != rne_bf16(f32(ref))).mean())


def mismatch(got, want):
    """(count, first index) of the elements whose bits differ; (0, None) if none."""
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert g.shape == w.shape and g.dtype.itemsize == w.dtype.itemsize, (g.shape, w.shape, g.dtype, w.dtype)
    kind = {2: np.uint16, 4: np.uint32}[g.dtype.itemsize]
    bad = np.argwhere(g.view(kind) != w.view(kind))
    return (0, None) if bad.size == 0 else (int(bad.shape[0]), tuple(int(i) for i in bad[0]))


# ---- activations -------------------------------------------------------------------------------------------------------------------------

GELU_C = np.array([-1.000037431716919, -1.1505244970321655, -0.4605136811733246, -0.05179140716791153,
                   0.007414536084979773, -0.0006474481779150665, 2.524326555430889e-05], np.float32)
ERF_C = np.array([-3.144179208902642e-05, 3.0881378916092217e-04, -1.0324339382350445e-03, -5.368884885683656e-04,
                  1.95839274674654e-02, -1.0291960090398788e-01, -6.36597752571106e-01, -1.128380298614502], np.float32)
QGELU_K = np.float32(-2.4554669595930157)


def ulp_step(x, steps):
    """x moved by `steps` fp32 ulps (the device's v_exp_f32 / v_rcp_f32 are within 1 ulp of the rounded exact value)."""
    x = np.asarray(x, np.float32)
    for _ in range(abs(steps)):
        x = np.nextafter(x, np.float32(np.inf if steps > 0 else -np.inf))
    return x


def exp2_f32(x, steps=0):
    with np.errstate(over="ignore", under="ignore"):
        return ulp_step(np.exp2(np.asarray(x, np.float32).astype(np.float64)).astype(np.float32), steps)


def gelu_bf16(y, exp_steps=0):
    """gelu_bf16_lockstep: t = min(|y|, 4 sqrt2); Q(t) by Horner in fma; e = exp2(Q); fma(-t, e, max(y, 0))."""
    y = np.asarray(y, np.float32)
    t = np.minimum(np.abs(y), CLAMP_F32)
    q = fma32(GELU_C[6], t, GELU_C[5])
    for k in range(4, -1, -1):
        q = fma32(q, t, GELU_C[k])
    return fma32(-t, exp2_f32(q, exp_steps), np.maximum(y, np.float32(0)))


def gelu_erf_f32(y, exp_steps=0):
    """The fp32 GEMMs' GELU: 0.5 y (1 + erf_fp32(y / sqrt 2)) (csrc/vit_gemm_common.hpp, gelu_erf)."""
    y = np.asarray(y, np.float32)
    x = y * np.float32(0.70710678118654752440)
    t = np.minimum(np.abs(x), np.float32(4.0))
    q = np.broadcast_to(ERF_C[0], t.shape)
    for c in ERF_C[1:]:
        q = fma32(q, t, c)
    e = exp2_f32(q * t * np.float32(1.4426950408889634), exp_steps)
    return np.float32(0.5) * y * (np.float32(1.0) + np.copysign(np.float32(1.0) - e, x))


def quick_gelu(y, exp_steps=0, rcp_steps=0):
    """t = y * QGELU_K; e = exp2(t); d = 1 + e; r = 1 / d; q = y * r."""
    y = np.asarray(y, np.float32)
    e = exp2_f32(y * QGELU_K, exp_steps)
    with np.errstate(over="ignore"):
        d = np.float32(1.0) + e
        r = ulp_step((1.0 / d.astype(np.float64)).astype(np.float32), rcp_steps)
    return y * r


def gelu_f64(y):
    """0.5 y erfc(-y / sqrt 2) in float64 (no cancellation in the negative tail)."""
    y = np.asarray(y, np.float64)
    return 0.5 * y * np.vectorize(math.erfc, otypes=[np.float64])(-y / math.sqrt(2.0))


def quick_gelu_f64(y):
    y = np.asarray(y, np.float64)
    return y / (1.0 + np.exp(-1.702 * y))


def half_ulp_bf16(g):
    """Half a bf16 ulp of |g| (normal range): 2^(floor(log2 |g|) - 8); 0 for 0."""
    g = np.abs(np.asarray(g, np.float64))
    with np.errstate(divide="ignore"):
        return np.where(g > 0, 2.0 ** (np.floor(np.log2(np.where(g > 0, g, 1.0))) - 8), 0.0)


GELU_HEADER_SHARE = 0.05      # include/vit_hip_kernels.h: the error stays below 5 % of half a bf16 ulp (for y >= -4 sqrt 2)
GELU_STATED_SHARE = 0.044     # csrc/vit_gemm_common.hpp: at most 4.4 % of half a bf16 ulp ...
GELU_STATED_ABS = 4.75e-6     # ... and 4.7e-6 absolute, with the rounding of the printed figure
GELU_FLOOR = 4.4e-8           # below the clamp the kernel returns the constant -t exp2(Q(t)) = -4.36e-8 where gelu tends to 0
GELU_FLOOR_GPU = 4.5e-8       # the GPU test's interval below the clamp: [-4.5e-8, 0]


def sweep_cpu():
    """fp32 pre-activations of the CPU test: dense over [-12, 12], and logarithmic toward 0 from both sides."""
    dense = np.linspace(-12.0, 12.0, 400001).astype(np.float32)
    log = (2.0 ** np.linspace(-40.0, 2.0, 20001)).astype(np.float32)
    return np.unique(np.concatenate([dense, log, -log]))


def sweep_gemm(M=257, N=256):
    """The sweep that goes through a GEMM: A[m][0] = a_m on the bf16 grid of sixteenths over [-8, 8], W[n][0] = 1, bias[n] a jittered
    fp32 ladder inside one grid step; y[m][n] = fp32(a_m + bias[n]) is exactly what the epilogue's first addition gives."""
    a = (np.arange(M, dtype=np.float32) - np.float32(M // 2)) * np.float32(16.0 / (M - 1))
    assert np.array_equal(rne_bf16(a), a)
    step = 16.0 / (M - 1)
    bias = ((np.arange(N, dtype=np.float64) + u(30, (N,), 0.0, 1.0).astype(np.float64)) * (step / N)).astype(np.float32)
    return a, bias, a[:, None] + bias[None, :]


def sweep_operands(a, N, K):
    A = np.zeros((a.size, K), np.float32)
    A[:, 0] = a
    W = np.zeros((N, K), np.float32)
    W[:, 0] = 1.0
    return A, W


def activation_share(model, exact, y, **steps):
    """max |model(y) - exact(y)| / (half a bf16 ulp of exact(y)) over y, and the max absolute error."""
    g = exact(y)
    e = np.abs(model(y, **steps).astype(np.float64) - g)
    h = half_ulp_bf16(g)
    return float((e[h > 0] / h[h > 0]).max()), float(e.max())


def quick_gelu_share(y):
    """The five-step sequence's worst error in half bf16 ulps of the result, over +-1 ulp on v_exp_f32 and on v_rcp_f32."""
    return max(activation_share(quick_gelu, quick_gelu_f64, y, exp_steps=a, rcp_steps=b)[0] for a in (-1, 0, 1) for b in (-1, 0, 1))


def quick_gelu_d_share():
    """d of the GPU test's QuickGELU bar as a share of half a bf16 ulp: the five-step sequence's worst error over +-1 ulp on v_exp_f32
    and v_rcp_f32, on the GPU test's own sweep, doubled.  (QGELU_K is the fp32 rounding of -1.702 log2 e, which the float64 reference does
    not share: that is inside the figure.)"""
    return 2.0 * quick_gelu_share(sweep_gemm()[2])


def emulated_differ_share(y, which):
    """The largest share of bf16 results that are not rne_bf16 of the exact value, over the emulation's +-1 ulp variants."""
    if which == "gelu":
        g = gelu_f64(y)
        return max(differ_share(bits16(gelu_bf16(y, exp_steps=s)), g) for s in (-1, 0, 1))
    g = quick_gelu_f64(y)
    return max(differ_share(bits16(quick_gelu(y, exp_steps=a, rcp_steps=b)), g) for a in (-1, 0, 1) for b in (-1, 0, 1))


# ---- mutants: what a subtly wrong kernel would store (tests/test_bf16_gemm_model.py shows which check of section 3 rejects each) ----------

def shifted_bias(bias):
    """The bias of the other tile parity: columns shifted by one 256-column tile (wrapping inside the vector)."""
    return np.roll(np.asarray(bias), -TILE)


def rows_below(rows, by=8):
    idx = np.minimum(np.arange(rows.shape[0]) + by, rows.shape[0] - 1)
    return rows[idx]


def swap_x16_pieces(x16, row):
    """One row's first two 8-element pieces exchanged (what a lane pair does that trades the wrong halves)."""
    out = np.array(x16)
    out[row, 0:8], out[row, 8:16] = x16[row, 8:16], x16[row, 0:8]
    return out


def strip_to_neighbour(part, strip, row):
    """One row's partial of `strip` written one strip further (the two exchanged)."""
    out = np.array(part)
    out[strip, row], out[strip + 1, row] = part[strip + 1, row], part[strip, row]
    return out


MUTANTS = ("truncating store", "acc rounded to bf16 before the bias", "bias of the other tile parity", "last K step dropped",
           "colsum with the wrong sign", "row pairs of the row 8 below", "x16 pieces exchanged", "partial in the neighbouring strip")
# mutant -> the checks of section 3 that reject it at MUTANT_SHAPE ("integer": the bit-exact family, "random": the float64 bars;
# tests/test_bf16_gemm_model.py asserts this table).  The two one-sided entries and their reasons:
#   acc rounded before the bias   integer accumulators up to 256 ARE bf16 values: the integer family cannot see the extra rounding,
#                                 the random family does (2^-9 of the accumulator against a bar of 1e-6).
#   partial in the neighbouring strip   the random family looks at the finalised pairs, and those are sums over the strips: moving a
#                                 partial between strips leaves them as they were.  The integer family compares strip by strip.
REJECTED_BY = {
    "truncating store": ("integer", "random"),
    "acc rounded to bf16 before the bias": ("random",),
    "bias of the other tile parity": ("integer", "random"),
    "last K step dropped": ("integer", "random"),
    "colsum with the wrong sign": ("integer", "random"),
    "row pairs of the row 8 below": ("integer", "random"),
    "x16 pieces exchanged": ("integer", "random"),
    "partial in the neighbouring strip": ("integer",),
}
