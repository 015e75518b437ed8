"""A numpy model of the bf16 attention kernels (routes 3, 4, 5 and 7 of csrc/vit_attention.hip and the class-row kernel), the integer
operand families on which their outputs are exact, and the bars tests/test_gpu_attention_bf16_accuracy.py holds them to.  No GPU;
tests/test_attention_bf16_model.py shows that the bars tell wrong kernels from a right one.

What the kernels share, and attention_bf16() does: scores in fp32 from the bf16 operands (the products are exact, one rounding of
their sum); p = exp2(fma(s, c, -m c)), or exp2(s - m) when the Q columns hold c q (q_scaled); P rounded to bf16 once; O accumulated in
fp32, sixteen keys per step; one multiplication by the fp32 reciprocal of the row sum; a bf16 store.  Where they differ (KERNELS):

  resident  attention_bf16_kernel, <= 224 keys           m the row's maximum; the row sum on the matrix pipe, of p AS ROUNDED
  stream    attention_bf16_stream_kernel, 225 - 704      64-key units, m a reference that moves when outgrown by more than 2^8; the sum
                                                         of the fp32 p
  chunked   attention_bf16_chunked_kernel, > 704         224-key chunks, m the running maximum (it moves whenever outgrown); fp32 p
  hd        attention_hd_kernel<.., bf16, ..>, 72 - 128  32-key tiles, the deferred reference; the sum of the fp32 p; and P goes to the
                                                         matrix pipe in TWO bf16 pieces, bf16(p) and bf16(p - bf16(p)): 16 bits of p

The model does not follow the matrix instruction's internal cuts (attention_split_model.mfma does, for the split kernel): the bars of
tier II are made of the float64 reference and of the share of outputs this model rounds the other way, not of its bits.

Tier I needs no model at all: on the integer families below every p is a power of two and every sum exact in fp32, so the output is
the correctly rounded quotient of two integers (integer_expected).
"""
import numpy as np

import attention_split_model as M

DEFER = 8.0
KERNELS = {  # name: (tile, defer, rounded_sum, p_pieces); tile None: one maximum over the row
    "resident": (None, None, True, 1),
    "stream": (64, DEFER, False, 1),
    "chunked": (224, 0.0, False, 1),
    "hd": (32, DEFER, False, 2),
}


def kernel_of(head_dim, T):
    """The kernel behind a bf16 P.V entry at this shape (route() in csrc/vit_attention.hip)."""
    if head_dim != 64:
        return "hd"
    return "resident" if T <= 224 else "stream" if T <= 704 else "chunked"


def f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def rne(x):
    """fp32 -> the nearest bf16 value (ties to even), as fp32"""
    return M.bf16_rne(x)


def trunc(x):
    """fp32 -> bf16 by dropping the low 16 bits (the mutants' rounding)"""
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def bits16(x):
    """the bits of bf16 values held in fp32"""
    return (np.ascontiguousarray(x, np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def rne_bits(x):
    """float64 or fp32 -> the bits of the nearest bf16.  Through fp32: the two roundings differ from one only within 2^-24 of a bf16
    rounding boundary."""
    return bits16(rne(f32(x)))


def attention_bf16(q, k, v, head_dim, q_scaled, rounded_sum, p_round=rne, store=rne, tile=None, defer=DEFER, p_pieces=1, group=16,
                   exp_ulps=0, mask_last=False, skip_rescale=False):
    """q [Tq][head_dim], k, v [T][head_dim]: bf16 values in fp32 -> (the fp32 value in front of the store [Tq][head_dim], the stored
    bits).  tile / defer: the keys are walked `tile` at a time and the reference m moves to a tile's maximum when that is more than
    `defer` above it in the exponent (None: one pass, m the row's maximum).  rounded_sum: the row sum is taken of the rounded p (in
    fp32 otherwise).  p_pieces: the bf16 pieces of p that reach P.V.  group: keys per rounding of the O accumulator.  exp_ulps: every
    exponential is moved by so many fp32 ulps (v_exp_f32 is within 1).  The mutants of the CPU test: p_round / store = trunc;
    mask_last: the last key is left out; skip_rescale: O and the row sum are not rescaled when the reference moves."""
    q, k, v = (np.asarray(a, np.float32) for a in (q, k, v))
    Tq, T = q.shape[0], k.shape[0]
    c = np.float32(1.0) if q_scaled else M.scale_f32(head_dim)
    s = f32(q.astype(np.float64) @ k.astype(np.float64).T)
    if mask_last:
        s[:, T - 1] = -np.inf
    v64 = v.astype(np.float64)
    o = np.zeros((Tq, v.shape[1]), np.float32)
    l = np.zeros(Tq, np.float32)
    m = np.full(Tq, -np.inf, np.float32)
    step = T if tile is None else tile
    for t0 in range(0, T, step):
        st = s[:, t0:t0 + step]
        cmax = st.max(1)
        with np.errstate(invalid="ignore"):
            grow = f32((cmax - m).astype(np.float32).astype(np.float64) * c)
            moved = (grow > (0.0 if tile is None else defer)) | np.isinf(m)
            m_new = np.where(moved, cmax, m).astype(np.float32)
            alpha = f32(np.exp2(f32((m - m_new).astype(np.float32).astype(np.float64) * c).astype(np.float64)))
        alpha = np.where(moved, alpha, np.float32(1.0)).astype(np.float32)
        if skip_rescale:
            alpha = np.where(np.isinf(m), alpha, np.float32(1.0)).astype(np.float32)
        m = m_new
        if q_scaled:
            e = (st - m[:, None]).astype(np.float32)
        else:
            e = f32(st.astype(np.float64) * c + f32(-m.astype(np.float64) * c)[:, None].astype(np.float64))
        p = f32(np.exp2(e.astype(np.float64)))
        if exp_ulps:
            p = (p.astype(np.float64) + exp_ulps * np.spacing(p).astype(np.float64)).astype(np.float32)
        hi = p_round(p)
        P = hi.astype(np.float64)
        if p_pieces == 2:
            P = P + p_round((p - hi).astype(np.float32)).astype(np.float64)
        o = o * alpha[:, None]
        l = l * alpha
        for g0 in range(0, st.shape[1], group):
            o = f32(o.astype(np.float64) + P[:, g0:g0 + group] @ v64[t0 + g0:t0 + g0 + group])
            l = f32(l.astype(np.float64) + (P if rounded_sum else p.astype(np.float64))[:, g0:g0 + group].sum(1))
    pre = o * (np.float32(1.0) / l)[:, None]
    return pre, bits16(store(pre))


def kernel_model(name, q, k, v, head_dim, q_scaled, **kw):
    tile, defer, rounded_sum, p_pieces = KERNELS[name]
    return attention_bf16(q, k, v, head_dim, q_scaled, rounded_sum, tile=tile, defer=defer, p_pieces=p_pieces, **kw)


# ---- tier I: integer operands ------------------------------------------------------------------------------------------------------------
# Q and K in {-1, 0, 1}, one element in eight non-zero; column 0 of Q +-1 per row, column 0 of K a level L_j; V an integer in -2 .. 2.
# With q_scaled the exponent is the plain product: an integer, p a power of two, exact in bf16; the accumulators and the row sum are
# exact in fp32 in any order as long as a row's scores spread over few enough bits (integer_width), whatever a deferred reference does.

INTEGER_FAMILIES = ("flat-rise", "plateau")
FLAT_RISE = 4                # L_j = round(FLAT_RISE (j / (T - 1))^2)
PLATEAU, PLATEAUS = 56, 3    # L_j = PLATEAU floor(PLATEAUS j / T): levels 2^56 apart, the jumps inside tiles and chunks
TOP_WINDOW = 40              # keys within 2^-TOP_WINDOW of a row's maximum are its top plateau; the others are 2^-PLATEAU + noise below
NEAR_BOUNDARY = 2.0 ** -20   # an element this close (relative) to a bf16 rounding boundary is left out
ZERO_SUM_BOUND = 2.0 ** -40  # |output| of an element whose top-plateau sum is exactly 0 ...
# ... in a row whose top plateau is walked first.  Where lower keys come first the accumulator holds their sum, 2^-56 of a product
# of the top plateau, when that plateau's first products arrive, and v_mfma_f32_32x32x16_bf16 cuts the accumulator TOWARD MINUS
# INFINITY to the 24-bit frame of the products (attention_split_model.mfma_add, profiles/r31): a negative one becomes minus one unit
# of the frame, 2^(E - 24) with E the exponents of p and v added, and stays when the plateau's sum is 0.  The bound there: that unit at
# the row's largest p and |v| = 2, over l, and the bf16 rounding of the store.
FRAME_UNIT = 2.0 ** -23 * (1.0 + 2.0 ** -8)
INTEGER_SEED = 2034


def levels(family, T):
    j = np.arange(T, dtype=np.float64)
    if family == "flat-rise":
        return np.round(FLAT_RISE * (j / max(T - 1, 1)) ** 2)
    if family == "plateau":
        return PLATEAU * np.floor(PLATEAUS * j / T)
    raise ValueError(family)


def integer_inputs(family, T, head_dim, heads, images, seed=INTEGER_SEED):
    """qkv [images * T][3 * heads * head_dim] fp32, small integers, every image and head with data of its own."""
    from vit_amd import synth
    D = heads * head_dim
    n = images * T

    def sparse(index):
        u = synth.uniform(seed, index, n * D, 0.0, 1.0).reshape(n, D)
        return np.where(u < 1.0 / 16, -1.0, np.where(u >= 15.0 / 16, 1.0, 0.0)).astype(np.float32)

    q, k = sparse(0), sparse(1)
    v = np.floor(synth.uniform(seed, 2, n * D, 0.0, 5.0)).reshape(n, D).astype(np.float32) - np.float32(2.0)
    sign = np.where(synth.uniform(seed, 3, n * heads, 0.0, 1.0) < 0.5, -1.0, 1.0).astype(np.float32).reshape(n, heads)
    q[:, 0::head_dim] = sign
    k[:, 0::head_dim] = np.tile(levels(family, T), images)[:, None].astype(np.float32)
    return np.ascontiguousarray(np.concatenate([q, k, v], axis=1))


def integer_head(q, k, v):
    """One head of an integer family in float64: (e [Tq][T] the exponents below the row's maximum, top [Tq][T] the keys of the top
    plateau, o [Tq][d] and l [Tq] the top plateau's exact sums, rest [Tq][d] what the keys below it add to o, to float64's precision)."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    s = q @ k.T
    e = s - s.max(1, keepdims=True)
    top = e >= -TOP_WINDOW
    p_top = np.where(top, np.exp2(np.maximum(e, -TOP_WINDOW)), 0.0)
    p_low = np.where(top, 0.0, np.exp2(e))
    return e, top, p_top @ v, p_top.sum(1), p_low @ v


def integer_width(q, k, v):
    """(bits, loose, gap).  bits: the most bits any partial sum of a row's top plateau can need, in any order: every term p_j v_jd and
    every p_j is a multiple of the row's smallest p, and no partial sum exceeds sum_j p_j max|v| -- ceil(log2) of that sum in units
    of the smallest p.  loose: the simpler sufficient figure, the spread of the row's exponents plus ceil(log2(T max|v|)), which
    counts every key at the row's maximum.  gap: the least distance in the exponent from a row's top plateau to a key below it
    (inf if none)."""
    e, top, _, _, _ = integer_head(q, k, v)
    e_min = np.where(top, e, 0.0).min(1, keepdims=True)
    vmax = max(float(np.abs(v).max()), 1.0)
    bits = float(np.ceil(np.log2(np.where(top, np.exp2(e - e_min), 0.0).sum(1) * vmax)).max())
    loose = float(-e_min.min()) + float(np.ceil(np.log2(k.shape[0] * vmax)))
    below = np.where(top, -np.inf, e)
    gap = float(-below.max()) if np.isfinite(below).any() else float("inf")
    return bits, loose, gap


def boundary_distance(x):
    """The distance of x to the nearest bf16 rounding boundary (the midpoint of two neighbouring bf16 values), relative to |x|; inf
    at 0."""
    a = np.abs(np.asarray(x, np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        ulp = np.exp2(np.floor(np.log2(a)) - 7.0)
        frac = np.mod(a / ulp, 1.0)
        return np.where(a > 0, np.abs(frac - 0.5) * ulp / a, np.inf)


def integer_expected(q, k, v):
    """(bits [Tq][d]: rne_bf16 of the exact o / l; compared [Tq][d]: not within NEAR_BOUNDARY of a rounding boundary; zero [Tq][d]:
    the top-plateau sum is exactly 0, the output is bounded by zero_bound(q, k, v) instead; p [Tq][T]: the exact row p / l in
    float64)."""
    e, top, o, l, rest = integer_head(q, k, v)
    exact = (o + rest) / l[:, None]
    zero = o == 0.0
    compared = (boundary_distance(exact) > NEAR_BOUNDARY) & ~zero
    return rne_bits(exact), compared, zero, np.exp2(e) / (l + np.where(top, 0.0, np.exp2(e)).sum(1))[:, None]


def zero_bound(q, k, v):
    """[Tq]: the bound on |output| where a row's top-plateau sum is exactly 0: ZERO_SUM_BOUND where the top plateau is walked first
    (the kernels walk the keys forwards), FRAME_UNIT max p / l where lower keys precede it."""
    e, top, _, l, _ = integer_head(q, k, v)
    preceded = ~top[:, 0]
    return np.where(preceded, FRAME_UNIT * np.exp2(e).max(1) / l, ZERO_SUM_BOUND)


def mfma_pv(q, k, v):
    """o / l of an integer head with P.V on attention_split_model.mfma, sixteen keys per instruction in the half-waves' order, one
    maximum per row: what the instruction's cuts do to the exact sums (the CPU test)."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    T = k.shape[0]
    s = q @ k.T
    pad = (T + 15) // 16 * 16
    P, V = np.zeros((q.shape[0], pad), np.float32), np.zeros((pad, v.shape[1]), np.float32)
    P[:, :T], V[:T] = np.exp2(s - s.max(1, keepdims=True)), v
    o = np.zeros((q.shape[0], v.shape[1]), np.float32)
    for g0 in range(0, pad, 16):
        o = M.mfma(o, P[:, g0 + M.PV_K_ORDER], V[g0 + M.PV_K_ORDER].T)
    return o * (np.float32(1.0) / f32(P.astype(np.float64).sum(1)))[:, None]


def fp32_walk(q, k, v, tile, defer, backwards=False):
    """o / l of an integer head in fp32 arithmetic, the keys walked `tile` at a time (tile None: one maximum), forwards or backwards,
    every addition a rounded fp32 addition in key order: the order-independence check of the CPU test."""
    q, k, v = (np.asarray(a, np.float32) for a in (q, k, v))
    Tq, T = q.shape[0], k.shape[0]
    s = f32(q.astype(np.float64) @ k.astype(np.float64).T)
    order = np.arange(T)[::-1] if backwards else np.arange(T)
    o, l = np.zeros((Tq, v.shape[1]), np.float32), np.zeros(Tq, np.float32)
    m = np.full(Tq, -np.inf, np.float32) if tile is not None else s.max(1)
    step = T if tile is None else tile
    for t0 in range(0, T, step):
        keys = order[t0:t0 + step]
        if tile is not None:
            cmax = s[:, keys].max(1)
            with np.errstate(invalid="ignore"):
                moved = ((cmax - m) > defer) | np.isinf(m)
                m_new = np.where(moved, cmax, m).astype(np.float32)
                alpha = np.where(moved, np.exp2((m - m_new).astype(np.float64)), 1.0).astype(np.float32)
            o, l, m = o * alpha[:, None], l * alpha, m_new
        for key in keys:
            p = np.exp2((s[:, key] - m).astype(np.float64)).astype(np.float32)
            assert np.array_equal(rne(p), p)
            l = l + p
            o = o + p[:, None] * v[key][None, :]
    return o * (np.float32(1.0) / l)[:, None]


# ---- tier II: the bars against float64 -----------------------------------------------------------------------------------------------------

def reference(q, k, v, head_dim, q_scaled):
    """(ref [Tq][d] float64, A [Tq][d] = sum p |v| / sum p) of bf16-rounded operands"""
    return M.attention_f64(q, k, v, head_dim, q_scaled), M.attention_f64(q, k, np.abs(v), head_dim, q_scaled)


def fp32_bar(e_seq, top):
    """r29's bar of the fp32 entries: 4 e_seq + 2^-23 |ref|max"""
    return 4.0 * e_seq + 2.0 ** -23 * top


def bracket(ref, bar):
    """(lo, hi) as bf16 values in float64: rne_bf16(ref - bar), rne_bf16(ref + bar)"""
    return rne(f32(ref - bar)).astype(np.float64), rne(f32(ref + bar)).astype(np.float64)


def values(bits):
    return (np.asarray(bits).astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def outside_bracket(bits, ref, bar):
    lo, hi = bracket(ref, bar)
    got = values(bits)
    return ~((got >= lo) & (got <= hi))


def differ_share(bits, ref):
    """the share of outputs that are not rne_bf16(ref)"""
    return float((np.asarray(bits) != rne_bits(ref)).mean())


def near_share(pre, floor):
    """the share of outputs whose value in front of the store lies within `floor` (absolute) of a bf16 rounding boundary"""
    pre = np.asarray(pre, np.float64)
    return float((boundary_distance(pre) * np.abs(pre) <= floor).mean())


def bias(bits, ref, A):
    """(mean, standard error) of (got - ref) / A over the image"""
    x = (values(bits) - ref) / A
    return float(x.mean()), float(x.std() / np.sqrt(x.size))


def tier2_bars(ref, A, e_seq, model_pre, model_bits):
    """Everything tier II holds an image's output to: bar (a) per element, the floor 4 e_seq + 2^-23 |ref|max, the cap of (b), the
    model's share, and (c)'s interval.  The cap is twice the model's share plus the share of model outputs within the floor of a
    rounding boundary; where that is 0 -- one-hot and constant-V, whose model values ARE bf16 values -- the kernel's share must be 0.
    (Not: 0 wherever the model's own share is 0.  With the hd kernel's two pieces of P the model has 0 of 28,368 outputs off in
    families whose allowance is 0.2 %, and another grain of accumulation moves one or two across: profiles/r34.)"""
    floor = fp32_bar(e_seq, float(np.abs(ref).max()))
    share = differ_share(model_bits, ref)
    mean, se = bias(model_bits, ref, A)
    return dict(bar_a=2.0 ** -8 * A + floor, floor=floor, model_share=share, cap=2.0 * share + near_share(model_pre, floor),
                mean=mean, se=se)


def tier2_check(bits, ref, A, bars):
    """The figures of an output against the bars and which of (a), (b), (c) it misses."""
    out = int(outside_bracket(bits, ref, bars["bar_a"]).sum())
    share = differ_share(bits, ref)
    mean, _ = bias(bits, ref, A)
    missed = []
    if out:
        missed.append("a")
    if share > bars["cap"]:
        missed.append("b")
    if abs(mean - bars["mean"]) > 4.0 * bars["se"]:
        missed.append("c")
    return dict(outside=out, share=share, mean=mean, e_kernel=float(np.abs(values(bits) - ref).max()), missed=missed)


def inside_old_bar(bits, ref, floor=1e-3):
    """the bar of tests/test_gpu_bf16.py and tests/test_gpu_attention_hd.py: 2^-8 |ref| + 1e-3 (4e-3 in the streamed maximum test)"""
    return bool((np.abs(values(bits) - ref) <= 2.0 ** -8 * np.abs(ref) + floor).all())
