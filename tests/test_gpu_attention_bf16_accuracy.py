"""The bf16 attention kernels -- attention_bf16_kernel (resident, up to 224 tokens), attention_bf16_stream_kernel (225 - 704),
attention_bf16_chunked_kernel (beyond), attention_hd_kernel<.., bf16, ..> (head dims 72 - 128) and the class-row kernel -- bit for bit
on operands whose sums are exact, and against float64 at bars of the size of the arithmetic.  tests/test_gpu_bf16.py and
tests/test_gpu_attention_hd.py hold them to 2^-8 |ref| + 1e-3 on U(-1.5, 1.5) inputs: a P that is truncated instead of rounded and a
truncating output store pass those (tests/test_attention_bf16_model.py shows it, and which bar here rejects each).
attention_bf16_model (A) holds the families, the kernels' model and the bars; its docstring states what the kernels share and where
they differ.

  tier I   integer operands, q_scaled entries (A.INTEGER_FAMILIES): every p a power of two, every sum exact in fp32 in any order, so
           the output is rne_bf16 of the exact o / l with no model of any instruction.  Elements within 2^-20 of a rounding boundary
           are left out (at most 0.5 %); an element whose top-plateau sum is exactly 0 is bounded instead: by 2^-40 where the row's
           top plateau is walked first, by one unit of the matrix instruction's 24-bit frame where lower keys precede it
           (A.FRAME_UNIT: the instruction cuts a negative accumulator 2^-56 below its products to minus one unit).  The class rows
           (fp32 p / l) are within 2 fp32 ulp of the exact quotient.  Three images of three heads, each with data of its own.
  tier II  attention_split_model.family_inputs rounded to bf16, seed ACCURACY_SEED, one image of two heads, plain and q_scaled:
           (a) every output between rne_bf16(ref - bar) and rne_bf16(ref + bar), bar = 2^-8 A + 4 e_seq + 2^-23 |ref|max with
               A = sum p |v| / sum p (one rounding of every p, in numerator and denominator, then the fp32 bar of
               tests/test_gpu_attention_accuracy.py);
           (b) the share of outputs that are not rne_bf16(ref) at most twice the model's, plus the share of outputs whose model value
               lies within 4 e_seq + 2^-23 |ref|max of a rounding boundary; 0 where that allowance is 0 (one-hot, constant-V);
           (c) the mean of (got - ref) / A within the model's mean +- 4 standard errors;
           (d) constant-V: every output row is the bits of the row.
           The class rows are fp32: e <= 4 e_seq + 2^-23 |ref|max, e_seq over all query rows of the image.

Token counts: 33 (ragged single tile), 197 (the workload), 224 (the resident kernel's full last tile), 225 and 704 (the stream
kernel's first and last length), 257 (a fifth 64-key sub-chunk), 705 (chunked).  Measured on the MI355X:
profiles/r34/bf16_attention_accuracy.md.
"""
import functools
import time

import numpy as np
import pytest

import attention_bf16_model as A
import attention_split_model as M
from vit_amd import binding as B

pytestmark = pytest.mark.gpu

TOKENS_64 = [33, 197, 224, 225, 257, 704, 705]
TOKENS_HD = [33, 197, 257]
TOKENS_II_64 = [33, 197, 225, 257, 705]   # tier II leaves out 224 and 704: the host's float64 side is what takes the time

PV = {  # name: (head_dim, q_scaled, the call on n images)
    "bf16io": (64, False, lambda bits, n, T, heads: B.attention_bf16io(bits, n, T, heads)),
    "bf16io-qscaled": (64, True, lambda bits, n, T, heads: B.attention_bf16io(bits, n, T, heads, q_scaled=True)),
    "hd72": (72, False, lambda bits, n, T, heads: B.attention_bf16io_hd(bits, n, T, heads, 72)),
    "hd72-qscaled": (72, True, lambda bits, n, T, heads: B.attention_bf16io_hd(bits, n, T, heads, 72, q_scaled=True)),
    "hd128": (128, False, lambda bits, n, T, heads: B.attention_bf16io_hd(bits, n, T, heads, 128)),
    "hd128-qscaled": (128, True, lambda bits, n, T, heads: B.attention_bf16io_hd(bits, n, T, heads, 128, q_scaled=True)),
}
CLS = {  # name: (head_dim, q_scaled, the call) -> [n][heads][T] fp32
    "cls": (64, False, lambda bits, n, T, heads: B.cls_attention_bf16(bits, n, T, heads)),
    "cls-qscaled": (64, True, lambda bits, n, T, heads: B.cls_attention_bf16(bits, n, T, heads, q_scaled=True)),
    "cls-hd72": (72, False, lambda bits, n, T, heads: B.cls_attention_bf16_hd(bits, n, T, heads, 72)),
    "cls-hd72-qscaled": (72, True, lambda bits, n, T, heads: B.cls_attention_bf16_hd(bits, n, T, heads, 72, q_scaled=True)),
}


def tokens_of(head_dim, tier):
    if head_dim != 64:
        return TOKENS_HD
    return TOKENS_64 if tier == 1 else TOKENS_II_64


def pv_cases(tier):
    return [(e, T) for e, (hd, qs, _) in PV.items() if qs or tier == 2 for T in tokens_of(hd, tier)]


def cls_cases(tier):
    return [(e, T) for e, (hd, qs, _) in CLS.items() if qs or tier == 2 for T in TOKENS_HD]


@pytest.fixture(scope="module", autouse=True)
def wall_time():
    t0 = time.perf_counter()
    yield
    print(f"\ntest_gpu_attention_bf16_accuracy.py: {time.perf_counter() - t0:.1f} s wall time")


def frozen(a):
    a.setflags(write=False)
    return a


# ---- tier I ------------------------------------------------------------------------------------------------------------------------------

IMAGES, HEADS_I = 3, 3


@functools.lru_cache(maxsize=None)
def integer_case(family, T, head_dim):
    """The bits the entries read and, per (image, head), what integer_expected says."""
    qkv = A.integer_inputs(family, T, head_dim, HEADS_I, IMAGES)
    bits = B.to_bf16_bits(qkv).reshape(qkv.shape)
    assert np.array_equal(B.from_bf16_bits(bits).reshape(qkv.shape), qkv)  # small integers are bf16 values
    want = {}
    for i in range(IMAGES):
        for h in range(HEADS_I):
            q, k, v = M.head_operands(qkv[i * T:(i + 1) * T], HEADS_I, head_dim, h)
            width, _, gap = A.integer_width(q, k, v)
            assert width <= 23 and gap >= A.TOP_WINDOW
            want[i, h] = A.integer_expected(q, k, v) + (A.zero_bound(q, k, v),)
    return frozen(bits), want


@pytest.mark.parametrize("family", A.INTEGER_FAMILIES)
@pytest.mark.parametrize("entry,T", pv_cases(1))
def test_integer_operands_give_the_bits_of_the_exact_quotient(entry, T, family):
    head_dim, _, run = PV[entry]
    bits, want = integer_case(family, T, head_dim)
    got = run(bits, IMAGES, T, HEADS_I).reshape(IMAGES * T, HEADS_I * head_dim)
    wrong = left = zeros = n = 0
    zero_top, zero_ratio, first = 0.0, 0.0, None
    for (i, h), (exp_bits, compared, zero, _, bound) in want.items():
        g = got[i * T:(i + 1) * T, h * head_dim:(h + 1) * head_dim]
        bad = (g != exp_bits) & compared
        if bad.any() and first is None:
            r, d = np.argwhere(bad)[0]
            first = (i, h, int(r), int(d), hex(int(g[r, d])), hex(int(exp_bits[r, d])))
        wrong += int(bad.sum())
        left += int((~compared & ~zero).sum())
        zeros += int(zero.sum())
        n += g.size
        if zero.any():
            zero_top = max(zero_top, float(np.abs(A.values(g[zero])).max()))
            zero_ratio = max(zero_ratio, float((np.abs(A.values(g)) / bound[:, None])[zero].max()))
    print(f"{entry} {family} T {T} ({A.kernel_of(head_dim, T)}): {wrong} of {n} differ from rne_bf16(o / l)  left out {100 * left / n:.3f} %  "
          f"zero sums {zeros}, largest |output| there {zero_top:.3e}, {zero_ratio:.3f} of its bound")
    assert left <= 0.005 * n
    assert wrong == 0, (entry, family, T, wrong, first)
    assert zero_ratio <= 1.0, (entry, family, T, zero_top, zero_ratio)


@pytest.mark.parametrize("family", A.INTEGER_FAMILIES)
@pytest.mark.parametrize("entry,T", cls_cases(1))
def test_integer_class_rows_are_the_exact_quotient(entry, T, family):
    """p / l in fp32: p a power of two, l exact, one division -- within 2 fp32 ulp of the exact quotient.  The count of rows that are
    not the correctly rounded quotient is printed: 0 means exp2f gave the exact powers of two."""
    head_dim, _, run = CLS[entry]
    bits, want = integer_case(family, T, head_dim)
    got = run(bits, IMAGES, T, HEADS_I)
    worst, inexact = 0.0, 0
    for (i, h), (_, _, _, p, _) in want.items():
        exact = p[0]
        ulp = np.spacing(exact.astype(np.float32)).astype(np.float64)
        off = np.abs(got[i, h].astype(np.float64) - exact) / ulp
        worst = max(worst, float(off.max()))
        inexact += int((got[i, h] != exact.astype(np.float32)).sum())
    print(f"{entry} {family} T {T}: {worst:.2f} ulp from the exact p / l, {inexact} of {IMAGES * HEADS_I * T} are not its fp32 rounding")
    assert worst <= 2.0, (entry, family, T, worst)


# ---- tier II -----------------------------------------------------------------------------------------------------------------------------

HEADS = 2


@functools.lru_cache(maxsize=None)
def rounded_inputs(family, T, head_dim, q_scaled):
    """(bits [T][3D], their values, info): the family's fp32 inputs rounded to bf16; q_scaled: the Q columns hold scale_f32(head_dim) * q,
    rounded, and the exponent is their plain product with K."""
    vals, info = M.family_inputs(family, T, head_dim, HEADS, M.ACCURACY_SEED)
    vals = vals.copy()
    if q_scaled:
        vals[:, :HEADS * head_dim] *= M.scale_f32(head_dim)
    bits = B.to_bf16_bits(vals).reshape(vals.shape)
    return frozen(bits), frozen(B.from_bf16_bits(bits).reshape(vals.shape)), info


@functools.lru_cache(maxsize=None)
def float64_case(family, T, head_dim, q_scaled):
    """Everything the CPU says about the rounded inputs, once: the float64 reference, A, e_seq, and the bars from the model of the
    kernel that takes the shape."""
    _, vals, _ = rounded_inputs(family, T, head_dim, q_scaled)
    heads = [M.head_operands(vals, HEADS, head_dim, h) for h in range(HEADS)]
    refs = [A.reference(q, k, v, head_dim, q_scaled) for q, k, v in heads]
    ref, Aa = (np.concatenate([r[j] for r in refs], axis=1) for j in range(2))
    seq = np.concatenate([M.attention_f32_sequential(q, k, v, head_dim, q_scaled) for q, k, v in heads], axis=1)
    e_seq = float(np.abs(seq - ref).max())
    model = [A.kernel_model(A.kernel_of(head_dim, T), q, k, v, head_dim, q_scaled) for q, k, v in heads]
    pre, mbits = (np.concatenate([m[j] for m in model], axis=1) for j in range(2))
    return frozen(ref), frozen(Aa), e_seq, A.tier2_bars(ref, Aa, e_seq, pre, mbits)


@pytest.mark.parametrize("family", M.FAMILIES)
@pytest.mark.parametrize("entry,T", pv_cases(2))
def test_rounded_families_against_float64(entry, T, family):
    head_dim, q_scaled, run = PV[entry]
    bits, _, _ = rounded_inputs(family, T, head_dim, q_scaled)
    ref, Aa, e_seq, bars = float64_case(family, T, head_dim, q_scaled)
    got = run(bits, 1, T, HEADS).reshape(T, HEADS * head_dim)
    c = A.tier2_check(got, ref, Aa, bars)
    margin = float((np.abs(A.values(got) - ref) / bars["bar_a"]).max())
    print(f"{entry} {family} T {T} ({A.kernel_of(head_dim, T)}): e_kernel {c['e_kernel']:.3e}  e_seq {e_seq:.3e}  floor {bars['floor']:.3e}  "
          f"(a) outside {c['outside']}, max e / bar {margin:.2f} (< 1 + half a bf16 ulp / bar)  (b) share {100 * c['share']:.3f} % model {100 * bars['model_share']:.3f} % "
          f"cap {100 * bars['cap']:.3f} %  (c) mean {c['mean']:+.3e} model {bars['mean']:+.3e} +- {4 * bars['se']:.3e}")
    assert "a" not in c["missed"], (entry, family, T, c["outside"], tuple(np.argwhere(A.outside_bracket(got, ref, bars["bar_a"]))[0]))
    assert "b" not in c["missed"], (entry, family, T, c["share"], bars["cap"])
    assert "c" not in c["missed"], (entry, family, T, c["mean"], bars["mean"], bars["se"])
    if family == "constant-V":  # (d)
        row = bits[0, 2 * HEADS * head_dim:]
        assert np.array_equal(bits[:, 2 * HEADS * head_dim:], np.broadcast_to(row, (T, row.size)))
        off = int((got != row[None, :]).sum())
        print(f"    {off} elements are not the constant row's bits")
        assert off == 0, (entry, T, off)


@functools.lru_cache(maxsize=None)
def class_row_case(family, T, head_dim, q_scaled):
    """(ref [heads][T] float64: the class row's softmax, the fp32 bar with e_seq taken over ALL query rows of the image: one row is a
    small sample of the arithmetic's error at this shape, and the bar's form is made for an image's maximum)."""
    _, vals, _ = rounded_inputs(family, T, head_dim, q_scaled)
    eye = np.eye(T, dtype=np.float32)
    ref, e_seq = [], 0.0
    for h in range(HEADS):
        q, k, _ = M.head_operands(vals, HEADS, head_dim, h)
        full = M.attention_f64(q, k, eye, head_dim, q_scaled)
        e_seq = max(e_seq, float(np.abs(M.attention_f32_sequential(q, k, eye, head_dim, q_scaled) - full).max()))
        ref.append(full[0])
    ref = np.stack(ref)
    return frozen(ref), e_seq, A.fp32_bar(e_seq, float(np.abs(ref).max()))


@pytest.mark.parametrize("family", M.FAMILIES)
@pytest.mark.parametrize("entry,T", cls_cases(2))
def test_class_rows_against_float64(entry, T, family):
    head_dim, q_scaled, run = CLS[entry]
    bits, _, _ = rounded_inputs(family, T, head_dim, q_scaled)
    ref, e_seq, bar = class_row_case(family, T, head_dim, q_scaled)
    got = run(bits, 1, T, HEADS)[0]
    e = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{entry} {family} T {T}: e_kernel {e:.3e}  e_seq {e_seq:.3e}  bar {bar:.3e}")
    assert np.isfinite(got).all() and e <= bar, (entry, family, T, e, bar)
