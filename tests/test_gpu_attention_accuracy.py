"""The accuracy of the fp32 attention entries against a float64 attention, at bars of the size of fp32 rounding -- the oracle tests
(tests/test_gpu_ops.py::test_attention, tests/test_gpu_attention_hd.py::test_fp32_matches_the_oracle, tests/test_gpu_attention_split.py
::test_matches_the_oracle) pin the reference's order of operations with bars of 1e-5 and more, about 80 times what the arithmetic
delivers.  Here every bar is a function of the float64 reference and of a CPU evaluation of the same inputs, or an exactness condition:

  (a) every fp32 entry:      e_kernel <= 4 e_seq + 2^-23 |ref|max.  e_seq: a sequential fp32 evaluation (attention_f32_sequential)
                             against float64; the factor 4 is the one tests/test_attention_split_model.py holds the split's model to;
                             the floor is one rounding of the output and one of the reciprocal of the row sum.
  (b) the split in addition: e_kernel <= 2 e_model + 2^-24 |ref|max, e_model from the numpy model of the kernel
                             (attention_split_model.attention_split), the form of tests/test_gpu_split_gemm.py.  A split that lost its
                             three small products is outside this bar in every family (the CPU test shows it).
  (c) one-hot rows:          the output is the selected V row, within 4 ulp in fp32 (1 ulp sequentially, one each for v_exp_f32 and
                             the reciprocal, one spare) and bit for bit in bf16 (a bf16 value times 1 + 1e-4 rounds back to itself).
  (d) constant V rows:       the output rows are that row, within (a) in fp32, and exactly 1.0 in bf16 when the row is 1.0.
  (e) V times 2^+-40:        the output times 2^+-40, bit for bit.

The errors are maxima over the image.  The input families are attention_split_model.family_inputs; one image, two heads (the second
head's columns are read at an offset); 33 keys (one past a 32-key tile), 197 (the workload), 257 (the chunked path of
vithip_attention_f32, a second 128-row workgroup and a fifth 64-key chunk of the streaming kernels).  vithip_attention_f32_rows and the
q_rows forms have the bits of these entries (test_gpu_ops.py, test_gpu_attention_hd.py, test_gpu_attention_split.py).

Measured on the MI355X: profiles/r29/attention_accuracy.md.  The bf16 entries beyond (c) and (d): tests/test_gpu_attention_bf16_accuracy.py.
"""
import functools

import numpy as np
import pytest

import attention_split_model as M
from vit_amd import binding as B

pytestmark = pytest.mark.gpu

HEADS = 2
TOKENS = [33, 197, 257]
ENTRIES = {  # name: (head_dim, the call on one image of two heads)
    "f32": (64, lambda qkv, T: B.attention(qkv, 1, T, HEADS)),            # resident up to 224 tokens, chunked beyond
    "hd72": (72, lambda qkv, T: B.attention_hd(qkv, 1, T, HEADS, 72)),    # the contraction padded to the MFMA's K step in bf16
    "hd128": (128, lambda qkv, T: B.attention_hd(qkv, 1, T, HEADS, 128)),
    "split": (64, lambda qkv, T: B.attention_split(qkv, 1, T, HEADS)),
}
BF16_ENTRIES = {  # name: (head_dim, q_scaled, the call)
    "bf16io": (64, False, lambda bits, T: B.attention_bf16io(bits, 1, T, HEADS)),
    "bf16io-qscaled": (64, True, lambda bits, T: B.attention_bf16io(bits, 1, T, HEADS, q_scaled=True)),
    "bf16io-hd72": (72, False, lambda bits, T: B.attention_bf16io_hd(bits, 1, T, HEADS, 72)),
}


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def case(family, T, head_dim):
    """The inputs and everything the CPU says about them, computed once: qkv, info, the float64 reference [T][heads * head_dim],
    |ref|max, e_seq and, at head_dim 64, e_model."""
    qkv, info = M.family_inputs(family, T, head_dim, HEADS, M.ACCURACY_SEED)
    heads = [M.head_operands(qkv, HEADS, head_dim, h) for h in range(HEADS)]
    ref = np.concatenate([M.attention_f64(q, k, v, head_dim) for q, k, v in heads], axis=1)
    seq = np.concatenate([M.attention_f32_sequential(q, k, v, head_dim) for q, k, v in heads], axis=1)
    c = dict(qkv=frozen(qkv), info=info, ref=frozen(ref), top=float(np.abs(ref).max()), e_seq=float(np.abs(seq - ref).max()), e_model=None)
    if head_dim == 64:
        model = np.concatenate([M.attention_split(q, k, v) for q, k, v in heads], axis=1)
        c["e_model"] = float(np.abs(model - ref).max())
    return c


@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("family", M.FAMILIES)
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_fp32_entry_against_float64(entry, family, T):
    head_dim, run = ENTRIES[entry]
    c = case(family, T, head_dim)
    got = run(c["qkv"].copy(), T).reshape(T, HEADS * head_dim)
    assert np.isfinite(got).all()
    e_kernel = float(np.abs(got - c["ref"]).max())
    bar_a = 4 * c["e_seq"] + 2.0 ** -23 * c["top"]
    line = f"{entry} {family} T {T}: e_kernel {e_kernel:.3e}  e_seq {c['e_seq']:.3e}  bar (a) {bar_a:.3e}  |ref|max {c['top']:.3g}"
    bar_b = None
    if entry == "split":
        bar_b = 2 * c["e_model"] + 2.0 ** -24 * c["top"]
        line += f"  e_model {c['e_model']:.3e}  bar (b) {bar_b:.3e}"
    print(line)
    assert e_kernel <= bar_a, (entry, family, T, e_kernel, bar_a)
    if bar_b is not None and family in M.SPLIT_BAR_FAMILIES:
        assert e_kernel <= bar_b, (entry, family, T, e_kernel, bar_b)
    if family == "one-hot":  # (c)
        for h in range(HEADS):
            q, k, v = M.head_operands(c["qkv"], HEADS, head_dim, h)
            perm = c["info"]["perm"][h]
            assert M.one_hot_gap(q, k, perm, head_dim) >= 200.0
            off = M.ulps(got[:, h * head_dim:(h + 1) * head_dim], v[perm])
            print(f"    head {h}: {off:.2f} ulp from the selected V row")
            assert off <= 4.0, (entry, T, h, off)
    if family == "constant-V":  # (d)
        off = float(np.abs(got.astype(np.float64) - c["info"]["c"].astype(np.float64)[None, :]).max())
        print(f"    {off:.3e} from the constant row")
        assert off <= bar_a, (entry, T, off, bar_a)


@pytest.mark.parametrize("exponent", [40, -40])
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_v_times_a_power_of_two_scales_the_output_exactly(entry, exponent):
    """(e): V enters the output linearly and 2^+-40 times the iid inputs is far from overflow and from the subnormals, in every bf16
    piece as well: no rounding changes."""
    T = 70
    head_dim, run = ENTRIES[entry]
    qkv = case("iid", T, head_dim)["qkv"].copy()
    plain = run(qkv, T)
    qkv[:, 2 * HEADS * head_dim:] *= np.float32(2.0 ** exponent)
    scaled = run(qkv, T)
    assert np.isfinite(scaled).all() and np.abs(plain).max() > 0.1
    assert np.array_equal(scaled.view(np.uint32), (plain * np.float32(2.0 ** exponent)).view(np.uint32))


def bf16_inputs(family, T, head_dim, q_scaled):
    """(the bits a bf16 entry reads, their values [T][3D]): the family's fp32 inputs rounded to bf16; q_scaled: the Q columns hold
    qscale(head_dim) * q, rounded, and the exponent is their plain product with K."""
    D = HEADS * head_dim
    vals = case(family, T, head_dim)["qkv"].copy()
    if q_scaled:
        vals[:, :D] *= M.scale_f32(head_dim)
    bits = B.to_bf16_bits(vals)
    return bits, B.from_bf16_bits(bits)


@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("entry", list(BF16_ENTRIES))
def test_bf16_one_hot_rows_are_the_bits_of_the_selected_value_row(entry, T):
    """(c) on the bf16 entries: Q, K and V rounded to bf16, the gap of 200 in the exponent checked on the rounded values."""
    head_dim, q_scaled, run = BF16_ENTRIES[entry]
    D = HEADS * head_dim
    bits, vals = bf16_inputs("one-hot", T, head_dim, q_scaled)
    perms = case("one-hot", T, head_dim)["info"]["perm"]
    got = run(bits, T).reshape(T, D)
    for h in range(HEADS):
        q, k, _ = M.head_operands(vals, HEADS, head_dim, h)
        s = q.astype(np.float64) @ k.astype(np.float64).T * (1.0 if q_scaled else float(M.scale_f32(head_dim)))
        rows = np.arange(T)
        top = s[rows, perms[h]].copy()
        s[rows, perms[h]] = -np.inf
        assert float((top - s.max(1)).min()) >= 200.0
        want = bits[:, 2 * D + h * head_dim:2 * D + (h + 1) * head_dim][perms[h]]
        wrong = int((got[:, h * head_dim:(h + 1) * head_dim] != want).sum())
        print(f"{entry} one-hot T {T} head {h}: {wrong} elements are not the selected row's bits")
        assert wrong == 0, (entry, T, h, wrong)


@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("entry", list(BF16_ENTRIES))
def test_bf16_rows_of_ones_give_ones(entry, T):
    """(d) on the bf16 entries: every V element 1.0.  The output is sum(the bf16 pieces of p) / sum(p), within 2^-9 of 1, and 1.0 is
    the even neighbour: the bits of 1.0."""
    head_dim, q_scaled, run = BF16_ENTRIES[entry]
    D = HEADS * head_dim
    bits, _ = bf16_inputs("iid", T, head_dim, q_scaled)
    bits = bits.copy()
    bits[:, 2 * D:] = 0x3F80
    got = run(bits, T)
    wrong = int((got != 0x3F80).sum())
    print(f"{entry} V = 1 T {T}: {wrong} elements are not 1.0")
    assert wrong == 0, (entry, T, wrong, np.unique(got))
