"""The bars of tests/test_gpu_attention_bf16_accuracy.py tell a wrong bf16 attention kernel from a right one: on the CPU, with
attention_bf16_model's model standing in for the kernels.  No GPU.

  * the model, and the model with another accumulation grain and v_exp_f32 one ulp off either way, hold (a) - (d) against float64 in
    every family, for every kernel's arithmetic, plain and q_scaled;
  * the integer families satisfy their bit-width, gap and left-out conditions at every shape the GPU test uses;
  * three fp32 summation orders -- 32-key tiles forwards and 64-key tiles backwards with the 2^8 deferral, one global maximum -- give
    the bits tier I expects;
  * the mutants (MUTANTS) each miss a named new bar in a named family; whether 2^-8 |ref| + 1e-3, the bar of tests/test_gpu_bf16.py,
    holds them there is asserted either way.
"""
import functools

import numpy as np
import pytest

import attention_bf16_model as A
import attention_split_model as M
from vit_amd import binding as B

HEADS = 2
SHAPE = {"resident": (197, 64), "stream": (257, 64), "chunked": (257, 64), "hd": (257, 72)}  # 257: a ragged last tile of one key


@functools.lru_cache(maxsize=None)
def case(family, kernel, q_scaled):
    T, head_dim = SHAPE[kernel]
    vals, info = M.family_inputs(family, T, head_dim, HEADS, M.ACCURACY_SEED)
    vals = vals.copy()
    if q_scaled:
        vals[:, :HEADS * head_dim] *= M.scale_f32(head_dim)
    vals = B.from_bf16_bits(B.to_bf16_bits(vals)).reshape(vals.shape)
    heads = [M.head_operands(vals, HEADS, head_dim, h) for h in range(HEADS)]
    refs = [A.reference(q, k, v, head_dim, q_scaled) for q, k, v in heads]
    ref, Aa = (np.concatenate([r[j] for r in refs], axis=1) for j in range(2))
    seq = np.concatenate([M.attention_f32_sequential(q, k, v, head_dim, q_scaled) for q, k, v in heads], axis=1)
    e_seq = float(np.abs(seq - ref).max())

    def run(**kw):
        out = [A.kernel_model(kernel, q, k, v, head_dim, q_scaled, **kw) for q, k, v in heads]
        return tuple(np.concatenate([o[j] for o in out], axis=1) for j in range(2))

    pre, bits = run()
    return dict(vals=vals, ref=ref, A=Aa, e_seq=e_seq, run=run, bits=bits, bars=A.tier2_bars(ref, Aa, e_seq, pre, bits),
                row=A.bits16(vals[0, 2 * HEADS * head_dim:]))


@pytest.mark.parametrize("q_scaled", [False, True], ids=["plain", "q_scaled"])
@pytest.mark.parametrize("kernel", list(A.KERNELS))
@pytest.mark.parametrize("family", M.FAMILIES)
def test_the_model_holds_the_bars(family, kernel, q_scaled):
    c = case(family, kernel, q_scaled)
    for name, kw in (("model", {}), ("8 keys per rounding, exp + 1 ulp", dict(group=8, exp_ulps=1)),
                     ("32 keys per rounding, exp - 1 ulp", dict(group=32, exp_ulps=-1))):
        bits = c["bits"] if not kw else c["run"](**kw)[1]
        r = A.tier2_check(bits, c["ref"], c["A"], c["bars"])
        assert r["missed"] == [], (family, kernel, name, r)
        if family == "constant-V":  # (d): 0 elements off, for both kinds of row sum
            assert (bits == c["row"][None, :]).all(), (kernel, name)
        if family in ("one-hot", "constant-V"):  # the allowance of (b) is 0: any output off is a miss
            assert c["bars"]["model_share"] == 0.0 and c["bars"]["cap"] == 0.0
    if family in ("offset", "retrieval", "constant-V") or (family == "rising" and kernel == "resident"):
        assert abs(c["bars"]["mean"]) <= 3e-5, c["bars"]["mean"]


@pytest.mark.parametrize("head_dim", [64, 72, 128])
@pytest.mark.parametrize("family", A.INTEGER_FAMILIES)
def test_the_integer_families_are_exact_in_fp32(family, head_dim):
    for T in ([33, 197, 224, 225, 257, 704, 705] if head_dim == 64 else [33, 197, 257]):
        qkv = A.integer_inputs(family, T, head_dim, 3, 3)
        assert np.array_equal(B.from_bf16_bits(B.to_bf16_bits(qkv)).reshape(qkv.shape), qkv)
        left = zeros = n = 0
        for i in range(3):
            for h in range(3):
                q, k, v = M.head_operands(qkv[i * T:(i + 1) * T], 3, head_dim, h)
                assert set(np.unique(q)) <= {-1.0, 0.0, 1.0} and np.abs(v).max() == 2.0 and (np.abs(q[:, 0]) == 1.0).all()
                assert np.array_equal(k[:, 0], A.levels(family, T).astype(np.float32))
                bits, loose, gap = A.integer_width(q, k, v)
                # `loose` counts every key at the row's maximum; it is what limits FLAT_RISE at head_dim 64 (23 at 225 keys) and passes
                # 23 beyond (27 at head_dim 128, 257 keys, where the other 127 columns alone spread a row's scores over 16 levels);
                # `bits` is what the exactness needs
                assert bits <= 23 and loose <= 27, (T, bits, loose)
                assert gap >= A.TOP_WINDOW and (family == "flat-rise") == (gap == float("inf"))
                _, compared, zero, p = A.integer_expected(q, k, v)
                assert abs(p.sum(1) - 1.0).max() < 1e-12
                left += int((~compared & ~zero).sum())
                zeros += int(zero.sum())
                n += compared.size
        assert left <= 0.001 * n, (T, left / n)  # the GPU test allows 0.5 %
        assert 0 < zeros <= 0.03 * n, (T, zeros / n)
        if family == "plateau":  # both directions: rows whose levels rise along the keys and rows whose levels fall
            assert {-1.0, 1.0} <= set(qkv[:T, 0])


ORDERS = {"32-key tiles, forwards": dict(tile=32, defer=A.DEFER), "64-key tiles, backwards": dict(tile=64, defer=A.DEFER, backwards=True),
          "one global maximum": dict(tile=None, defer=None)}


@pytest.mark.parametrize("T", [33, 197, 225, 257, 705])
@pytest.mark.parametrize("family", A.INTEGER_FAMILIES)
def test_three_summation_orders_give_the_expected_bits(family, T):
    qkv = A.integer_inputs(family, T, 64, 3, 1)
    q, k, v = M.head_operands(qkv, 3, 64, 1)
    bits, compared, zero, _ = A.integer_expected(q, k, v)
    for name, kw in ORDERS.items():
        got = A.fp32_walk(q, k, v, **kw)
        assert np.array_equal(A.rne_bits(got)[compared], bits[compared]), (family, T, name)
        assert float(np.abs(got[zero]).max(initial=0.0)) <= A.ZERO_SUM_BOUND, (family, T, name)
        if family == "flat-rise":  # nothing below the top plateau: the zero sums are zeros
            assert (got[zero] == 0).all()


@pytest.mark.parametrize("T", [33, 197])
@pytest.mark.parametrize("family", A.INTEGER_FAMILIES)
def test_the_matrix_instruction_keeps_the_bits_and_the_zero_bound(family, T):
    """P.V on the model of v_mfma_f32_32x32x16_bf16 (profiles/r31): the same bits wherever they are compared.  Zero sums: 2^-40 holds
    where the top plateau is walked first, and in flat-rise; where lower keys precede it the instruction's cut of a negative
    accumulator leaves minus one unit of the products' frame, above 2^-40 and within zero_bound -- what the MI355X returns
    (profiles/r34: 4.05e-8 at 33 keys, 1.02e-8 at 197, this model's figures after the store's rounding)."""
    qkv = A.integer_inputs(family, T, 64, 3, 1)
    above = 0
    for h in range(3):
        q, k, v = M.head_operands(qkv, 3, 64, h)
        bits, compared, zero, _ = A.integer_expected(q, k, v)
        got = A.mfma_pv(q, k, v)
        assert np.array_equal(A.rne_bits(got)[compared], bits[compared])
        bound = np.broadcast_to(A.zero_bound(q, k, v)[:, None], got.shape)
        assert (np.abs(A.rne(got))[zero] <= bound[zero]).all()
        first = np.broadcast_to((bound == A.ZERO_SUM_BOUND), got.shape)
        assert family == "plateau" or first.all()
        above += int((np.abs(got)[zero & ~first] > A.ZERO_SUM_BOUND).sum())
    assert (above > 0) == (family == "plateau")


# mutant: (the model's arguments, {family: (new bars it misses there, inside 2^-8 |ref| + 1e-3 there)}), on the stream kernel's
# arithmetic (the fp32 p are summed) at 257 keys.  The two truncations pass the old bar on the inputs the old tests use (iid: outputs
# of 0.1 to 0.7, the bar 1 - 2 % of them) and only (c) sees them there; on outputs of about 3 they are half a bf16 ulp of bias and
# (b) and (c) see them, and so would the old bar -- which no test applied to such outputs.  A dropped key and a skipped rescale are
# outside the old bar wherever they are outside a new one: those two the old tests could see.
MUTANTS = {
    "P truncated to bf16": (dict(p_round=A.trunc), {"iid": ("c", True), "offset": ("bc", False), "constant-V": ("bc", False)}),
    "a truncating store": (dict(store=A.trunc), {"iid": ("c", True), "offset": ("bc", False), "constant-V": ("bc", False)}),
    "the last key of the ragged tile masked": (dict(mask_last=True), {"offset": ("ab", False), "iid": ("ab", False)}),
    "no rescale when the reference moves": (dict(skip_rescale=True), {"rising": ("abc", False), "peaked": ("abc", False)}),
}


@pytest.mark.parametrize("q_scaled", [False, True], ids=["plain", "q_scaled"])
@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutants_miss_a_new_bar(mutant, q_scaled):
    kw, expected = MUTANTS[mutant]
    for family, (missed, inside_old) in expected.items():
        c = case(family, "stream", q_scaled)
        bits = c["run"](**kw)[1]
        r = A.tier2_check(bits, c["ref"], c["A"], c["bars"])
        print(f"{mutant}, {family}: outside (a) {r['outside']}, share {100 * r['share']:.2f} % (cap {100 * c['bars']['cap']:.2f} %), "
              f"mean {r['mean']:+.2e} (model {c['bars']['mean']:+.2e} +- {4 * c['bars']['se']:.1e}), e {r['e_kernel']:.2e}")
        assert set(missed) <= set(r["missed"]), (mutant, family, r)
        assert A.inside_old_bar(bits, c["ref"]) == inside_old, (mutant, family)
        if family == "constant-V":  # (d)
            assert (bits != c["row"][None, :]).mean() > 0.4


@pytest.mark.parametrize("family", ["offset", "rising", "constant-V"])
def test_a_truncated_p_is_no_fault_under_a_rounded_sum(family):
    """The resident kernel sums p as rounded.  A truncated P is then a set of weights normalised by its own sum: twice the spread of
    a rounded one, no bias, and it passes every bar -- which is why the mutant is "in a kernel that sums the unrounded p".  The same P
    under the fp32 sum misses (b) and (c)."""
    c = case(family, "resident", True)
    bits = c["run"](p_round=A.trunc)[1]
    assert A.tier2_check(bits, c["ref"], c["A"], c["bars"])["missed"] == []
    if family == "constant-V":
        assert (bits == c["row"][None, :]).all()
    T, head_dim = SHAPE["resident"]
    heads = [M.head_operands(c["vals"], HEADS, head_dim, h) for h in range(HEADS)]
    bits = np.concatenate([A.attention_bf16(q, k, v, head_dim, True, False, p_round=A.trunc)[1] for q, k, v in heads], axis=1)
    assert {"b", "c"} <= set(A.tier2_check(bits, c["ref"], c["A"], c["bars"])["missed"])
