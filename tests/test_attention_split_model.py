"""The arithmetic of the split attention kernel (tests/attention_split_model.py) against a float64 attention: it holds the bars
the fp32 kernels are tested with (tests/test_gpu_ops.py::test_attention, ::test_attention_peaked_rows), and it is no less accurate
than a sequential fp32 evaluation of the same inputs.  No GPU.

Recorded (max |model - f64|, max |sequential fp32 - f64|, ratio), one head of 64 columns, uniform inputs, seed = key count:
    +-1.5,   5 keys: 1.19e-07  2.98e-07  0.40
    +-1.5,  16 keys: 1.12e-07  1.57e-07  0.71
    +-1.5,  33 keys: 1.81e-07  1.89e-07  0.96
    +-1.5, 197 keys: 1.38e-07  1.72e-07  0.81
    +-8,   197 keys: 4.98e-05  6.34e-05  0.78    (|ref| max 8.0: 6.2e-06 of it)
    keys 100.. of 130 times 6 (the rescale branch): 4.19e-07, 6.2e-07 of |ref| max
(with the two roundings per matrix instruction that the kernel's bits showed; with one they were 1.1e-7 to 1.4e-7 and 3.15e-05)

Below that: the input families of tests/test_gpu_attention_accuracy.py, where the GPU bars are derived from this model and from the
sequential evaluation -- what both deliver per family, that a split without its small products is outside the split's bar, and the
exactness cases (one-hot rows, V times a power of two).
"""
import functools

import numpy as np
import pytest

import attention_split_model as M
from attention_split_model import attention_f32_sequential, attention_f64, attention_split, bf16_rne, split3

CASES = [(1.5, 5), (1.5, 16), (1.5, 33), (1.5, 197), (8.0, 197)]


def operands(amp, T):
    rng = np.random.default_rng(T)
    return tuple(rng.uniform(-amp, amp, (T, 64)).astype(np.float32) for _ in range(3))


def test_the_pieces_are_bf16_values_that_add_up():
    x = np.random.default_rng(0).uniform(-8, 8, 4096).astype(np.float32)
    hi, mid, lo = split3(x)
    for piece in (hi, mid, lo):
        assert not (piece.view(np.uint32) & 0xFFFF).any()
    assert np.array_equal(hi.astype(np.float64) + mid + lo, x.astype(np.float64))
    # torch's conversion is round to nearest even: a tie goes to the even bf16
    ties = np.array([1.00390625, 1.01171875], np.float32)  # 1 + 2^-8 (down to 1), 1 + 3 * 2^-8 (up to 1 + 2^-6)
    assert np.array_equal(bf16_rne(ties), np.array([1.0, 1.015625], np.float32))


def test_softmax_weights_split_exactly_up_to_the_deferred_maximum():
    """0 <= p <= 2^8: three pieces of 8 bits hold all 24 bits of p."""
    p = np.exp2(np.random.default_rng(1).uniform(-40, 8, 20000)).astype(np.float32)
    hi, mid, lo = split3(p)
    assert np.array_equal(hi.astype(np.float64) + mid + lo, p.astype(np.float64))


@pytest.mark.parametrize("amp,T", CASES)
def test_model_holds_the_bars_and_is_no_worse_than_sequential_fp32(amp, T):
    q, k, v = operands(amp, T)
    ref = attention_f64(q, k, v)
    top = float(np.abs(ref).max())
    e_model = float(np.abs(attention_split(q, k, v) - ref).max())
    e_seq = float(np.abs(attention_f32_sequential(q, k, v) - ref).max())
    print(f"+-{amp}, {T} keys: model {e_model:.3e}  sequential fp32 {e_seq:.3e}  ratio {e_model / e_seq:.2f}  |ref| max {top:.3g}")
    if amp == 8.0:
        assert e_model <= 2e-4 * top          # test_attention_peaked_rows
    else:
        assert e_model <= 1e-5 * max(1.0, top)  # test_attention
    assert e_model <= 4 * e_seq + 1e-7


def test_the_rescale_branch_is_exercised_and_exact_enough():
    """Keys 100.. six times larger: the running maximum moves after the first tiles (tests/test_gpu_ops.py::
    test_attention_chunked_running_max_moves, bar 2e-5 |ref| max)."""
    rng = np.random.default_rng(7)
    q, k, v = (rng.uniform(-1, 1, (130, 64)).astype(np.float32) for _ in range(3))
    k[100:] *= 6.0
    ref = attention_f64(q, k, v)
    err = float(np.abs(attention_split(q, k, v) - ref).max())
    print(f"rescale: {err:.3e} (bar {2e-5 * float(np.abs(ref).max()):.3e})")
    assert err <= 2e-5 * float(np.abs(ref).max())


def test_head_dim_64_keeps_the_bits_of_the_64_only_helpers():
    """attention_f64 and attention_f32_sequential take a head_dim now; at 64 they are the expressions they were (restated here: the
    scores / 8.0, the constant 0.125 * log2(e), 64 FMA steps)."""
    assert M.scale_f32(64) == M.SCALE and M.scale_f32(64).dtype == np.float32
    for amp, T in ((1.5, 33), (8.0, 197)):
        q, k, v = operands(amp, T)
        q64, k64, v64 = (a.astype(np.float64) for a in (q, k, v))
        s = q64 @ k64.T / 8.0
        p = np.exp(s - s.max(1, keepdims=True))
        assert np.array_equal(attention_f64(q, k, v), (p / p.sum(1, keepdims=True)) @ v64)
        assert np.array_equal(attention_f64(q, k, v, 64), attention_f64(q, k, v))
        s = np.zeros((T, T), np.float32)
        for d in range(64):
            s = M.f32(s.astype(np.float64) + np.outer(q64[:, d], k64[:, d]))
        mneg = M.f32(-s.max(1).astype(np.float64) * M.SCALE)
        p = M.f32(np.exp2(M.f32(s.astype(np.float64) * M.SCALE + mneg[:, None].astype(np.float64)).astype(np.float64)))
        total, o = np.zeros(T, np.float32), np.zeros((T, 64), np.float32)
        for key in range(T):
            total = total + p[:, key]
            o = M.f32(o.astype(np.float64) + np.outer(p[:, key].astype(np.float64), v64[key]))
        want = o * (np.float32(1.0) / total)[:, None]
        assert np.array_equal(attention_f32_sequential(q, k, v).view(np.uint32), want.view(np.uint32))
        assert np.array_equal(attention_f32_sequential(q, k, v, 64).view(np.uint32), want.view(np.uint32))


# ---- the input families of tests/test_gpu_attention_accuracy.py: what the model and the sequential evaluation deliver on them ---------

HEADS = 2
MUTANT = ((0, 1), (1, 0), (0, 0))  # the three largest piece products alone: a wrong piece index, a lost accumulate


@functools.lru_cache(maxsize=None)
def family_case(family, T):
    """(qkv, info, float64 reference [T][128], model, mutant, sequential fp32), two heads of 64, the draw the GPU tests use."""
    qkv, info = M.family_inputs(family, T, 64, HEADS, M.ACCURACY_SEED)
    heads = [M.head_operands(qkv, HEADS, 64, h) for h in range(HEADS)]
    return (qkv, info) + tuple(np.concatenate([fn(*qkv_h) for qkv_h in heads], axis=1) for fn in (
        attention_f64, attention_split, lambda q, k, v: attention_split(q, k, v, MUTANT), attention_f32_sequential))


def worst(a, ref):
    return float(np.abs(a.astype(np.float64) - ref).max())


@pytest.mark.parametrize("T", [33, 197])
@pytest.mark.parametrize("family", M.FAMILIES)
def test_family_model_is_within_four_sequential_errors_and_the_mutant_is_not_within_two_model_errors(family, T):
    """Bar (a) of the GPU tests on the model itself, 4 e_seq + 2^-23 |ref|max (one rounding of the output, one of the reciprocal),
    and the reason for bar (b), 2 e_model + 2^-24 |ref|max: a split that lost its three small products is outside it in every
    family at these key counts, so (b) is asserted on all of them.  It is close with an offset V and a flat softmax: 1.08 times the
    bar at 197 keys, and at 257 keys, which the GPU tests run as well, the mutant is inside (5.6e-6, bar 5.9e-6): there (b) still
    holds the kernel to twice its model but would not catch this fault; the other six families do, 2 to 33 times over.
    Recorded, 33 / 197 keys (e_seq, e_model, e_mutant):
        iid         2.1e-7 1.6e-7 4.1e-6 / 2.6e-7 1.5e-7 2.3e-6      peaked      6.3e-5 2.6e-5 6.2e-4 / 6.4e-5 8.9e-5 1.0e-3
        offset      1.3e-6 1.1e-6 8.5e-6 / 3.8e-6 2.3e-6 5.2e-6      one-hot     2.4e-7 2.4e-7 1.6e-5 / 2.4e-7 2.4e-7 1.6e-5
        retrieval   1.6e-6 1.4e-6 3.6e-5 / 3.6e-6 2.4e-6 1.6e-5      constant-V  1.7e-6 1.2e-6 2.1e-5 / 4.1e-6 2.6e-6 1.9e-5
        rising      7.2e-7 6.4e-7 4.9e-5 / 6.9e-6 3.4e-6 4.3e-5"""
    _, _, ref, model, mutant, seq = family_case(family, T)
    top = float(np.abs(ref).max())
    e_model, e_mutant, e_seq = worst(model, ref), worst(mutant, ref), worst(seq, ref)
    bar_a, bar_b = 4 * e_seq + 2.0 ** -23 * top, 2 * e_model + 2.0 ** -24 * top
    print(f"{family}, {T} keys: sequential fp32 {e_seq:.3e}  model {e_model:.3e} (bar {bar_a:.3e})  mutant {e_mutant:.3e} (split bar {bar_b:.3e})"
          f"  |ref| max {top:.3g}")
    assert e_model <= bar_a
    assert family in M.SPLIT_BAR_FAMILIES
    assert e_mutant > bar_b


@pytest.mark.parametrize("T", [33, 197])
def test_one_hot_rows_return_the_selected_value_row(T):
    """q_i = 200 k_perm(i): every other key is at least 200 below in the exponent (float64), so every fp32 evaluation has p = 0 for
    it and the output is v_perm(i) -- within 1 ulp, not bit for bit: fma(s, c, -m c) keeps the rounding of m c in the exponent, so p
    and the row sum are 2^tiny, not 1."""
    qkv, info, _, model, _, seq = family_case("one-hot", T)
    for h in range(HEADS):
        q, k, v = M.head_operands(qkv, HEADS, 64, h)
        gap = M.one_hot_gap(q, k, info["perm"][h], 64)
        want = v[info["perm"][h]]
        cols = slice(64 * h, 64 * h + 64)
        print(f"one-hot, {T} keys, head {h}: gap {gap:.0f}, model {M.ulps(model[:, cols], want):.2f} ulp, sequential {M.ulps(seq[:, cols], want):.2f} ulp")
        assert gap >= 200.0
        assert M.ulps(model[:, cols], want) <= 1.0
        assert M.ulps(seq[:, cols], want) <= 1.0


@pytest.mark.parametrize("T", [33, 197, 257])
@pytest.mark.parametrize("head_dim", [64, 72, 128])
def test_rising_scores_move_the_deferred_maximum_and_stay_under_it(head_dim, T):
    """The 32-key tile walk of attention_hd_kernel and attention_split_kernel on the rising family: in some row the exponent outgrows
    the running maximum by more than kDefer = 8 in at least two tiles behind the first (O and the row sum are rescaled twice; at 33
    keys there is one tile behind the first, and it moves), and in some row a tile's maximum is above the running one by no more than
    8, so the maximum stays and p passes 1."""
    qkv, _ = M.family_inputs("rising", T, head_dim, HEADS, M.ACCURACY_SEED)
    for h in range(HEADS):
        q, k, _ = M.head_operands(qkv, HEADS, head_dim, h)
        s = M.scaled_scores_f64(q, k, head_dim)
        assert (s.argmax(1) >= T - 4).all() and (s[:, -1] - s[:, 0]).min() > 8.0  # every row rises to its end
        moves, held = M.deferred_maximum_walk(s)
        print(f"rising head_dim {head_dim} {T} keys head {h}: at most {moves.max()} moves and {held.max()} tiles held in a row")
        assert moves.max() >= min(2, (T - 1) // 32)
        assert held.max() >= 1


def test_v_times_a_power_of_two_scales_the_models_output_exactly():
    qkv, _, _, model, _, _ = family_case("iid", 33)
    for e in (40, -40):
        for h in range(HEADS):
            q, k, v = M.head_operands(qkv, HEADS, 64, h)
            got = attention_split(q, k, v * np.float32(2.0 ** e))
            assert np.array_equal(got.view(np.uint32), (model[:, 64 * h:64 * h + 64] * np.float32(2.0 ** e)).view(np.uint32)), (e, h)


def test_a_row_does_not_depend_on_the_other_query_rows():
    q, k, v = operands(1.5, 70)
    full = attention_split(q, k, v)
    assert np.array_equal(attention_split(q[:1], k, v), full[:1])
    assert np.array_equal(attention_split(q[40:41], k, v), full[40:41])
