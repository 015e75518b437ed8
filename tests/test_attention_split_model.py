"""The arithmetic of the split attention kernel (tests/attention_split_model.py) against a float64 attention: it holds the bars
the fp32 kernels are tested with (tests/test_gpu_ops.py::test_attention, ::test_attention_peaked_rows), and it is no less accurate
than a sequential fp32 evaluation of the same inputs.  No GPU.

Recorded (max |model - f64|, max |sequential fp32 - f64|, ratio), one head of 64 columns, uniform inputs, seed = key count:
    +-1.5,   5 keys: 1.41e-07  2.98e-07  0.47
    +-1.5,  16 keys: 1.44e-07  1.57e-07  0.91
    +-1.5,  33 keys: 1.14e-07  1.89e-07  0.60
    +-1.5, 197 keys: 1.16e-07  1.72e-07  0.68
    +-8,   197 keys: 3.15e-05  6.34e-05  0.50    (|ref| max 8.0: 3.9e-06 of it)
    keys 100.. of 130 times 6 (the rescale branch): 2.99e-07, 4.4e-07 of |ref| max
"""
import numpy as np
import pytest

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


def test_a_row_does_not_depend_on_the_other_query_rows():
    q, k, v = operands(1.5, 70)
    full = attention_split(q, k, v)
    assert np.array_equal(attention_split(q[:1], k, v), full[:1])
    assert np.array_equal(attention_split(q[40:41], k, v), full[40:41])
