"""The framed-buffer helper (tests/strided.py) on host arrays: prove that its checks fire before the GPU tests rely on them.

Host buffers stand in for device buffers: window() and assert_untouched() take the flat array, so the code a GPU test runs on a
downloaded frame is the code tested here.
"""
import numpy as np
import pytest

import strided as S

DTYPES = [np.float32, np.uint16, np.int32]


def _data(rows, width, dtype):
    v = np.arange(rows * width).reshape(rows, width)
    return (v * 0.25 - 3).astype(np.float32) if dtype == np.float32 else v.astype(dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows,width,ld,offset", [(5, 10, 11, 1), (3, 4, 4, 0), (1, 1, 9, 3), (37, 200, 1000, 0)])
def test_clean_frame_passes_and_window_round_trips(dtype, rows, width, ld, offset):
    f = S.Frame(rows, width, ld, dtype, offset=offset)
    data = _data(rows, width, dtype)
    img = f.image(data)
    assert img.size == offset + (rows + 2 * S.GUARD) * ld
    f.assert_untouched(img)
    got = f.window(img)
    assert got.dtype == np.dtype(dtype) and got.shape == (rows, width)
    assert np.array_equal(S.as_bits(got), S.as_bits(data))
    # an output frame: the window holds the sentinel until it is written
    blank = f.image()
    f.assert_untouched(blank)
    assert S.has_sentinel(f.window(blank)) and not S.has_sentinel(got)


def test_guard_cannot_shrink():
    with pytest.raises(AssertionError):
        S.Frame(4, 4, 8, guard=255)
    assert S.GUARD >= 256


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("where", ["pad column", "guard row before", "guard row after", "last element", "in front of the base"])
def test_one_flipped_element_fails_and_is_named(dtype, where):
    rows, width, ld, offset = 6, 10, 13, 2
    f = S.Frame(rows, width, ld, dtype, offset=offset)
    img = f.image(_data(rows, width, dtype))
    g = f.guard
    row, col = {"pad column": (3, 11), "guard row before": (-1, 4), "guard row after": (rows, 0),
                "last element": (rows + g - 1, ld - 1), "in front of the base": (None, 1)}[where]
    flat = col if row is None else offset + (row + g) * ld + col
    if where == "last element":
        assert flat == img.size - 1
    img[flat] ^= 1                                   # one bit of one element
    with pytest.raises(AssertionError) as e:
        f.assert_untouched(img)
    assert f"(row {row}, column {col})" in str(e.value), str(e.value)
    img[flat] ^= 1
    f.assert_untouched(img)


def test_a_write_inside_the_window_is_not_reported():
    f = S.Frame(4, 8, 12)
    img = f.image(np.zeros((4, 8), np.float32))
    for r, c in ((0, 0), (3, 7), (0, 7), (3, 0)):
        img[(f.guard + r) * f.ld + c] = 0x3F800000
    f.assert_untouched(img)
    assert f.window(img)[3, 7] == 1.0


def test_sentinel_nan_is_told_from_a_computed_nan():
    """The fp32 sentinel is a NaN with a payload of its own: 0 / 0 or inf - inf give the default NaN of the arithmetic, and a sum
    that a sentinel entered carries ITS payload on, so a frame element overwritten with a computed NaN is still a change."""
    f = S.Frame(2, 4, 6)
    img = f.image(np.ones((2, 4), np.float32))
    sent = img[:1].view(np.float32)
    assert np.isnan(sent[0]) and int(img[0]) == 0x7FC5A5A5
    with np.errstate(invalid="ignore"):
        computed = (np.float32(np.inf) - np.float32(np.inf)).reshape(1).astype(np.float32)
    assert np.isnan(computed[0]) and int(computed.view(np.uint32)[0]) != 0x7FC5A5A5
    assert not S.has_sentinel(computed) and S.has_nan(computed) and S.has_sentinel(sent)
    pad = (f.guard + 1) * f.ld + 5                  # a pad column of window row 1
    img[pad] = computed.view(np.uint32)[0]
    with pytest.raises(AssertionError) as e:
        f.assert_untouched(img)
    assert "(row 1, column 5)" in str(e.value)
    # bf16: the sentinel is a NaN too, and has_nan() reads bf16 bit patterns
    b = np.array([0x7FC5, 0x3F80, 0x7F80, 0xFFC0], np.uint16)
    assert S.has_sentinel(b) and S.has_nan(b) and not S.has_nan(b[1:3]) and S.has_nan(b[3:])
