"""vithip_dense_upsample_argmax_f32 and vithip_dense_grid_f32 (csrc/vit_dense.hip) on the GPU.

The expectation is tests/dense_head_model.py, the numpy statement of the arithmetic (pinned to PyTorch in
tests/test_dense_head_model.py): labels are compared one for one, no tolerance.  The sizes are the six of the model's test plus the
edges of the kernel: 1 and 255 classes, a single cell, a single pixel, a window that is walked in slices of classes (37 -> 37 with 255
classes) and one that makes the tile shrink (64 -> 16).
"""
import functools

import numpy as np
import pytest

import dense_head_model as M
import strided
from vit_amd import binding as B

pytestmark = pytest.mark.gpu

# g, out_h, out_w, classes
SIZES = [(4, 64, 64, 21), (4, 37, 53, 21), (16, 224, 224, 150), (37, 74, 70, 19), (5, 5, 5, 3), (8, 3, 2, 3),
         (4, 64, 64, 1), (4, 33, 65, 255), (1, 9, 5, 7), (6, 1, 1, 5), (37, 37, 37, 255), (64, 16, 16, 21), (3, 300, 2, 4)]
NAN, INF = np.float32(np.nan), np.float32(np.inf)
SENTINEL_BYTES = np.array([strided.SENTINEL[np.dtype(np.int32)]], np.uint32).view(np.uint8)


@functools.lru_cache(maxsize=None)
def case(g, out_h, out_w, classes, n=2):
    """(logits [n][g * g][classes], the model's labels), computed once."""
    rng = np.random.default_rng(g * 1000 + out_h * 7 + out_w + classes)
    logits = rng.standard_normal((n, g * g, classes)).astype(np.float32)
    want = M.labels_batch(logits, g, out_h, out_w)
    logits.setflags(write=False); want.setflags(write=False)
    return logits, want


def same(got, want):
    assert got.dtype == want.dtype == np.uint8 and got.shape == want.shape
    if not np.array_equal(got, want):
        i, y, x = np.argwhere(got != want)[0]
        raise AssertionError(f"labels differ first at image {i}, pixel ({y}, {x}): got {int(got[i, y, x])}, want {int(want[i, y, x])}; "
                             f"{int((got != want).sum())} of {got.size} differ")


@pytest.mark.parametrize("g,out_h,out_w,classes", SIZES)
def test_labels_equal_the_model(g, out_h, out_w, classes):
    logits, want = case(g, out_h, out_w, classes)
    same(B.dense_upsample_argmax(logits, out_h, out_w), want)


@pytest.mark.parametrize("g,out_h,out_w,classes", [(4, 37, 53, 21), (37, 74, 70, 19), (8, 3, 2, 3), (37, 37, 37, 255)])
def test_padded_rows_and_strides_and_nothing_outside_the_labels_is_written(g, out_h, out_w, classes):
    logits, want = case(g, out_h, out_w, classes, 3)
    words = (out_h * out_w + 3) // 4
    frames = {}
    got = B.dense_upsample_argmax(logits, out_h, out_w, ld_logits=classes + 3, image_rows=g * g + 2, out_ld_words=words + 5,
                                  pad_value=1e30, frames=strided, out=frames)
    same(got, want)
    frames["labels"].assert_untouched()
    frames["logits"].assert_untouched()
    tail = np.ascontiguousarray(frames["labels"].window()).view(np.uint8)[:, out_h * out_w:]   # the last word's bytes behind the labels
    used = out_h * out_w % 4
    assert tail.shape == (3, 4 - used if used else 0)
    if used:
        assert np.array_equal(tail, np.tile(SENTINEL_BYTES[used:], (3, 1)))
    src = np.concatenate([logits, np.full((3, 2, classes), 1e30, np.float32)], axis=1).reshape(-1, classes)
    assert np.array_equal(strided.as_bits(frames["logits"].window()), strided.as_bits(src))  # the logits are only read


def test_ties_nan_and_inf_follow_the_order():
    g, classes = 4, 6
    rng = np.random.default_rng(5)
    logits = rng.standard_normal((5, g * g, classes)).astype(np.float32)
    logits[0, :, 1] = logits[0, :, 4] = 9.0          # equal classes: the lower label
    logits[1, :, 3] = NAN                             # a NaN class is skipped
    logits[2] = NAN                                   # no candidate anywhere: 255
    logits[3, :, 2] = INF                             # +Inf wins wherever its weight is not zero
    logits[4, 5, :] = -INF                            # one cell of -Inf: an ordinary value
    want = M.labels_batch(logits, g, 16, 12)
    assert (want[0] == 1).all() and (want[1] != 3).all() and (want[2] == 255).all() and (want[3] == 2).sum() > 0
    same(B.dense_upsample_argmax(logits, 16, 12), want)
    # at the identity size the weights are exactly 1 and 0, and 0 * Inf is NaN: the model says which pixels lose the class
    want = M.labels_batch(logits, g, g, g)
    same(B.dense_upsample_argmax(logits, g, g), want)


def test_a_non_finite_image_changes_only_its_own_labels():
    g, out_h, out_w, classes = 16, 224, 224, 150
    logits, want = case(g, out_h, out_w, classes)
    three = np.stack([logits[0], np.full_like(logits[0], NAN), logits[1]])
    three[1, ::3] = INF
    got = B.dense_upsample_argmax(three, out_h, out_w)
    same(got[[0, 2]], want)
    same(got[1:2], M.labels_batch(three[1:2], g, out_h, out_w))


def test_grid_is_the_transpose_bit_for_bit():
    for g, classes in ((4, 21), (37, 19), (16, 150), (1, 1), (5, 255), (7, 33)):
        rng = np.random.default_rng(g + classes)
        logits = rng.standard_normal((3, g * g, classes)).astype(np.float32)
        logits[1, 0, 0] = NAN
        got = B.dense_grid(logits)
        assert got.shape == (3, classes, g, g)
        want = np.ascontiguousarray(logits.transpose(0, 2, 1)).reshape(3, classes, g, g)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        for i in range(3):
            assert np.array_equal(M.grid_to_logits(got[i]).view(np.uint32), logits[i].view(np.uint32))


def test_refusals_leave_the_output_untouched():
    g, out_h, out_w, classes, n = 4, 37, 53, 21, 2
    logits, _ = case(g, out_h, out_w, classes)
    words = (out_h * out_w + 3) // 4
    dL = strided.framed(logits.reshape(n * g * g, classes))
    dO = strided.out_frame(n, words, dtype=np.int32)
    ok = dict(logits_ptr=dL.ptr, ld_logits=classes, image_stride=g * g * classes, out_ptr=dO.ptr, out_image_stride=4 * words, images=n, g=g,
              classes=classes, out_h=out_h, out_w=out_w)
    for bad in (dict(logits_ptr=None), dict(out_ptr=None), dict(images=0), dict(g=0), dict(classes=0), dict(classes=256), dict(out_h=0),
                dict(out_w=4097), dict(ld_logits=classes - 1), dict(image_stride=g * g * classes - 1), dict(out_image_stride=out_h * out_w - 1)):
        assert B.dense_upsample_argmax_raw(**{**ok, **bad}) == 1, bad
    arr = dO.download()
    dO.assert_untouched(arr)
    assert (strided.as_bits(dO.window(arr)) == strided.SENTINEL[np.dtype(np.int32)]).all()
    assert B.dense_upsample_argmax_raw(**ok) == 0      # and the same buffers are fine as they are
    got = np.ascontiguousarray(dO.window()).view(np.uint8)[:, :out_h * out_w].reshape(n, out_h, out_w)
    same(got.copy(), case(g, out_h, out_w, classes)[1])
