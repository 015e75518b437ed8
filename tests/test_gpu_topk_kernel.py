"""vithip_softmax_topk_f32 (csrc/vit_topk.hip) on the GPU.

The expectation is never the kernel under test: for PROB it is tests/topk_model.py applied to the probabilities that
vithip_softmax_top1_f32 returns for the same logits, for LOGIT the model applied to the logits.  Everything is compared bit for bit.
"""
import functools

import numpy as np
import pytest

import topk_model as M
from vit_amd import binding as B

pytestmark = pytest.mark.gpu

CLASSES = (1, 2, 5, 63, 64, 65, 255, 256, 257, 1000, 1001, 4099)
ROWS = (1, 3, 7)
FILL = 0xA5A5A5A5
NAN, INF = np.float32(np.nan), np.float32(np.inf)


@functools.lru_cache(maxsize=None)
def seeded(classes, rows):
    """(logits, probabilities, top-1 labels, top-1 probabilities): the last three from vithip_softmax_top1_f32, computed once."""
    rng = np.random.default_rng(classes * 16 + rows)
    logits = (rng.standard_normal((rows, classes)) * 3).astype(np.float32)
    return (logits,) + reference(logits)


def reference(logits):
    probs, label, prob = B.softmax_top1(logits)
    return probs, label, prob


def expect(logits, k, score, probs=None):
    if score == "logit":
        return M.topk_records(logits, k, M.EMPTY_SCORE["logit"])
    return M.topk_records(reference(logits)[0] if probs is None else probs, k, M.EMPTY_SCORE["prob"])


def same(got, want):
    assert got.dtype == want.dtype == np.int32 and got.shape == want.shape
    if not np.array_equal(got, want):
        r, c = np.argwhere(got != want)[0]
        raise AssertionError(f"records differ first at row {r}, word {c}: got {int(got[r, c]):#x}, want {int(want[r, c]):#x}; "
                             f"{int((got != want).sum())} words differ")


def slot0_is_top1(rec, label, prob):
    labels, scores = M.split(rec)
    assert np.array_equal(labels[:, 0], label)
    assert np.array_equal(scores[:, 0].view(np.uint32), prob.view(np.uint32))


@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("classes", CLASSES)
def test_records_equal_the_model_on_the_parent_kernels_probabilities(classes, rows):
    logits, probs, label, prob = seeded(classes, rows)
    for k in sorted({k for k in (1, 2, 5, min(64, classes)) if k <= classes}):
        got = B.softmax_topk(logits, k, "prob")
        same(got, expect(logits, k, "prob", probs))
        slot0_is_top1(got, label, prob)
        same(B.softmax_topk(logits, k, "logit"), expect(logits, k, "logit"))


@pytest.mark.parametrize("classes", (257, 1000))
def test_quantised_logits_tie_inside_a_stride_across_lanes_and_across_waves(classes):
    rng = np.random.default_rng(classes)
    logits = rng.integers(-2, 3, (3, classes)).astype(np.float32)
    probs, label, prob = reference(logits)
    assert all(np.unique(probs[r]).size <= 5 for r in range(3))  # the ties are really there
    for k in (5, 64):
        got = B.softmax_topk(logits, k, "prob")
        same(got, expect(logits, k, "prob", probs))
        slot0_is_top1(got, label, prob)
        same(B.softmax_topk(logits, k, "logit"), expect(logits, k, "logit"))


def test_two_equal_maxima_give_the_lower_label_first():
    classes, c = 1000, 100
    rng = np.random.default_rng(77)
    pairs = [(c, c + 1), (c, c + 64), (c, c + 256), (0, classes - 1)]
    logits = (rng.standard_normal((len(pairs), classes)) * 3).astype(np.float32)
    for r, (a, b) in enumerate(pairs):
        logits[r, [a, b]] = logits[r].max() + np.float32(1.0)
    for score in ("prob", "logit"):
        got = B.softmax_topk(logits, 3, score)
        same(got, expect(logits, 3, score))
        labels, scores = M.split(got)
        assert labels[:, :2].tolist() == [list(p) for p in pairs]
        assert np.array_equal(scores[:, 0].view(np.uint32), scores[:, 1].view(np.uint32))


@pytest.mark.parametrize("classes,k", [(1000, 64), (257, 5), (5, 5)])
def test_an_all_equal_row_gives_labels_in_order(classes, k):
    logits = np.full((2, classes), 0.75, np.float32)
    for score in ("prob", "logit"):
        got = B.softmax_topk(logits, k, score)
        same(got, expect(logits, k, score))
        assert np.array_equal(M.split(got)[0], np.tile(np.arange(k, dtype=np.int32), (2, 1)))


def poison_one_nan(row):
    row[17] = NAN


def poison_all_nan(row):
    row[:] = NAN


def poison_plus_inf(row):
    row[33] = INF


def poison_minus_inf(row):
    row[[0, 5, 63, 64, 65, 69, 30, 31]] = -INF


def poison_few_candidates(row):
    keep = row[[3, 64, 69, 20, 21, 22, 40, 41, 42, 66]].copy()
    row[:] = NAN
    row[[3, 64, 69, 20, 21, 22, 40, 41, 42, 66]] = keep


@pytest.mark.parametrize("poison", [poison_one_nan, poison_all_nan, poison_plus_inf, poison_minus_inf, poison_few_candidates],
                         ids=lambda f: f.__name__)
def test_a_non_finite_row_follows_the_rule_and_leaves_its_neighbours_alone(poison):
    classes, k = 70, 64
    rng = np.random.default_rng(3)
    logits = (rng.standard_normal((3, classes)) * 3).astype(np.float32)
    clean = logits[[0, 2]].copy()
    poison(logits[1])
    probs, label, prob = reference(logits)
    for score in ("prob", "logit"):
        got = B.softmax_topk(logits, k, score)
        same(got, expect(logits, k, score, probs))
        same(got[[0, 2]], B.softmax_topk(clean, k, score))  # rows 0 and 2: the records of a launch without the poisoned row
        labels, scores = M.split(got)
        if score == "prob":
            slot0_is_top1(got, label, prob)
            if poison in (poison_one_nan, poison_all_nan, poison_plus_inf):  # every probability of the row is NaN: all slots empty
                assert (labels[1] == M.EMPTY_LABEL).all() and (scores[1] == -1.0).all()
            if poison is poison_minus_inf:   # exp(-inf) = 0: probability 0.0 is a candidate, ranked last, by label
                assert labels[1, 62:].tolist() == [0, 5] and (scores[1, 62:] == 0.0).all()
        else:
            if poison is poison_one_nan:
                assert 17 not in labels[1] and (labels[1] != M.EMPTY_LABEL).all()
            if poison is poison_plus_inf:
                assert labels[1, 0] == 33 and scores[1, 0] == INF
            if poison is poison_minus_inf:
                assert labels[1, 62:].tolist() == [0, 5] and (scores[1, 62:] == -INF).all()
            if poison is poison_few_candidates:
                assert sorted(labels[1, :10].tolist()) == [3, 20, 21, 22, 40, 41, 42, 64, 66, 69]
                assert (labels[1, 10:] == M.EMPTY_LABEL).all() and (scores[1, 10:] == -INF).all()
            if poison is poison_all_nan:
                assert (labels[1] == M.EMPTY_LABEL).all() and (scores[1] == -INF).all()


@pytest.mark.parametrize("classes,k", [(1000, 5), (257, 64), (4099, 2), (5, 1)])
def test_only_the_records_are_written_and_the_logits_only_read(classes, k):
    rows, guard = 3, 64
    logits = seeded(classes, rows)[0]
    for score in ("prob", "logit"):
        seen = {}
        got = B.softmax_topk(logits, k, score, ld_logits=classes + 3, ld_out=2 * k + 5, guard=guard, fill_bits=FILL, out_offset=1, out=seen)
        same(got, expect(logits, k, score))
        ld = 2 * k + 5
        raw = seen["raw"]
        assert raw.size == 2 * guard + 1 + rows * ld
        assert (raw[:guard + 1] == FILL).all() and (raw[guard + 1 + rows * ld:] == FILL).all()
        body = raw[guard + 1:guard + 1 + rows * ld].reshape(rows, ld)
        assert (body[:, 2 * k:] == FILL).all()
        assert np.array_equal(body[:, :2 * k].view(np.int32), got)
        assert np.array_equal(seen["logits_raw"], seen["logits_raw_before"])


def test_refusals_return_invalid_value_and_a_valid_launch_follows():
    logits = seeded(65, 3)[0]
    for bad in (dict(k=0), dict(k=-1), dict(k=66), dict(k=5, ld_logits=64), dict(k=5, ld_out=9), dict(k=5, score=2), dict(k=5, score=-1)):
        with pytest.raises(B.VitError) as err:
            B.softmax_topk(logits, **bad)
        assert err.value.code == 1, bad
    big = np.zeros((1, 100), np.float32)
    with pytest.raises(B.VitError) as err:
        B.softmax_topk(big, 65)
    assert err.value.code == 1
    same(B.softmax_topk(logits, 5), expect(logits, 5, "prob"))
