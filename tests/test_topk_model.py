"""tests/topk_model.py, the reference of the top-k GPU tests, against a brute-force Python loop that states the contract once more:
candidates = the non-NaN entries; (score descending, label ascending) by pairwise comparison; leftover slots empty.  No GPU."""
import numpy as np
import pytest

import topk_model as M


def brute_force(scores, k, empty_score):
    scores = np.asarray(scores, np.float32)
    rows, classes = scores.shape
    out = np.empty((rows, 2 * k), np.int32)
    for r in range(rows):
        taken, labels, values = set(), [], []
        for _ in range(k):
            best = None
            for c in range(classes):
                s = scores[r, c]
                if c in taken or s != s:
                    continue
                if best is None or s > scores[r, best]:   # equal scores: the earlier (lower) label stays
                    best = c
            if best is None:
                labels.append(M.EMPTY_LABEL)
                values.append(np.float32(empty_score))
            else:
                taken.add(best)
                labels.append(best)
                values.append(scores[r, best])
        out[r, :k] = labels
        out[r, k:] = np.array(values, np.float32).view(np.int32)
    return out


def check(scores, k):
    for empty in M.EMPTY_SCORE.values():
        got, want = M.topk_records(scores, k, empty), brute_force(scores, k, empty)
        assert got.dtype == np.int32 and got.shape == (len(scores), 2 * k)
        assert np.array_equal(got, want)
    return got


@pytest.mark.parametrize("classes,k", [(1, 1), (2, 2), (7, 3), (64, 5), (100, 64), (257, 1)])
def test_random_rows(classes, k):
    rng = np.random.default_rng(classes * 100 + k)
    check((rng.standard_normal((4, classes)) * 3).astype(np.float32), k)


def test_rows_quantised_to_three_values_rank_equal_scores_by_label():
    rng = np.random.default_rng(5)
    scores = rng.integers(-1, 2, (5, 40)).astype(np.float32)
    got = check(scores, 12)
    labels, values = M.split(got)
    for r in range(5):
        for j in range(1, 12):
            assert values[r, j - 1] > values[r, j] or (values[r, j - 1] == values[r, j] and labels[r, j - 1] < labels[r, j])


def test_an_all_equal_row_gives_the_labels_in_order():
    labels, values = M.split(check(np.full((2, 9), 0.25, np.float32), 9))
    assert np.array_equal(labels, np.tile(np.arange(9, dtype=np.int32), (2, 1))) and (values == 0.25).all()


def test_negative_zero_ties_positive_zero_and_keeps_its_own_bits():
    scores = np.array([[-1.0, 0.0, -0.0, 0.0, -0.0, -2.0]], np.float32)
    labels, values = M.split(check(scores, 5))
    assert labels[0].tolist() == [1, 2, 3, 4, 0]
    assert values[0].view(np.uint32).tolist() == [0, 0x80000000, 0, 0x80000000, 0xBF800000]


def test_nan_entries_are_no_candidates_and_leave_empty_slots():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    scores = np.array([[nan, 1.0, nan, -inf, inf, nan], [nan] * 6, [3.0, 2.0, 1.0, 0.0, -1.0, -2.0]], np.float32)
    for name, empty in M.EMPTY_SCORE.items():
        labels, values = M.split(M.topk_records(scores, 5, empty))
        assert labels[0].tolist() == [4, 1, 3, M.EMPTY_LABEL, M.EMPTY_LABEL]
        assert values[0, :3].tolist() == [inf, 1.0, -inf] and (values[0, 3:] == empty).all()
        assert (labels[1] == M.EMPTY_LABEL).all() and (values[1] == empty).all()
        assert labels[2].tolist() == [0, 1, 2, 3, 4]
    check(scores, 5)
    check(scores, 6)


def test_k_equal_to_classes_and_a_single_class():
    rng = np.random.default_rng(9)
    scores = rng.standard_normal((3, 17)).astype(np.float32)
    labels, _ = M.split(check(scores, 17))
    assert all(sorted(labels[r].tolist()) == list(range(17)) for r in range(3))
    got = check(np.array([[0.5], [np.nan]], np.float32), 1)
    assert got[0].tolist() == [0, int(np.float32(0.5).view(np.int32))] and got[1, 0] == M.EMPTY_LABEL
