"""The contract of the top-k records (vithip_softmax_topk_f32, vit_engine_topk_*) in numpy, for the tests to compare the kernel with.

A row's candidates are its non-NaN scores.  They are ranked by "higher score first; among equal scores (==, so -0.0 ties +0.0) the
lower label first"; slot j takes the j-th of them -- its label and the bits of ITS score -- and slots without a candidate hold the
label EMPTY_LABEL and empty_score (-1.0 for probabilities, -inf for logits).  No sort-stability assumption: every slot is found by
explicit comparisons among the candidates still unranked.
"""
import numpy as np

EMPTY_LABEL = 0x7FFFFFFF
EMPTY_SCORE = {"prob": np.float32(-1.0), "logit": np.float32(-np.inf)}


def topk_records(scores, k, empty_score):
    """scores float32 [rows][classes] -> int32 [rows][2k]: k labels, then the k scores' bit patterns."""
    scores = np.ascontiguousarray(scores, np.float32)
    rows, classes = scores.shape
    assert 1 <= k <= classes
    labels = np.full((rows, k), EMPTY_LABEL, np.int32)
    values = np.full((rows, k), empty_score, np.float32)
    for r in range(rows):
        cand = np.flatnonzero(~np.isnan(scores[r]))  # ascending labels
        for j in range(min(k, cand.size)):
            s = scores[r, cand]
            best = s.max()                        # no NaN among the candidates; -0.0 == +0.0
            first = int(np.flatnonzero(s == best)[0])  # the lowest label among the equal ones
            labels[r, j] = cand[first]
            values[r, j] = s[first]               # that element's own bits
            cand = np.delete(cand, first)
    return np.concatenate([labels, values.view(np.int32)], axis=1)


def split(records):
    """int32 [rows][2k] -> (labels int32 [rows][k], scores float32 [rows][k])"""
    records = np.ascontiguousarray(records, np.int32)
    k = records.shape[1] // 2
    return records[:, :k].copy(), records[:, k:].copy().view(np.float32)
