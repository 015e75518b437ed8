"""vithip_knn_topk_f32 / _bf16bank (csrc/vit_knn.hip) against float64 NumPy and, where every sum is exact, bit for bit against
tests/topk_model.py.

The bar of a score is the bound of an fp32 dot product of D terms in any order, plus the residual of the query's split:
bar[i][g] = (D + 2) * 2^-24 * (|q_i| . |b_g|), b the bank as the kernel reads it (rounded to bf16 for the bf16 bank).
"""
import numpy as np
import pytest

import topk_model as M
from engine_helpers import same_bits
from vit_amd import binding as B

pytestmark = pytest.mark.gpu

DTYPES = ["f32", "bf16"]
EMPTY = M.EMPTY_LABEL


def unit_rows(rows, D, seed):
    x = np.random.default_rng(seed).standard_normal((rows, D))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def as_bank(bank, dtype):
    """(what knn_topk takes, the fp32 values the kernel reads)"""
    if dtype == "f32":
        return bank, bank
    bits = B.to_bf16_bits(bank)
    return bits, B.from_bf16_bits(bits)


def check_against_float64(rec, q, b, k):
    """The rule of the module's head for the first 2k words of every row of rec; b: the bank's values as read."""
    D = q.shape[1]
    q64, b64 = q.astype(np.float64), b.astype(np.float64)
    exact = q64 @ b64.T
    bar = (D + 2) * 2.0 ** -24 * (np.abs(q64) @ np.abs(b64).T)
    idx, sc = B.split_topk(rec[:, :2 * k])
    for i in range(q.shape[0]):
        cand = ~np.isnan(exact[i])
        live = idx[i] != EMPTY
        assert live.sum() == min(k, cand.sum()) and live[:live.sum()].all(), (i, idx[i])
        got = idx[i][live]
        assert len(set(got.tolist())) == got.size and (got >= 0).all() and (got < b.shape[0]).all() and cand[got].all()
        assert (np.abs(sc[i][live].astype(np.float64) - exact[i, got]) <= bar[i, got]).all(), i
        assert (sc[i][1:] <= sc[i][:-1]).all() and (sc[i][~live] == -np.inf).all(), i
        if live.all():
            omitted = cand.copy()
            omitted[got] = False
            assert (exact[i, omitted] <= float(sc[i][-1]) + bar[i, omitted] + bar[i, got[-1]]).all(), i


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [8, 392, 768])
@pytest.mark.parametrize("G", [1, 31, 129, 1000, 4099])
def test_against_float64(G, D, dtype):
    q33, bank = unit_rows(33, D, 11 + D), unit_rows(G, D, 13 * G + D)
    arg, read = as_bank(bank, dtype)
    for n in (1, 33):
        for k in (1, 10, min(G, 256)):
            for slices in (0, 1, 3):
                check_against_float64(B.knn_topk(q33[:n], arg, k, slices), q33[:n], read, k)


@pytest.fixture(scope="module")
def tied():
    """Integer entries in -2..2 and D = 64: every sum is exact in both dtypes.  Rows are duplicated across the tile boundary (128),
    the boundaries of three slices (100, 200) and the ends."""
    rng = np.random.default_rng(5)
    q = rng.integers(-2, 3, size=(33, 64)).astype(np.float32)
    bank = rng.integers(-2, 3, size=(300, 64)).astype(np.float32)
    for a, b in ((127, 128), (99, 100), (199, 200), (0, 299), (126, 129)):
        bank[b] = bank[a]
    scores = (q.astype(np.float64) @ bank.astype(np.float64).T).astype(np.float32)
    return q, bank, scores, {k: M.topk_records(scores, k, M.EMPTY_SCORE["logit"]) for k in (5, 256)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("slices", [1, 3])
@pytest.mark.parametrize("k", [5, 256])
def test_exact_with_ties(tied, k, slices, dtype):
    q, bank, scores, want = tied
    top = np.sort(scores, axis=1)[:, -5:]
    assert (np.diff(top, axis=1) == 0).any(axis=1).sum() >= 8  # ties among the five best of many rows
    assert same_bits(B.knn_topk(q, as_bank(bank, dtype)[0], k, slices), want[k])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [10, 256])
@pytest.mark.parametrize("order", ["rising", "falling"])
def test_filter_worst_and_best_case(order, k, dtype):
    """Similarity to query 0 rising with the row (every row survives the threshold: a compaction per tile) and falling."""
    G, D = 4099, 8
    t = (np.arange(G, dtype=np.float64) + 0.5) / G
    bank = np.zeros((G, D), np.float32)
    bank[:, 0], bank[:, 1] = t, np.sqrt(1 - t * t)
    if order == "falling":
        bank = bank[::-1].copy()
    q = np.zeros((2, D), np.float32)
    q[0, 0], q[1, :2] = 1.0, (0.6, -0.8)
    arg, read = as_bank(bank, dtype)
    for slices in (0, 1):
        check_against_float64(B.knn_topk(q, arg, k, slices), q, read, k)


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_and_empty_slots(dtype):
    q, bank = unit_rows(3, 16, 21), unit_rows(200, 16, 22)
    bank[77, 3] = np.nan
    arg, read = as_bank(bank, dtype)
    clean = B.knn_topk(q, arg, 10, 3)
    check_against_float64(clean, q, read, 10)
    assert 77 not in B.split_topk(clean)[0]
    bad = q.copy()
    bad[1, 5] = np.nan
    got = B.knn_topk(bad, arg, 10, 3)
    idx, sc = B.split_topk(got)
    assert (idx[1] == EMPTY).all() and (sc[1] == -np.inf).all()
    assert same_bits(got[[0, 2]], clean[[0, 2]])
    small = as_bank(unit_rows(31, 16, 23), dtype)
    got = B.knn_topk(q, small[0], 40, 0)
    check_against_float64(got, q, small[1], 40)
    idx, sc = B.split_topk(got)
    assert (idx[:, 31:] == EMPTY).all() and (sc[:, 31:] == -np.inf).all() and (idx[:, :31] != EMPTY).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_footprint_strides_and_batch_position(dtype):
    D, k, fill = 24, 7, 0xA5A5A5A5
    q, bank = unit_rows(34, D, 31), unit_rows(300, D, 32)
    q[32] = q[0]
    arg = as_bank(bank, dtype)[0]
    plain = B.knn_topk(q[:33], arg, k, 3)
    got = B.knn_topk(q, arg, k, 3, ld_records=2 * k + 3, ldq=D + 8, ldb=D + 8, fill_bits=fill, n=33)  # NaN in the pad columns
    assert same_bits(got[:33, :2 * k], plain)
    assert (got[:33, 2 * k:].view(np.uint32) == fill).all() and (got[33].view(np.uint32) == fill).all()
    assert same_bits(plain[32], plain[0]) and same_bits(B.knn_topk(q[:1], arg, k, 0)[0], plain[0])
