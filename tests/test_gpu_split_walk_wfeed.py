"""The image walk's W feed (split3_step_pf): a wave loads its W fragments straight from the pre-split image, in
matrix operand order, a step ahead and into a second register set; LDS holds A only.  A segment's first step requests W's
fragments at its top, its last step requests none.  None of that may move a bit: every case holds `tile=9, arith=ARITH_SPLIT3,
w_split=True` to the one-tile-per-workgroup kernel that splits both operands on the fly (`tile=10`, no image), `==` on the bit
patterns, with the operand recipe (`hard`) of tests/test_gpu_split_walk_pipeline.py.

What can go wrong here is an address (the lane -> chunk map: plane, half, 32-row block, the wave's column offset, the tile's panel,
the K step) or a moment (a fragment used before it landed, or overwritten before its last use: first and last steps of a segment,
odd and even numbers of prefetching steps, a cold request behind an epilogue, behind unpark and in front of park).
The kernel these tests compare with (tile = 10, arith = ARITH_SPLIT3) is itself held to float64 and to a bit-exact host model in
tests/test_gpu_split_gemm_accuracy.py."""
import functools

import numpy as np
import pytest

import strided
from test_gpu_split_walk_pipeline import EPILOGUES, bits, fold_rows, hard, u
from vit_amd import binding as B

pytestmark = pytest.mark.gpu

S = B.ARITH_SPLIT3


# ---- the lane -> chunk map: A = I gives C[m][n] = W[n][m] exactly (lo, + mid, + hi: each partial sum exact) ---------------------

def bf16_round(x):
    """fp32 -> the nearest bf16 (ties to even), as fp32.  Finite values only."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


def three_piece_weights(N, K):
    """W[n][k] distinct per (n, k), each with three non-zero pieces: mantissa fields of 7, 8 and 8 bits, the middle one in
    2..254 and the last one odd, so that neither remainder fits the piece in front of it."""
    idx = np.arange(N * K, dtype=np.int64).reshape(N, K)
    f1, f2, f3 = idx % 127, 2 + (idx // 127) % 253, 1 + 2 * ((idx * 37) % 128)
    mant = ((f1 << 16) | (f2 << 8) | f3).astype(np.uint32)
    expo = (127 + idx // (127 * 253) - (idx % 3)).astype(np.uint32)
    sign = ((idx % 5) == 0).astype(np.uint32)
    W = ((sign << 31) | (expo << 23) | mant).view(np.float32)
    hi = bf16_round(W)
    mid = bf16_round(W - hi)
    lo = W - hi - mid
    assert (hi != 0).all() and (mid != 0).all() and (lo != 0).all() and (bf16_round(lo) == lo).all()
    assert np.unique(bits(W)).size == W.size
    return W


@pytest.mark.parametrize("N", [72, 128 + 33, 128 * 3])
@pytest.mark.parametrize("K", [32, 160])
def test_identity_a_returns_w_element_by_element(K, N):
    """N = 72: one panel, and the wave column wn = 1 sees 8 valid rows and 56 zero rows of the image.  A wrong plane, half, block
    or wave offset puts another element of W (or a zero) where W[n][m] belongs."""
    W = three_piece_weights(N, K)
    A, b = np.eye(K, dtype=np.float32), np.zeros(N, np.float32)
    got = B.gemm(A, W, b, tile=9, arith=S, w_split=True)
    assert np.array_equal(bits(got), bits(W.T)), np.argwhere(bits(got) != bits(W.T))[:4]
    assert np.array_equal(bits(got), bits(B.gemm(A, W, b, tile=10, arith=S)))


# ---- ragged rows, columns and tile lengths under every epilogue ---------------------------------------------------------------
# M x N = 5 x 72 (one tile, mostly padding) ... (128 x 5 + 3) x (128 x 129 + 72) = 6 x 130 = 780 tiles on the walk's 512 workgroups:
# workgroups cross tile boundaries, so the cold W request behind an epilogue runs.  K = 32, 64, 96, 160 = 2, 4, 6, 10 steps: the
# first step next to the last, odd and even counts of prefetching steps between them.

MS, NS, KS = [5, 128 * 5 + 3], [72, 128 * 129 + 72], [32, 64, 96, 160]
# The row statistics exist for N % 64 == 0, N <= 2048 only (vithip_gemm_f32 refuses the others), and come from the epilogue for
# N % 128 == 0: that epilogue runs the same M and K at widths it takes: one tile row, and 41 x 13 = 533 tiles.
STATS_SHAPES = [(5, 128 * 5), (128 * 40 + 3, 128 * 13)]
CASES = [(M, N, K) + e for M in MS for N in NS for K in KS for e in EPILOGUES if not e[4]] + \
        [(M, N, K) + e for M, N in STATS_SHAPES for K in KS for e in EPILOGUES if e[4]]


@functools.lru_cache(maxsize=None)
def operands(M, N, K):
    """One set of operands per shape, shared by the cases that use it and never written."""
    ops = hard(70, (M, K), 1.0), hard(71, (N, K), 0.05), u(72, (N,), 0.1), u(73, (M, N), 2.0), fold_rows(74, M)
    for x in ops:
        x.setflags(write=False)
    return ops


def run(M, N, K, epi, res, fold, image, **kw):
    A, W, b, R, rows = operands(M, N, K)
    return B.gemm(A, W, b, residual=R if res else None, epilogue=epi, ln=(rows, None) if fold else None, arith=S,
                  tile=9 if image else 10, w_split=image, **kw)


@pytest.mark.parametrize("M,N,K,name,epi,res,fold,stats", CASES)
def test_ragged_shapes_under_every_epilogue_give_the_same_bits(M, N, K, name, epi, res, fold, stats):
    rs = {} if stats else None
    got = run(M, N, K, epi, res, fold, True, row_stats=rs)
    assert np.array_equal(bits(got), bits(run(M, N, K, epi, res, fold, False))), (name, M, N, K)
    if stats:   # the row sums of the stored rows: those of the walk that splits W on the fly
        A, W, b, R, _ = operands(M, N, K)
        rs0 = {}
        B.gemm(A, W, b, residual=R, epilogue=epi, tile=9, row_stats=rs0, arith=S)
        assert np.array_equal(bits(rs["rows"]), bits(rs0["rows"])), name


# ---- the hand-over: a cold W request behind unpark, a last step without one in front of park --------------------------------------

@pytest.mark.parametrize("late", [0, 1])
@pytest.mark.parametrize("epi,res", [(B.EPI_BIAS_GELU, False), (B.EPI_BIAS_RESIDUAL, True)])
def test_hand_over_on_time_and_late_gives_the_same_bits(epi, res, late):
    M, N, K = 128 * 100, 768, 768   # 600 tiles on 512 workgroups
    st = {}
    got = run(M, N, K, epi, res, False, True, workspace=True, handover_test=late, stats=st)
    assert np.array_equal(bits(got), bits(run(M, N, K, epi, res, False, False))), late
    assert st["taken"] + st["recomputed"] > 0, st


# ---- special values: every 32-row block of every wave column of a panel, and A ------------------------------------------------

def test_inf_nan_and_subnormals_in_every_block_of_a_panel_give_the_same_bits():
    M, N, K = 128 + 3, 128 * 2, 96
    A, W, b = hard(80, (M, K), 1.0), hard(81, (N, K), 0.1), u(82, (N,), 0.1)
    special = [np.inf, -np.inf, np.nan, np.float32(1e-45)]
    for panel in range(2):
        for i, row in enumerate((5, 40, 70, 127)):   # wave column 0: blocks 0 and 1; wave column 1: blocks 0 and 1
            W[128 * panel + row, (7 * row + panel) % K] = special[(i + panel) % 4]
            W[128 * panel + row, (11 * row + 50) % K] = np.float32(-1e-45)
    A[3, 0], A[M - 1, 95], A[100, 17], A[64, 40] = np.inf, np.nan, np.float32(-1e-45), -np.inf
    ref = B.gemm(A, W, b, tile=10, arith=S)
    got = B.gemm(A, W, b, tile=9, arith=S, w_split=True)
    assert np.array_equal(bits(got), bits(ref))
    assert np.isnan(ref[M - 1]).all() and np.isnan(ref[:, 70]).all() and np.isnan(ref[:, 128 + 40]).all()


# ---- leading dimensions: lda > K, ldc > N, the padding of C keeps its sentinel ------------------------------------------------

@pytest.mark.parametrize("epi,res", [(B.EPI_BIAS_GELU, False), (B.EPI_BIAS_RESIDUAL, True)])
def test_padded_a_and_c_give_the_same_bits_and_leave_the_padding(epi, res):
    M, N, K = 128 + 3, 128 + 72, 64
    A, W, b, R = u(90, (M, K), 1.0), u(91, (N, K), 0.05), u(92, (N,), 0.1), u(93, (M, N), 2.0)
    out = {}
    got = B.gemm(A, W, b, residual=R if res else None, epilogue=epi, tile=9, arith=S, w_split=True, lda=K + 4, ldc=N + 4,
                 frames=strided, out=out)
    out["C"].check()   # nothing outside the window changed, every element of it written
    ref = B.gemm(A, W, b, residual=R if res else None, epilogue=epi, tile=10, arith=S)
    assert np.array_equal(bits(got), bits(ref))
