"""The image walk in 64 x 256 tiles: four waves side by side share one split of A.  A workgroup stages 64 rows x
32 k per step -- threads 0..127 the first 16 of k, threads 128..255 the second -- into two 16-deep sub-buffers, runs the
24-instruction body once per sub-buffer with one barrier, and every wave column reads its own half panel of the weight image.
None of that may move a bit: every case asserts through vithip_gemm_f32_walk_tile that the geometry it means to exercise is the
one that runs, and holds `tile=9, arith=ARITH_SPLIT3, w_split=True` to the one-tile-per-workgroup kernel that splits both operands
on the fly (`tile=10`, no image), `==` on the bit patterns, with the operand recipe (`hard`) of
tests/test_gpu_split_walk_pipeline.py.

What can go wrong here is an address (a wave's panel of the image, its 64-row offset inside the panel, the block, the half, the
sub-step of a staged chunk or of a W fragment) or a moment (a sub-buffer read before the barrier that completes it or overwritten
before its last read; a fragment of the second sub-step requested or used across a segment's end; the fold's copy of 64 row
pairs; the hand-over in 32-deep steps).  The kernel these tests compare with (tile = 10, arith = ARITH_SPLIT3) is itself held to
float64 and to a bit-exact host model in tests/test_gpu_split_gemm_accuracy.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import strided
from test_gpu_split_walk_pipeline import EPILOGUES, bits, fold_rows, hard, u
from test_gpu_split_walk_wfeed import three_piece_weights
from vit_amd import binding as B

pytestmark = pytest.mark.gpu

S = B.ARITH_SPLIT3
SHARED_A, SQUARE = (64, 256), (128, 128)


def image_walk(A, W, b, geometry, **kw):
    """tile = 9 with the weight image; asserts the tile the walk reports for exactly this call."""
    w = {}
    got = B.gemm(A, W, b, tile=9, arith=S, w_split=True, walk=w, **kw)
    assert w["tile"] == geometry, (w, geometry)
    return got


# ---- the lane -> chunk map: A = I gives C[m][n] = W[n][m] exactly (lo, + mid, + hi: each partial sum exact) ---------------------

@pytest.mark.parametrize("N", [256, 768])
@pytest.mark.parametrize("K", [32, 160])
def test_identity_a_returns_w_element_by_element(K, N):
    """One tile column (N = 256: panels 0 and 1, wave columns 0..3) and three.  A wrong panel, 64-row offset inside it, block, half
    or sub-step puts another element of W where W[n][m] belongs: the elements are pairwise distinct and have three pieces each."""
    W = three_piece_weights(N, K)
    A, b = np.eye(K, dtype=np.float32), np.zeros(N, np.float32)
    got = image_walk(A, W, b, SHARED_A)
    assert np.array_equal(bits(got), bits(W.T)), np.argwhere(bits(got) != bits(W.T))[:4]
    assert np.array_equal(bits(got), bits(B.gemm(A, W, b, tile=10, arith=S)))


# ---- ragged rows and tile lengths under every epilogue -----------------------------------------------------------------------------
# M = 5 (one tile row, mostly padding), 64 x 5 + 3, 64 x 90 + 3: with N = 256 x 7 that is 91 x 7 = 637 tiles on the walk's 512
# workgroups, so workgroups cross tile boundaries and the cold requests behind an epilogue run.  K = 32, 64, 96, 160 = 1, 2, 3, 5
# steps of 32: the first step is the last; odd and even counts of prefetching steps.  Both widths are whole 256-column tiles and at
# most 2048, so the epilogue that takes the row statistics runs the same shapes.

MS, NS, KS = [5, 64 * 5 + 3, 64 * 90 + 3], [256, 256 * 7], [32, 64, 96, 160]
CASES = [(M, N, K) + e for M in MS for N in NS for K in KS for e in EPILOGUES]


@functools.lru_cache(maxsize=None)
def operands(M, N, K):
    """One set of operands per shape, shared by the cases that use it and never written."""
    ops = hard(170, (M, K), 1.0), hard(171, (N, K), 0.05), u(172, (N,), 0.1), u(173, (M, N), 2.0), fold_rows(174, M)
    for x in ops:
        x.setflags(write=False)
    return ops


@functools.lru_cache(maxsize=None)
def reference(M, N, K, epi, res, fold):
    """tile = 10: one tile per workgroup, both operands split on the fly.  Computed once per shape and epilogue."""
    A, W, b, R, rows = operands(M, N, K)
    ref = B.gemm(A, W, b, residual=R if res else None, epilogue=epi, ln=(rows, None) if fold else None, arith=S, tile=10)
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize("M,N,K,name,epi,res,fold,stats", CASES)
def test_ragged_shapes_under_every_epilogue_give_the_same_bits(M, N, K, name, epi, res, fold, stats):
    A, W, b, R, rows = operands(M, N, K)
    rs = {} if stats else None
    got = image_walk(A, W, b, SHARED_A, residual=R if res else None, epilogue=epi, ln=(rows, None) if fold else None, row_stats=rs)
    assert np.array_equal(bits(got), bits(reference(M, N, K, epi, res, fold))), (name, M, N, K)
    if stats:   # the row sums of the stored rows: those of the 128 x 128 walk that splits W on the fly
        assert rs["in_epilogue"] == 1
        rs0 = {}
        B.gemm(A, W, b, residual=R, epilogue=epi, tile=9, row_stats=rs0, arith=S)
        assert np.array_equal(bits(rs["rows"]), bits(rs0["rows"])), name


# ---- the hand-over in 32-deep steps ------------------------------------------------------------------------------------------------

def test_hand_over_on_time_and_late_gives_the_same_bits_and_clears_its_flags():
    """64 x 204 rows x 768 columns = 612 tiles on 512 workgroups: 100 owners hand the first 8 of 16 steps of their extra tile to a
    helper.  Under the GELU epilogue the pipelined step follows unpark and precedes park; the residual epilogue's walk reads its
    fragments at each pass's top.  Every owner decides exactly once, and a finished launch leaves every flag 0."""
    M, N, K = 64 * 204, 768, 512
    A, W, b, R = hard(180, (M, K), 1.0), hard(181, (N, K), 0.05), u(182, (N,), 0.1), u(183, (M, N), 2.0)
    L = B.lib()
    owners = (M // 64) * (N // 256) - 2 * B.device_info(0)["compute_units"]
    assert owners == 100 or B.device_info(0)["compute_units"] != 256
    ws = B.gemm_workspace()
    dA, dW, db, dR = (B.DeviceArray.from_numpy(a) for a in (A, W, b, R))
    dImg = B.split3_weights_device(dW, N, K)
    B.gemm_workspace_stats(ws)
    for epi, res in ((B.EPI_BIAS_GELU, None), (B.EPI_BIAS_RESIDUAL, R)):
        ref = B.gemm(A, W, b, residual=res, epilogue=epi, tile=10, arith=S)
        for late in (0, 1):
            dC = B.DeviceArray.from_numpy(np.full((M, N), 7.0, np.float32))
            args = B.CGemmArgs(dA.ptr, K, dW.ptr, K, db.ptr, dR.ptr if res is not None else None, N, dC.ptr, N, M, N, K, epi, 9, 0, ws,
                               late, None, None, None, None, S, dImg.ptr)
            assert B.gemm_walk_tile(args) == SHARED_A
            B.hip_check(L.vithip_gemm_f32(None, C.byref(args)), "vithip_gemm_f32")
            assert np.array_equal(bits(dC.numpy()), bits(ref)), (epi, late)
            st = B.gemm_workspace_stats(ws)
            assert st["taken"] + st["recomputed"] == owners, (st, late)      # every owner decided exactly once
            if late:
                assert st["recomputed"] > 0, st
            assert not B.gemm_workspace_flags(ws).any(), (epi, late)          # parked pieces consumed, withdrawn marks cleared
    L.vithip_gemm_f32_workspace_destroy(C.c_void_p(ws))


# ---- leading dimensions: lda > K, ldc > N, ldr > N; the padding of C keeps its sentinel ---------------------------------------------

@pytest.mark.parametrize("name,epi,res,fold,stats", [e for e in EPILOGUES if e[0] in ("gelu", "residual", "residual+stats", "fold")])
def test_padded_operands_give_the_same_bits_and_leave_the_padding(name, epi, res, fold, stats):
    """One shape per epilogue class: plain, plain residual, the residual walk with the row statistics, fold consumer."""
    M, N, K = 64 * 2 + 3, 256 * 2, 64
    A, W, b, R, rows = u(190, (M, K), 1.0), u(191, (N, K), 0.05), u(192, (N,), 0.1), u(193, (M, N), 2.0), fold_rows(194, M)
    kw = dict(residual=R if res else None, epilogue=epi, ln=(rows, None) if fold else None)
    out, rs = {}, ({} if stats else None)
    got = image_walk(A, W, b, SHARED_A, lda=K + 4, ldc=N + 4, ldr=N + 8 if res else None, frames=strided, out=out, row_stats=rs, **kw)
    out["C"].check()   # nothing outside the window changed, every element of it written
    assert np.array_equal(bits(got), bits(B.gemm(A, W, b, tile=10, arith=S, **kw))), name
    if stats:
        out["stats"].check()
        assert np.array_equal(bits(rs["rows"]), bits(B.rowstats_f32(got)))


# ---- special values through both sub-step halves of the workgroup ------------------------------------------------------------------

def test_special_values_in_every_block_and_sub_step_give_the_same_bits():
    """One row of A per 32-row block of each of three tile rows, with a special value at a k of the first sub-step (staged by
    threads 0..127) and one at a k of the second (threads 128..255), in a different 32-deep step each."""
    M, N, K = 64 * 2 + 3, 256, 96
    A, W, b = hard(200, (M, K), 1.0), hard(201, (N, K), 0.1), u(202, (N,), 0.1)
    special = [np.inf, -np.inf, np.nan, np.float32(1e-45), np.float32(-1e-45), np.float32(0.0), np.float32(-0.0)]
    rows = (5, 40, 64 + 20, 64 + 50, 128 + 1)
    for i, row in enumerate(rows):
        A[row, 32 * (i % 3) + (3 * i) % 16] = special[i % 7]                 # k % 32 < 16: sub-step 0
        A[row, 32 * ((i + 1) % 3) + 16 + (5 * i) % 16] = special[(i + 3) % 7]  # k % 32 >= 16: sub-step 1
    W[70, 7], W[128 + 40, 50], W[255, 95] = np.float32(1e-45), -np.inf, np.float32(-1e-45)
    ref = B.gemm(A, W, b, tile=10, arith=S)
    got = image_walk(A, W, b, SHARED_A)
    assert np.array_equal(bits(got), bits(ref))
    # +-Inf has no finite remainder (its mid piece is Inf - Inf) and NaN is NaN: rows 5, 40, 84 and 129 are NaN, and so is the
    # column of W's -Inf
    assert all(np.isnan(ref[row]).all() for row in (5, 40, 64 + 20, 128 + 1)) and np.isnan(ref[:, 128 + 40]).all()


# ---- widths the 64 x 256 tile does not take: the 128 x 128 walk stays -----------------------------------------------------------------

@pytest.mark.parametrize("N", [384, 72])
def test_widths_off_the_256_grid_run_the_square_walk(N):
    M, K = 64 * 5 + 3, 96
    A, W, b = hard(210, (M, K), 1.0), hard(211, (N, K), 0.05), u(212, (N,), 0.1)
    got = image_walk(A, W, b, SQUARE, epilogue=B.EPI_BIAS_GELU)
    assert np.array_equal(bits(got), bits(B.gemm(A, W, b, epilogue=B.EPI_BIAS_GELU, tile=10, arith=S)))
