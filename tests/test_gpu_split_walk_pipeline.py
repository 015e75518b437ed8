"""The pipelined step of the image walk (split3_step_pf): the fragments of K step g + 1 are read under the matrix
instructions of step g, the step's barrier sits inside it, a segment's first step reads its fragments at its top and its last
step prefetches none; A's split is dealt out over the gaps between the matrix instructions in quarters of a plane (the residual
epilogues' walk takes only that half).  None of that may move a bit: every case holds `tile=9, arith=ARITH_SPLIT3, w_split=True` to the
one-tile-per-workgroup kernel that splits both operands on the fly (`tile=10`, no image), `==` on the bit patterns.

Shapes: more than 512 tiles (the walk's grid is 2 workgroups per CU), so workgroups run two tiles and the cold start behind an
epilogue is exercised, with ragged last rows and columns; K = 32, 64, 96, 160 = 2, 4, 6 and 10 steps per tile: the first step
next to the last, odd and even numbers of prefetching steps between them, and tiles shorter than the fold's counted wait assumes.

A segment of a single 16-deep step cannot occur: K is a multiple of 32 (vitgemm::KALIGN), so a whole tile has an even number of
steps, at least two, and the hand-over cuts a tile at a multiple of 32 in k as well (persistent_piece_steps chooses the piece in
32-deep steps, at least four of them, and leaves the owner at least eight): both parts are even and longer than one step.
The kernel these tests compare with (tile = 10, arith = ARITH_SPLIT3) is itself held to float64 and to a bit-exact host model in
tests/test_gpu_split_gemm_accuracy.py."""
import functools

import numpy as np
import pytest

from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

S = B.ARITH_SPLIT3
SHAPES = [(128 * 101 + 5, 768), (128 * 40 + 1, 320 + 128 * 12)]


def u(k, shape, a, seed=2121):
    n = int(np.prod(shape))
    return synth.uniform(seed, k, n, -a, a).reshape(shape)


def hard(k, shape, a):
    """Uniform values over many binades, with subnormals and large magnitudes sprinkled in."""
    rng = np.random.default_rng(k)
    x = (u(k, shape, a) * np.exp2(rng.integers(-20, 8, shape))).astype(np.float32)
    flat = x.reshape(-1)
    pick, n = rng.permutation(flat.size), flat.size // 64
    flat[pick[:n]] = (rng.uniform(-1, 1, n) * 1e-39).astype(np.float32)        # subnormal
    flat[pick[n:2 * n]] = (rng.uniform(-1, 1, n) * 1e12).astype(np.float32)
    return x


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def fold_rows(k, M):
    rng = np.random.default_rng(k)
    return np.stack([rng.uniform(0.5, 1.5, M), rng.uniform(-1, 1, M)], 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def operands(M, N, K):
    """One set of operands per shape, shared by the cases that use it and never written."""
    ops = hard(50, (M, K), 1.0), hard(51, (N, K), 0.05), u(52, (N,), 0.1), u(53, (M, N), 2.0), fold_rows(54, M)
    for x in ops:
        x.setflags(write=False)
    return ops


@functools.lru_cache(maxsize=None)
def reference(M, N, K, epi, res, fold):
    """tile = 10: one tile per workgroup, both operands split on the fly."""
    A, W, b, R, rows = operands(M, N, K)
    ref = B.gemm(A, W, b, residual=R if res else None, epilogue=epi, tile=10, ln=(rows, None) if fold else None, arith=S)
    ref.setflags(write=False)
    return ref


def walk(M, N, K, epi, res, fold, **kw):
    A, W, b, R, rows = operands(M, N, K)
    return B.gemm(A, W, b, residual=R if res else None, epilogue=epi, tile=9, ln=(rows, None) if fold else None, arith=S,
                  w_split=True, **kw)


@pytest.mark.parametrize("K", [32, 64, 96, 160])
@pytest.mark.parametrize("M,N", SHAPES)
def test_short_tiles_give_the_bits_of_the_on_the_fly_split(M, N, K):
    got = walk(M, N, K, B.EPI_BIAS_GELU, False, False)
    assert np.array_equal(bits(got), bits(reference(M, N, K, B.EPI_BIAS_GELU, False, False))), (M, N, K)


# (epilogue, residual, fold consumer, row statistics): EPILOGUES of tests/test_gpu_split_weight_planes.py
EPILOGUES = [("bias", B.EPI_BIAS, False, False, False), ("gelu", B.EPI_BIAS_GELU, False, False, False),
             ("residual", B.EPI_BIAS_RESIDUAL, True, False, False), ("residual+stats", B.EPI_BIAS_RESIDUAL, True, False, True),
             ("fold", B.EPI_BIAS, False, True, False), ("fold+gelu", B.EPI_BIAS_GELU, False, True, False)]


@pytest.mark.parametrize("name,epi,res,fold,stats", EPILOGUES)
@pytest.mark.parametrize("M,N", SHAPES)
def test_every_epilogue_at_four_steps_gives_the_same_bits(name, epi, res, fold, stats, M, N):
    K = 64
    rs = {} if stats else None
    got = walk(M, N, K, epi, res, fold, row_stats=rs)
    assert np.array_equal(bits(got), bits(reference(M, N, K, epi, res, fold))), name
    if stats:   # the row sums of the stored rows: those of the walk that splits W on the fly (the step this one replaces)
        A, W, b, R, _ = operands(M, N, K)
        rs0 = {}
        B.gemm(A, W, b, residual=R, epilogue=epi, tile=9, row_stats=rs0, arith=S)
        assert np.array_equal(bits(rs["rows"]), bits(rs0["rows"])), name


@pytest.mark.parametrize("late", [0, 1])
@pytest.mark.parametrize("epi,res", [(B.EPI_BIAS_GELU, False), (B.EPI_BIAS_RESIDUAL, True)])
def test_steps_around_the_hand_over_give_the_same_bits(epi, res, late):
    """600 tiles on 512 workgroups, the hand-over on time (0) and late (1).  Under the GELU epilogue the walk runs the pipelined
    step: a prefetching step follows unpark and precedes park.  The residual epilogues' walk keeps its fragment reads behind the
    barrier and takes the finer restage slots alone."""
    M, N, K = 128 * 100, 768, 768
    st = {}
    got = walk(M, N, K, epi, res, False, workspace=True, handover_test=late, stats=st)
    assert np.array_equal(bits(got), bits(reference(M, N, K, epi, res, False))), late
    assert st["taken"] + st["recomputed"] > 0, st


def test_inf_nan_and_subnormal_operands_give_the_same_bits():
    M, N, K = 128 * 4 + 3, 128 * 129 + 72, 96    # 650 tiles, ragged both ways
    A, W, b = hard(60, (M, K), 1.0), hard(61, (N, K), 0.1), u(62, (N,), 0.1)
    W[5, 7], W[17, 40], W[130, 3], W[N - 1, 95] = np.inf, -np.inf, np.nan, np.float32(1e-45)
    A[3, 0], A[M - 1, 95], A[200, 17] = np.inf, np.nan, np.float32(-1e-45)
    ref = B.gemm(A, W, b, tile=10, arith=S)
    got = B.gemm(A, W, b, tile=9, arith=S, w_split=True)
    assert np.array_equal(bits(got), bits(ref))
    assert np.isnan(ref[:, 130]).all() and np.isnan(ref[M - 1]).all()
