"""A numpy model of the three-piece split of the fp32 GEMMs (vithip_gemm_args.arith = 1, csrc/vit_gemm_common.hpp): every fp32
operand is hi + mid + lo bf16 pieces, exactly, and the six piece products of rank <= 2 accumulated per 16-deep K step in the
kernel's order are no less accurate than a sequential fp32 FMA chain.  No GPU.

The model of one v_mfma_f32_32x32x16_bf16: the 16 products of a step are exact in fp32 (8-bit x 8-bit significands) and their
sum is added to the accumulator with one rounding (the sum itself in float64 here)."""
import numpy as np
import pytest

TERMS = ((0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0))   # (A piece, W piece), 0 = hi, 1 = mid, 2 = lo: the kernel's order


def bf16_rne(x):
    x = np.asarray(x, np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def split3(x):
    x = np.asarray(x, np.float32)
    hi = bf16_rne(x)
    r1 = (x - hi).astype(np.float32)
    mid = bf16_rne(r1)
    lo = bf16_rne((r1 - mid).astype(np.float32))
    return hi, mid, lo


def split_gemm(A, W):
    """A [M][K] . W[N][K]^T the way the split kernels compute it."""
    K = A.shape[1]
    pa, pw = split3(A), split3(W)
    acc = np.zeros((A.shape[0], W.shape[0]), np.float32)
    for k0 in range(0, K, 16):
        for ia, iw in TERMS:
            step = pa[ia][:, k0:k0 + 16].astype(np.float64) @ pw[iw][:, k0:k0 + 16].astype(np.float64).T
            acc = (acc.astype(np.float64) + step).astype(np.float32)
    return acc


def fma_chain(A, W):
    """The sequential fp32 chain: one rounding per product added (what v_mfma_f32_32x32x2_f32 does per k)."""
    acc = np.zeros((A.shape[0], W.shape[0]), np.float32)
    A64, W64 = A.astype(np.float64), W.astype(np.float64)
    for k in range(A.shape[1]):
        acc = (acc.astype(np.float64) + np.outer(A64[:, k], W64[:, k])).astype(np.float32)
    return acc


def test_pieces_add_up_exactly_across_the_exponent_range():
    rng = np.random.default_rng(0)
    # normal fp32 values from 2^-100 to 2^100 and both signs, plus the awkward significands (all ones, halfway cases)
    e = rng.integers(-100, 100, 200_000)
    x = (rng.uniform(1.0, 2.0, e.size) * np.exp2(e.astype(np.float64))).astype(np.float32)
    x *= np.where(rng.random(x.size) < 0.5, -1, 1).astype(np.float32)
    # (outside the range: |x| within half a bf16 ulp of FLT_MAX, whose hi rounds to inf, and x below 2^-110 or so, whose lo is a
    # subnormal -- neither is an activation or a weight of this model)
    special = np.array([1.0, -1.0, 1.9999999, 1.00390625, 1.0039062, 1.0039063, 3.3e38, 1.2e-30], np.float32)
    x = np.concatenate([x, special, np.nextafter(special, np.float32(np.inf)), np.zeros(1, np.float32)])
    hi, mid, lo = split3(x)
    for piece in (hi, mid, lo):                           # each piece is a bf16 value
        assert not (piece.view(np.uint32) & 0xFFFF).any()
    total = hi.astype(np.float64) + mid.astype(np.float64) + lo.astype(np.float64)
    assert np.array_equal(total, x.astype(np.float64))
    # the dropped products are small: |mid| <= 2^-8 |x|, |lo| <= 2^-16 |x|
    nz = x != 0
    assert (np.abs(mid[nz]) <= np.abs(x[nz]) * 2.0 ** -8).all() and (np.abs(lo[nz]) <= np.abs(x[nz]) * 2.0 ** -16).all()


def test_identity_product_is_exact():
    rng = np.random.default_rng(1)
    W = rng.standard_normal((48, 64)).astype(np.float32) * np.float32(3.7)
    assert np.array_equal(split_gemm(np.eye(64, dtype=np.float32), W), W.T)


def _operands(kind, M, N, K, rng):
    if kind == "ops":        # the operand ranges of tests/test_gpu_ops.py (uniform activations, 0.05-scaled weights)
        return rng.uniform(-1, 1, (M, K)).astype(np.float32), (rng.standard_normal((N, K)) * 0.05).astype(np.float32)
    # the LayerNorm fold's near-constant rows (tests/test_gpu_lnfold.py): a large common offset plus tiny variation, against
    # the centred weights
    A = (5.0 + rng.standard_normal((M, K)) * 1e-3).astype(np.float32)
    W = (rng.standard_normal((N, K)) * 0.05).astype(np.float32)
    return A, (W - W.mean(1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("kind", ["ops", "fold"])
@pytest.mark.parametrize("K", [768, 3072])
def test_split_dot_products_are_no_worse_than_an_fp32_chain(kind, K):
    rng = np.random.default_rng(K + len(kind))
    A, W = _operands(kind, 24, 20, K, rng)
    exact = A.astype(np.float64) @ W.astype(np.float64).T
    mag = np.abs(A).astype(np.float64) @ np.abs(W).astype(np.float64).T     # the scale of the rounding errors
    e_split = np.abs(split_gemm(A, W) - exact) / mag
    e_chain = np.abs(fma_chain(A, W) - exact) / mag
    assert e_split.max() <= e_chain.max()
    assert e_split.mean() <= e_chain.mean()
    assert e_split.max() < 2e-7
