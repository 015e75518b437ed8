"""vithip_mxfp8_weights + vithip_gemm_mxfp8 against quantize_mx(A) @ quantize_mx(W).T + bias in float64 (tests/mxfp8_model.py).

Bar per element: K * 2^-23 * (|A^| @ |W^|.T) -- twice the worst case of any fp32 summation order with round to nearest; the factor of
two allows a truncating adder tree inside the matrix instruction.  bf16 outputs add one bf16 ulp of |ref|; the activations take the
pre-activation's bar through their Lipschitz constants (GELU 1.13, QuickGELU 1.10), and GELU the 4.5e-8 the header states for the
kernels' polynomial below -4 sqrt 2.  At K <= 256 the bar is below 4e-5 of the term sum and one fp8 step is 6e-2 of an element: a
single element rounded or scaled differently from the model fails.  Bias and residual are U(-1, 1) beside term sums of K / 4 and
more, so their two fp32 additions stay far inside the bar.

Operands are U(-1, 1) with these blocks planted in A (bf16) and W (fp32) alike: all zero; amax a power of two; x * 2^-X in (448, 512)
and at 448; fp8 subnormals with ties at 2^-10 and 2.5 * 2^-9; exact ties between two e4m3 values, both parities; amax 2^-120 (X at
its clamp); and one row alternating blocks of magnitude 1e4 and 1e-4.  A's pad columns [K, lda) and guard rows hold NaN patterns
(tests/strided.py) and every output frame is checked for stores outside its window."""
import numpy as np
import pytest

import bf16_gemm_model as G
import strided
from mxfp8_model import quantize_mx
from vit_amd import binding as B

pytestmark = pytest.mark.gpu
SHAPES = [(1, 8, 64, 64), (33, 136, 192, 200), (287, 264, 128, 128), (5, 128, 256, 3 * 256)]   # M, N, K, lda
EPILOGUES = {"bf16": B.BF16_EPI_BF16, "gelu": B.BF16_EPI_BF16_GELU, "qgelu": B.BF16_EPI_BF16_QGELU, "residual": B.BF16_EPI_F32_RESIDUAL}


def bf16_exact(x):
    return B.from_bf16_bits(B.to_bf16_bits(np.asarray(x, np.float32)))


def special_blocks(rng):
    u = lambda s=1.0: bf16_exact(rng.uniform(-s, s, 32))
    zero, pow2, sat, sub, tie, tiny = np.zeros(32, np.float32), 0.9 * u(), 0.9 * u(), 0.5 * u(), 0.5 * u(), u()
    pow2[5] = 2.0
    sat[[0, 3, 9, 30]] = [1.9375, -1.875, 1.75, 1.8125]                    # X = -8: 496, -480, 448, 464
    sub[0], sub[1:6] = 1.0, np.ldexp([3.0, 2.5, 0.5, -1.5, 7.5], -17)     # X = -8: 3, 2.5, 0.5, -1.5, 7.5 steps of 2^-9
    tie[0], tie[1:5] = 1.0, np.array([17.0, 19.0, -34.0, 3.25]) / 256      # X = -8: 17 -> 16, 19 -> 20, -34 -> -32, 3.25 -> 3.25
    return [zero, bf16_exact(pow2), sat, sub, tie, np.ldexp(tiny, -120).astype(np.float32)]


def operands(M, N, K, seed=38):
    """A bf16-exact [M][K] and W fp32 [N][K] with the special blocks planted at every second block, and the mixed row."""
    rng = np.random.default_rng(seed + 1000 * M + N + K)
    A, W = bf16_exact(rng.uniform(-1, 1, (M, K))), rng.uniform(-1, 1, (N, K)).astype(np.float32)
    for X in (A, W):
        blocks = X.reshape(-1, 32)
        if X.shape[0] > 2:   # row 1: blocks of magnitude 1e4 and 1e-4 side by side
            X[1] = bf16_exact(rng.uniform(-1, 1, K) * np.repeat(np.where(np.arange(K // 32) % 2, 1e-4, 1e4), 32))
        for i, blk in enumerate(special_blocks(rng)):
            if 4 * i < len(blocks):   # the two blocks of the smallest A: one random, one zero
                blocks[(7 * i + 1) % len(blocks)] = blk
    return bf16_exact(A), W


@pytest.mark.parametrize("epi", list(EPILOGUES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm_against_the_float64_model(shape, epi):
    M, N, K, lda = shape
    A, W = operands(M, N, K)
    rng = np.random.default_rng(7)
    bias, R = rng.uniform(-1, 1, N).astype(np.float32), rng.uniform(-1, 1, (M, N)).astype(np.float32)
    Aq, Wq, out = quantize_mx(A), quantize_mx(W), {}
    pre, bar = Aq @ Wq.T + bias.astype(np.float64), K * 2.0 ** -23 * (np.abs(Aq) @ np.abs(Wq).T)
    if epi == "residual":   # in place, ldc > N
        got = B.gemm_mxfp8(B.to_bf16_bits(A), W, bias, R, EPILOGUES[epi], lda=lda, ldc=N + 4, in_place=True, frames=strided, out=out)
        ref = pre + R
    else:
        got = B.from_bf16_bits(B.gemm_mxfp8(B.to_bf16_bits(A), W, bias, None, EPILOGUES[epi], lda=lda, ldc=N + 8, frames=strided, out=out))
        ref, lip, floor = {"bf16": (pre, 1.0, 0.0), "gelu": (G.gelu_f64(pre), 1.13, 4.5e-8), "qgelu": (G.quick_gelu_f64(pre), 1.10, 0.0)}[epi]
        bar = lip * bar + floor + np.ldexp(1.0, np.frexp(np.abs(ref))[1] - 1 - 7)
    out["C"].check()
    err = np.abs(got.astype(np.float64) - ref)
    worst = np.unravel_index(np.argmax(err - bar), err.shape)
    print(f"{shape} {epi}: max err / bar = {(err / bar).max():.3f}, worst at {worst}: got {got[worst]!r}, ref {ref[worst]!r}, bar {bar[worst]:.3e}")
    assert (err <= bar).all()


def test_weight_image_and_gemm_on_an_identity_give_the_quantised_weights_exactly():
    """A = I (every block of A: amax 1, element 256 * 2^-8 exactly): C = W^.T with no rounding anywhere, element for element; and the
    image itself: the e8m0 bytes and the element bytes of vithip_mxfp8_weights in the layout the header states."""
    N, K = 136, 128
    W = operands(3, N, K, seed=5)[1]
    W[2] *= np.float32(2.0 ** 20)
    Wq = quantize_mx(W)
    Wg = np.where(np.abs(W) < 2.0 ** -100, np.float32(0), W)   # the GEMM's half: fp32 subnormals of C are not the format's business
    got = B.gemm_mxfp8(B.to_bf16_bits(np.eye(K, dtype=np.float32)), Wg, np.zeros(N), np.zeros((K, N)), B.BF16_EPI_F32_RESIDUAL)
    assert np.array_equal(got.astype(np.float64), quantize_mx(Wg).T)
    img = B.mxfp8_weights(W)                              # [32-row block][K step][2112]
    assert img.shape == (8, K // 64, 2112)
    elems = img[:, :, :2048].reshape(8, K // 64, 2, 32, 2, 16).transpose(0, 3, 1, 4, 2, 5).reshape(256, K)   # [row][k]
    scales = img[:, :, 2048:].reshape(8, K // 64, 2, 32).transpose(0, 3, 1, 2).reshape(256, K // 32).astype(np.int32)
    import torch
    deq = torch.from_numpy(elems.copy()).view(torch.float8_e4m3fn).to(torch.float64).numpy() * np.repeat(np.ldexp(1.0, scales - 127), 32, 1)
    assert np.array_equal(deq[:N], Wq) and not elems[N:].any() and not scales[N:].any()
    amax = np.abs(W.astype(np.float64)).reshape(N, K // 32, 32).max(-1)
    assert np.array_equal(scales[:N], np.where(amax > 0, np.clip(np.frexp(amax)[1] - 9, -127, 127), -127) + 127)
