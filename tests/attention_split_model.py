"""A numpy model of the split attention kernel (vithip_attention_f32_split, csrc/vit_attention_hd.hip: attention_split_kernel) for
one head of 64 columns, a float64 reference and a sequential-fp32 evaluation to set it against.  No GPU.

The model follows the kernel step by step: Q, K, V and the softmax weights P in three bf16 pieces (hi, mid, lo, each rounded to
nearest even; torch does the rounding), keys in tiles of 32, the contraction over d in four steps of 16 with the six piece products
of a step added small terms first, the exp2 softmax with the deferred running maximum (it moves only when a row's scores outgrow it
by more than 2^8), the row sums in the kernel's lane order (two half-wave sums of fp32 adds), P.V sixteen keys at a time with the
same six terms, and one multiplication by the reciprocal of the row sum at the end.

The model of one v_mfma_f32_32x32x16_bf16 is the one of tests/test_split_gemm_model.py: the 16 products of a step are exact in fp32
and their sum (float64 here) is added to the accumulator with one rounding.  v_exp_f32 is float64 exp2 rounded to fp32.
"""
import numpy as np
import torch

TERMS = ((0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0))  # (K or V piece, Q or P piece), 0 = hi, 1 = mid, 2 = lo: the kernel's order
HD = 64
SCALE = np.float32(0.125 * 1.4426950408889634)            # (1 / sqrt(64)) * log2(e): kScale64
DEFER = np.float32(8.0)


def f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


def bf16_rne(x):
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    return t.to(torch.bfloat16).to(torch.float32).numpy()


def split3(x):
    x = np.asarray(x, np.float32)
    hi = bf16_rne(x)
    r1 = (x - hi).astype(np.float32)
    mid = bf16_rne(r1)
    lo = bf16_rne((r1 - mid).astype(np.float32))
    return hi, mid, lo


def mfma(acc, a, b):
    """acc [M][N] fp32 += a [M][16] . b [N][16]^T: exact products, one rounding."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (acc.astype(np.float64) + a.astype(np.float64) @ b.astype(np.float64).T).astype(np.float32)


def tile_keys(h):
    """The keys of a 32-key tile that half-wave h holds in registers 0..15."""
    v = np.arange(16)
    return (v & 3) + 8 * (v >> 2) + 4 * h


def attention_split(q, k, v):
    """q [Tq][64], k, v [T][64] fp32 -> [Tq][64] fp32, as attention_split_kernel computes one head."""
    q, k, v = (np.asarray(a, np.float32) for a in (q, k, v))
    Tq, T = q.shape[0], k.shape[0]
    pad = (T + 31) // 32 * 32
    kp, vp = np.zeros((pad, HD), np.float32), np.zeros((pad, HD), np.float32)
    kp[:T], vp[:T] = k, v
    qs, ks, vs = split3(q), split3(kp), split3(vp)
    o = np.zeros((Tq, HD), np.float32)
    m_run = np.full(Tq, -np.inf, np.float32)
    l_run = np.zeros((2, Tq), np.float32)  # the two half-waves' sums
    for tile0 in range(0, T, 32):
        s = np.zeros((Tq, 32), np.float32)
        for d0 in range(0, HD, 16):
            for ik, iq in TERMS:
                s = mfma(s, qs[iq][:, d0:d0 + 16], ks[ik][tile0:tile0 + 32, d0:d0 + 16])
        s[:, np.arange(32) + tile0 >= T] = -np.inf
        cmax = s.max(1)
        with np.errstate(invalid="ignore"):
            moved = f32((cmax - m_run).astype(np.float32).astype(np.float64) * SCALE) > DEFER
        m_new = np.where(moved, cmax, m_run).astype(np.float32)
        mneg = f32(-m_new.astype(np.float64) * SCALE)
        with np.errstate(invalid="ignore", over="ignore"):
            p = f32(np.exp2(f32(s.astype(np.float64) * SCALE + mneg[:, None].astype(np.float64)).astype(np.float64)))
            alpha = f32(np.exp2(f32((m_run - m_new).astype(np.float32).astype(np.float64) * SCALE).astype(np.float64)))
        alpha = np.where(moved, alpha, np.float32(1.0)).astype(np.float32)
        m_run = m_new
        l_run = l_run * alpha[None, :]
        o = o * alpha[:, None]
        for h in range(2):
            acc = np.zeros(Tq, np.float32)
            for key in tile_keys(h):
                acc = acc + p[:, key]
            l_run[h] = l_run[h] + acc
        ps = split3(p)
        for g0 in range(0, 32, 16):
            if tile0 + g0 >= T:
                break
            keys = slice(tile0 + g0, tile0 + g0 + 16)
            for iv, ip in TERMS:
                o = mfma(o, ps[ip][:, g0:g0 + 16], vs[iv][keys].T)
    inv = np.float32(1.0) / (l_run[0] + l_run[1])
    return o * inv[:, None]


def attention_f64(q, k, v):
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    s = q @ k.T / 8.0
    p = np.exp(s - s.max(1, keepdims=True))
    return (p / p.sum(1, keepdims=True)) @ v


def attention_f32_sequential(q, k, v):
    """Plain fp32, one operation after the other: every score an FMA chain over d, the row maximum, p = exp2(fma(s, c, -m c)), the
    row sum and every output an FMA chain over the keys, one multiplication by the reciprocal of the sum."""
    q, k, v = (np.asarray(a, np.float32) for a in (q, k, v))
    Tq, T = q.shape[0], k.shape[0]
    s = np.zeros((Tq, T), np.float32)
    for d in range(HD):
        s = f32(s.astype(np.float64) + np.outer(q[:, d].astype(np.float64), k[:, d].astype(np.float64)))
    mneg = f32(-s.max(1).astype(np.float64) * SCALE)
    p = f32(np.exp2(f32(s.astype(np.float64) * SCALE + mneg[:, None].astype(np.float64)).astype(np.float64)))
    total = np.zeros(Tq, np.float32)
    o = np.zeros((Tq, HD), np.float32)
    for key in range(T):
        total = total + p[:, key]
        o = f32(o.astype(np.float64) + np.outer(p[:, key].astype(np.float64), v[key].astype(np.float64)))
    return o * (np.float32(1.0) / total)[:, None]
