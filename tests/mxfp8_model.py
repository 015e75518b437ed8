"""The MXFP8 format of include/vit_hip_kernels.h on the host, and a float64 pre-norm ViT forward over the Network tensor order with a
hook on the operands of the four encoder linears (QKV, out_proj, fc1, fc2)."""
import numpy as np
import torch


def quantize_mx(x, axis=-1):
    """x -> its MXFP8 value in float64: blocks of 32 along `axis`, X = floor(log2(amax)) - 8 in [-127, 127] (amax == 0: -127),
    elements x * 2^-X clamped to +-448 (torch's float8_e4m3fn does not saturate) and rounded to nearest even to e4m3."""
    x = np.moveaxis(np.asarray(x, np.float64), axis, -1)
    b = x.reshape(x.shape[:-1] + (x.shape[-1] // 32, 32))
    amax = np.abs(b).max(-1, keepdims=True)
    X = np.where(amax > 0, np.clip(np.frexp(amax)[1] - 1 - 8, -127, 127), -127).astype(np.int32)   # frexp: amax = m 2^e, m in [0.5, 1)
    scaled = np.clip(np.ldexp(b, -X), -448.0, 448.0)
    q = torch.from_numpy(scaled).to(torch.float32).to(torch.float8_e4m3fn).to(torch.float64).numpy()
    return np.moveaxis(np.ldexp(q, X).reshape(x.shape), -1, axis)


def quantize_both(a, w):
    return quantize_mx(a), quantize_mx(w)


def layernorm(x, g, b, eps):
    mu, var = x.mean(-1, keepdims=True), x.var(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * g + b


def forward_cls(cfg, weights, images, hook=None, eps=1e-6):
    """The final LayerNorm of the class rows [n][D] (the engine's features("cls")) of a GELU model, in float64.  hook(a, w) -> (a, w)
    replaces the operands of every encoder linear a @ w.T."""
    W = [np.asarray(w, np.float64) for w in weights]
    D, P, heads, n = cfg.embed_dim, cfg.patch_size, cfg.num_heads, images.shape[0]
    G, hd = cfg.img_size // P, D // heads

    def linear(a, w, b):
        a, w = hook(a, w) if hook else (a, w)
        return a @ w.T + b

    p = np.asarray(images, np.float64).reshape(n, cfg.in_chans, G, P, G, P).transpose(0, 2, 4, 1, 3, 5).reshape(n, G * G, -1)
    pos = W[3].reshape(-1, D)
    x = np.concatenate([np.broadcast_to(W[0].reshape(1, -1, D), (n, 1, D)), p @ W[1].reshape(D, -1).T + W[2]], 1) + pos
    for l in range(cfg.depth):
        g1, b1, wq, bq, wo, bo, g2, b2, w1, bb1, w2, bb2 = W[4 + 12 * l: 16 + 12 * l]
        q, k, v = (t.reshape(n, -1, heads, hd).transpose(0, 2, 1, 3) for t in np.split(linear(layernorm(x, g1, b1, eps), wq.reshape(3 * D, D), bq), 3, -1))
        s = q @ k.transpose(0, 1, 3, 2) / np.sqrt(hd)
        s = np.exp(s - s.max(-1, keepdims=True))
        y = ((s / s.sum(-1, keepdims=True)) @ v).transpose(0, 2, 1, 3).reshape(n, -1, D)
        x = x + linear(y, wo.reshape(D, D), bo)
        h = linear(layernorm(x, g2, b2, eps), w1.reshape(-1, D), bb1)
        h = 0.5 * h * (1.0 + torch.erf(torch.from_numpy(h / np.sqrt(2.0))).numpy())
        x = x + linear(h, w2.reshape(D, -1), bb2)
    return layernorm(x[:, 0], W[-4], W[-3], eps)
