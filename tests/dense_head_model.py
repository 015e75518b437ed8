"""The dense linear head's arithmetic in numpy: what vithip_dense_upsample_argmax_f32 and vit_dense_head_fold_batchnorm state.

Upsampling, per axis of g source cells and `out` destination pixels, in fp32, every product and sum rounded on its own:

    scale = (float)g / (float)out
    src   = scale * ((float)dst + 0.5f) - 0.5f, a negative value becomes 0
    i0 = (int)src;  i1 = i0 + (i0 < g - 1);  l1 = src - (float)i0;  l0 = 1.0f - l1

    v = l0y * (l0x * v00 + l1x * v01) + l1y * (l0x * v10 + l1x * v11)

and the label of a pixel: the class of the highest v; among equal values (==) the lower label; a class whose v is NaN is not a
candidate (+-Inf are ordinary values); a pixel without a candidate gets 255.  numpy float32 arrays round every operation to fp32 and
fuse nothing, so the functions below are that statement, value for value.
"""
import numpy as np

NO_LABEL = 255
F = np.float32


def axis_taps(g: int, out: int):
    """(i0, i1, l0, l1) of every destination index 0..out-1: int64 indices, float32 weights."""
    scale = F(g) / F(out)
    src = scale * (np.arange(out).astype(F) + F(0.5)) - F(0.5)
    src = np.where(src < F(0), F(0), src).astype(F)
    i0 = src.astype(np.int64)
    i1 = i0 + (i0 < g - 1)
    l1 = (src - i0.astype(F)).astype(F)
    l0 = (F(1.0) - l1).astype(F)
    return i0, i1, l0, l1


def upsample(logits, g: int, out_h: int, out_w: int) -> np.ndarray:
    """logits [g * g][classes] (patch p in raster order) -> float32 [out_h][out_w][classes], the interpolated values."""
    m = np.ascontiguousarray(logits, F).reshape(g, g, -1)
    y0, y1, l0y, l1y = axis_taps(g, out_h)
    x0, x1, l0x, l1x = axis_taps(g, out_w)
    l0x, l1x = l0x[None, :, None], l1x[None, :, None]
    l0y, l1y = l0y[:, None, None], l1y[:, None, None]
    with np.errstate(invalid="ignore", over="ignore"):
        top = l0x * m[y0][:, x0] + l1x * m[y0][:, x1]
        bot = l0x * m[y1][:, x0] + l1x * m[y1][:, x1]
        v = l0y * top + l1y * bot
    assert v.dtype == F
    return v


def argmax_labels(v) -> np.ndarray:
    """v [...][classes] -> uint8 [...]: higher wins, ties to the lower label, NaN is no candidate, no candidate gives 255."""
    v = np.asarray(v, F)
    assert 1 <= v.shape[-1] <= 255
    best = np.full(v.shape[:-1], -np.inf, F)
    label = np.full(v.shape[:-1], NO_LABEL, np.uint8)
    for c in range(v.shape[-1]):  # ascending: an equal value never replaces the lower label
        vc = v[..., c]
        with np.errstate(invalid="ignore"):
            take = (vc > best) | ((label == NO_LABEL) & ~np.isnan(vc))
        best = np.where(take, vc, best)
        label = np.where(take, np.uint8(c), label)
    return label


def labels(logits, g: int, out_h: int, out_w: int) -> np.ndarray:
    """logits [g * g][classes] -> uint8 [out_h][out_w]."""
    return argmax_labels(upsample(logits, g, out_h, out_w))


def labels_batch(logits, g: int, out_h: int, out_w: int) -> np.ndarray:
    """logits [n][g * g][classes] -> uint8 [n][out_h][out_w]."""
    return np.stack([labels(l, g, out_h, out_w) for l in logits])


def grid_to_logits(grid) -> np.ndarray:
    """A GRID row [classes][g][g] back to token-major logits [g * g][classes]."""
    grid = np.asarray(grid, F)
    return np.ascontiguousarray(grid.reshape(grid.shape[0], -1).T)


def fold_batchnorm(weight, bias, gamma, beta, mean, var, eps):
    """vit_dense_head_fold_batchnorm: in double, k ascending, one sum after the other (np.cumsum adds in order; np.sum does not).
    s[k] = gamma[k] / sqrt(var[k] + eps); b'[c] = (float)(b[c] + sum_k W[c][k] * (beta[k] - mean[k] * s[k])); W'[c][k] = (float)(W[c][k] * s[k])."""
    W = np.asarray(weight, F).astype(np.float64)
    b = np.asarray(bias, F).astype(np.float64)
    gamma, beta, mean, var = (np.asarray(a, F).astype(np.float64) for a in (gamma, beta, mean, var))
    s = gamma / np.sqrt(var + np.float64(eps))
    t = beta - mean * s
    sums = np.array([np.cumsum(np.concatenate(([0.0], W[c] * t)))[-1] for c in range(W.shape[0])])
    return (W * s).astype(F), (b + sums).astype(F)
