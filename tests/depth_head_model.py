"""The depth head's tail (vithip_dense_depth_f32) twice over, for the GPU tests: the upstream order in float64 through
torch.nn.functional.interpolate, and the header's arithmetic restated in numpy fp32 (every product and sum rounded, bins summed
ascending).  The distance between the two is the reference's own fp32 error, E32, from which the tests take their bar."""
import numpy as np
import torch
import torch.nn.functional as F


def reference64(cell, centres, g, u, out_hw, min_depth, max_depth):
    """cell [n][g * g][bins] (logits + z, any float dtype) -> float64 [n][out_h][out_w]: interpolate, relu + 0.1, normalise, expectation,
    clamp, interpolate."""
    x = torch.from_numpy(np.asarray(cell, np.float64)).reshape(len(cell), g, g, -1).permute(0, 3, 1, 2)
    up = F.interpolate(x, size=(u * g, u * g), mode="bilinear", align_corners=False)
    r = torch.relu(up) + 0.1
    r = r / r.sum(dim=1, keepdim=True)
    d = torch.einsum("nbhw,b->nhw", r, torch.from_numpy(np.asarray(centres, np.float64)))
    d = d.clamp(float(min_depth), float(max_depth))
    return F.interpolate(d[:, None], size=tuple(out_hw), mode="bilinear", align_corners=False)[:, 0].numpy()


def _taps(src_n, dst_n):
    f = np.float32
    src = np.maximum(f(src_n) / f(dst_n) * (np.arange(dst_n, dtype=f) + f(0.5)) - f(0.5), f(0))
    i0 = np.minimum(src.astype(np.int64), src_n - 1)
    l1 = src - i0.astype(f)
    return i0, i0 + (i0 < src_n - 1), f(1) - l1, l1


def _resize32(m, dst_h, dst_w):
    """m fp32 [n][h][w][...] -> [n][dst_h][dst_w][...] with the header's per-axis expressions."""
    y0, y1, ly0, ly1 = _taps(m.shape[1], dst_h)
    x0, x1, lx0, lx1 = _taps(m.shape[2], dst_w)
    ex = (slice(None),) + (None,) * (m.ndim - 3)
    top, bot = m[:, y0], m[:, y1]
    h0 = lx0[ex] * top[:, :, x0] + lx1[ex] * top[:, :, x1]
    h1 = lx0[ex] * bot[:, :, x0] + lx1[ex] * bot[:, :, x1]
    ey = (None, slice(None), None) + (None,) * (m.ndim - 3)
    return ly0[ey] * h0 + ly1[ey] * h1


def restate32(cell, centres, g, u, out_hw, min_depth, max_depth):
    """The contract in fp32: cell fp32 [n][g * g][bins] -> fp32 [n][out_h][out_w]."""
    f = np.float32
    v = _resize32(np.asarray(cell, f).reshape(len(cell), g, g, -1), u * g, u * g)
    r = np.where(v < 0, f(0), v) + f(0.1)
    s = np.cumsum(r, axis=-1, dtype=f)[..., -1]  # cumsum adds in order, one rounding per bin
    t = np.cumsum(r * np.asarray(centres, f), axis=-1, dtype=f)[..., -1]
    d = np.clip(t / s, f(min_depth), f(max_depth))
    return _resize32(d, *out_hw)


def bar(ref64, cell32, centres, g, u, out_hw, min_depth, max_depth):
    """(E32, the bar): 4 x the fp32 restatement's own distance from float64 (another order of up to 256 additions), floored at four
    roundings of a value up to max_depth (clamp and stage 2)."""
    e32 = float(np.abs(restate32(cell32, centres, g, u, out_hw, min_depth, max_depth).astype(np.float64) - ref64).max())
    return e32, max(4 * e32, 2.0 ** -22 * max_depth)
