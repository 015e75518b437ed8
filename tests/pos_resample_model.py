"""Resampling of a ViT position embedding to another patch grid, restated in numpy (helper, no tests in it).

The definition that csrc/vit_pos_resample.hip and vit_engine_load_weights_resampled are compared with (DESIGN.md states it too).
pos [1 + g_src^2][D]: row 0, the class token's embedding, is copied; rows 1.. are a g_src x g_src raster of D-vectors that is resampled
to g_dst x g_dst, separably.  An axis is a table: per output index a first source index, a tap count and fp32 weights; the source
index of tap k is clamp(first + k, 0, in - 1).  Every operation is one IEEE fp32 operation (numpy float32 scalars: a product and a sum
are two roundings, never a fused multiply-add).

    "bicubic"     torch.nn.functional.interpolate(mode="bicubic", align_corners=False, antialias=False)   A = -0.75, always 4 taps
    "bicubic_aa"  the same with antialias=True (timm's resample_abs_pos_embed)                             A = -0.5, support scales

tests/test_pos_resample_model.py pins it to PyTorch's CPU kernels; the host table of the library has to equal table() bit for bit.
"""
import numpy as np

MODES = {"bicubic": 0, "bicubic_aa": 1}  # VIT_POS_BICUBIC, VIT_POS_BICUBIC_AA
F = np.float32


def _mode(mode) -> int:
    return MODES[mode] if isinstance(mode, str) else int(mode)


def _table_bicubic(n_in: int, n_out: int):
    A = F(-0.75)

    def cub1(x):
        return ((A + F(2)) * x - (A + F(3))) * x * x + F(1)

    def cub2(x):
        return ((A * x - F(5) * A) * x + F(8) * A) * x - F(4) * A

    scale = F(n_in) / F(n_out)
    rows = []
    for o in range(n_out):
        r = scale * (F(o) + F(0.5)) - F(0.5)
        b = np.floor(r)
        t = F(r - b)
        w = [cub2(t + F(1)), cub1(t), cub1(F(1) - t), cub2(F(2) - t)]
        rows.append((int(b) - 1, np.array(w, np.float32)))
    return rows


def _filter_aa(x):
    A = F(-0.5)
    x = F(abs(x))
    if x < F(1):
        return ((A + F(2)) * x - (A + F(3))) * x * x + F(1)
    if x < F(2):
        return (((x - F(5)) * x + F(8)) * x - F(4)) * A
    return F(0)


def _table_aa(n_in: int, n_out: int):
    scale = F(n_in) / F(n_out)
    support = F(2) * scale if scale >= F(1) else F(2)
    inv = F(1) / scale if scale >= F(1) else F(1)
    rows = []
    for o in range(n_out):
        center = scale * (F(o) + F(0.5))
        xmin = max(int(center - support + F(0.5)), 0)
        cnt = min(int(center + support + F(0.5)), n_in) - xmin
        w = [_filter_aa((F(j + xmin) - center + F(0.5)) * inv) for j in range(cnt)]
        tot = F(0)
        for v in w:
            tot = F(tot + v)
        rows.append((xmin, np.array([F(v / tot) for v in w], np.float32)))
    return rows


def table(mode, n_in: int, n_out: int):
    """The axis table: a list of n_out pairs (first source index, float32 weights); len(weights) is the tap count."""
    with np.errstate(all="raise"):
        return (_table_bicubic, _table_aa)[_mode(mode)](int(n_in), int(n_out))


def apply_tables(grid: np.ndarray, ty, tx) -> np.ndarray:
    """grid [h][w][D] fp32 -> [len(ty)][len(tx)][D]: per output the rows of the taps first (along x), then their sum along y; every
    accumulator starts at 0.0f, taps in order, multiply then add, each rounded (vectorised over D only)."""
    grid = np.ascontiguousarray(grid, np.float32)
    h, w, D = grid.shape
    out = np.empty((len(ty), len(tx), D), np.float32)
    for y, (fy, wy) in enumerate(ty):
        for x, (fx, wx) in enumerate(tx):
            acc = np.zeros(D, np.float32)
            for j, wj in enumerate(wy):
                iy = min(max(fy + j, 0), h - 1)
                row = np.zeros(D, np.float32)
                for i, wi in enumerate(wx):
                    ix = min(max(fx + i, 0), w - 1)
                    row = row + wi * grid[iy, ix]
                acc = acc + wj * row
            out[y, x] = acc
    return out


def resample(pos: np.ndarray, g_dst: int, mode) -> np.ndarray:
    """pos [1 + g_src^2][D] -> [1 + g_dst^2][D]; the class row is the input's bits."""
    pos = np.ascontiguousarray(pos, np.float32)
    T, D = pos.shape
    g_src = int(round((T - 1) ** 0.5))
    assert g_src * g_src + 1 == T, "the patch part of pos must be a square grid"
    t = table(mode, g_src, g_dst)
    out = np.empty((1 + g_dst * g_dst, D), np.float32)
    out[0] = pos[0]
    out[1:] = apply_tables(pos[1:].reshape(g_src, g_src, D), t, t).reshape(g_dst * g_dst, D)
    return out
