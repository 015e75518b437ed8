"""The tap contract (vithip_tap_f32, vit_engine_intermediate_*) restated in numpy: the four layouts over rows that something else
has normalised -- pyoracle.layer_norm for the oracle references, the LayerNorm kernel itself for the bitwise kernel test.

Rows come as [images * tokens][dim] (or [images][tokens][dim]); a layout picks and arranges them per image, moving no bit:

    cls      [images][dim]             row 0
    tokens   [images][tokens][dim]     every row, class row first
    patches  [images][tokens-1][dim]   rows 1..
    map      [images][dim][tokens-1]   the transpose of patches: [dim][g][g] for a square grid, raster order
"""
import numpy as np

LAYOUTS = ("cls", "tokens", "patches", "map")


def arrange(rows, images, tokens, layout):
    r = np.asarray(rows).reshape(images, tokens, -1)
    if layout == "cls":
        return r[:, 0].copy()
    if layout == "tokens":
        return r.copy()
    if layout == "patches":
        return r[:, 1:].copy()
    if layout == "map":
        return np.ascontiguousarray(r[:, 1:].transpose(0, 2, 1))
    raise ValueError(layout)


def block_elems(tokens, dim, layout):
    return {"cls": 1, "tokens": tokens, "patches": tokens - 1, "map": tokens - 1}[layout] * dim


def reference(oracle, x, gamma, beta, images, tokens, layout, norm):
    """x [images * tokens][dim] -> the block of every image: the oracle's LayerNorm of the rows (norm) or the rows themselves."""
    x = np.asarray(x, np.float32).reshape(images * tokens, -1)
    rows = oracle.layer_norm(x, gamma, beta) if norm else x
    return arrange(rows, images, tokens, layout)


def intermediate_reference(oracle, stages, layers, final_gamma, final_beta, kind, norm, grid=None):
    """stages: per image the oracle's residual streams (forward_image(..., want_stages=True)[2]: stages[l + 1] is behind encoder
    layer l) -> [n][K] + block; grid = g reshapes a map block to [dim][g][g]."""
    out = []
    for st in stages:
        tokens = st[0].shape[0]
        blocks = [reference(oracle, st[l + 1], final_gamma, final_beta, 1, tokens, kind, norm)[0] for l in layers]
        out.append(np.stack(blocks))
    out = np.stack(out)
    if kind == "map" and grid:
        out = out.reshape(out.shape[:3] + (grid, grid))
    return out
