"""vithip_dense_depth_f32 (csrc/vit_depth.hip) on the GPU against the upstream order in float64 (tests/depth_head_model.py).

The bar of a case is max |got - ref| <= max(4 * E32, 2^-22 * max_depth), E32 the distance of a numpy fp32 restatement of the header's
arithmetic from the same float64 reference -- taken from the reference side, never from the kernel.  Every case runs with and without
the class token's bias, with padded logit rows and image strides, and with its output inside a sentinel-filled frame.
"""
import functools

import numpy as np
import pytest

import depth_head_model as M
import strided
from vit_amd import binding as B

pytestmark = pytest.mark.gpu

# g, bins, u, (out_h, out_w), images
CASES = [(4, 2, 1, (4, 4), 2),          # both resizes are identities
         (1, 7, 8, (5, 3), 2),          # a single cell
         (3, 256, 4, (37, 53), 3),      # odd grid, full bins, non-square output
         (5, 255, 3, (7, 9), 2),        # odd u, bins no multiple of 4, stage 2 shrinks
         (16, 256, 4, (224, 224), 3),   # the ViT-S/B/L-14 shape at 224
         (37, 64, 4, (148, 148), 2)]    # the 518 grid, stage 2 identity, the largest window
MIN_DEPTH, MAX_DEPTH = 0.001, 10.0


@functools.lru_cache(maxsize=None)
def case(g, bins, u, out, n, with_cls):
    """(logits, z or None, centres, float64 reference, E32, bar), computed once."""
    rng = np.random.default_rng(g * 1000 + bins * 7 + u)
    logits = (3 * rng.standard_normal((n, g * g, bins))).astype(np.float32)
    logits[0] = -10 - np.abs(logits[0])                    # all negative: s = 0.1 * bins, the depth is the mean of the centres
    logits[1, :, bins // 3] = 50                           # one dominant bin in every cell
    z = rng.standard_normal((n, bins)).astype(np.float32) if with_cls else None
    centres = np.linspace(MIN_DEPTH, MAX_DEPTH, bins).astype(np.float32)
    cell = logits + z[:, None] if with_cls else logits
    ref = M.reference64(cell, centres, g, u, out, MIN_DEPTH, MAX_DEPTH)
    e32, bar = M.bar(ref, cell, centres, g, u, out, MIN_DEPTH, MAX_DEPTH)
    assert np.abs(ref[0] - centres.astype(np.float64).mean()).max() < 1e-12
    return logits, z, centres, ref, e32, bar


@pytest.mark.parametrize("with_cls", [False, True])
@pytest.mark.parametrize("g,bins,u,out,n", CASES)
def test_depth_matches_float64_within_the_fp32_bar_and_writes_nothing_else(g, bins, u, out, n, with_cls):
    logits, z, centres, ref, e32, bar = case(g, bins, u, out, n, with_cls)
    frames = {}
    got = B.dense_depth(logits, centres, u, *out, cls_logits=z, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, ld_logits=bins + 3,
                        image_rows=g * g + 2, out_ld=out[0] * out[1] + 5, pad_value=1e30, frames=strided, out=frames)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"g={g} bins={bins} u={u} out={out} cls={with_cls}: max |got - ref| = {err:.3e}, E32 = {e32:.3e}, bar = {bar:.3e}")
    assert got.dtype == np.float32 and np.isfinite(got).all() and err <= bar, (err, e32, bar)
    frames["depth"].assert_untouched()
    frames["logits"].assert_untouched()
