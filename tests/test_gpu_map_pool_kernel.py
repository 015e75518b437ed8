"""vithip_map_pool_f32 and vithip_gelu_tanh_rows_f32 (csrc/vit_map_head.hip) against float64.

The pooling against concat_h(Wv_h z_h + bv_h) of the float64 LayerNorm rows at the fp32 op bar of tests/test_gpu_ops.py (REL = 2e-5 of
max |ref|), and bitwise where the contract says so.  x as tests/test_gpu_pool_layernorm_kernel.py draws it (pattern + noise); the
folded queries N(0, c^2 / dim): c = 2 is a spread softmax, c = 40 a nearly one-hot one with |scores| of order 100, where an
exponential without its maximum subtraction overflows.
"""
import numpy as np
import pytest

import strided
from engine_helpers import same_bits
from test_gpu_pool_layernorm_kernel import operands
from test_gpu_quickgelu_gemm import sweep
from vit_amd import binding as B

pytestmark = pytest.mark.gpu

REL = 2e-5  # tests/test_gpu_ops.py
TS = 64     # key rows per segment (MAP_TS in csrc/vit_map_head.hip)
KEYS = [1, 2, TS - 1, TS, TS + 1, 50, 196, 257, 729]
SHAPES = [(64, 1), (192, 3), (768, 12), (1024, 32), (1152, 16), (2048, 16)]  # every register variant, heads that pad, hd = 72
HIP_INVALID_VALUE = 1


def head_operands(dim, heads, c, seed):
    rng = np.random.default_rng(seed)
    a = rng.normal(0.0, c / np.sqrt(dim), (heads, dim)).astype(np.float32)
    wv = rng.normal(0.0, 1.0 / np.sqrt(dim), (dim, dim)).astype(np.float32)
    return a, wv, rng.uniform(-0.5, 0.5, dim).astype(np.float32)


def reference(x, gamma, beta, a, wv, bv, images, tokens, first_tok):
    x64 = np.asarray(x, np.float64).reshape(images, tokens, -1)[:, first_tok:]
    y = (x64 - x64.mean(-1, keepdims=True)) / np.sqrt(x64.var(-1, keepdims=True) + 1e-6) * gamma.astype(np.float64) + beta.astype(np.float64)
    heads, dim = a.shape
    s = np.einsum("ntd,hd->nht", y, a.astype(np.float64))
    p = np.exp(s - s.max(-1, keepdims=True))
    z = np.einsum("nht,ntd->nhd", p / p.sum(-1, keepdims=True), y)
    out = np.einsum("nhd,hjd->nhj", z, wv.astype(np.float64).reshape(heads, dim // heads, dim))
    return out.reshape(images, dim) + bv.astype(np.float64)


def close(got, ref, what):
    err, scale = float(np.abs(got.astype(np.float64) - ref).max()), float(np.abs(ref).max())
    print(f"{what}: max |d| = {err:.3e}, max |ref| = {scale:.3e}, ratio {err / scale:.2e}")
    assert np.isfinite(got).all(), what
    assert err <= REL * scale, what


@pytest.mark.parametrize("dim,heads", SHAPES)
@pytest.mark.parametrize("keys", KEYS)
def test_matches_float64(keys, dim, heads):
    for first_tok, images, c in ((0, 1, 2.0), (1, 3, 40.0), (5, 1, 40.0), (5, 3, 2.0), (0, 3, 40.0), (1, 1, 2.0)):
        tokens = keys + first_tok
        x, gamma, beta = operands(images, tokens, dim, seed=keys + dim + first_tok)
        a, wv, bv = head_operands(dim, heads, c, seed=dim + heads)
        got = B.map_pool(x, gamma, beta, a, wv, bv, images, tokens, first_tok)
        close(got, reference(x, gamma, beta, a, wv, bv, images, tokens, first_tok), f"{(images, tokens, first_tok, dim, heads)} c={c}")
        if keys == 1:  # one key: the softmax is 1, out = Wv y_0 + bv
            y0 = reference(x, gamma, beta, np.zeros_like(a), wv, bv, images, tokens, first_tok)
            close(got, y0, "one key")


@pytest.mark.parametrize("tokens,dim,heads", [(2, 64, 1), (66, 192, 3), (197, 768, 12), (130, 1024, 32), (50, 2048, 16)])
def test_an_image_has_the_same_bits_alone_and_at_every_place_of_a_batch(tokens, dim, heads):
    images = 5
    x, gamma, beta = operands(images, tokens, dim, seed=11 + tokens)
    a, wv, bv = head_operands(dim, heads, 8.0, seed=tokens)
    x = x.reshape(images, tokens, dim)
    alone = B.map_pool(x[0], gamma, beta, a, wv, bv, 1, tokens)
    for place in (0, images // 2, images - 1):
        order = list(range(1, images))
        order.insert(place, 0)
        batch = B.map_pool(x[order].reshape(images * tokens, dim), gamma, beta, a, wv, bv, images, tokens)
        assert same_bits(batch[place], alone[0]), place


@pytest.mark.parametrize("tokens,dim,heads", [(2, 64, 1), (17, 192, 3), (197, 768, 12), (66, 1024, 32), (18, 2048, 16)])
def test_padding_changes_nothing_and_only_the_output_rows_and_the_workspace_are_written(tokens, dim, heads):
    images = 3
    x, gamma, beta = operands(images, tokens, dim, seed=7 + dim)
    a, wv, bv = head_operands(dim, heads, 4.0, seed=dim)
    dense = B.map_pool(x, gamma, beta, a, wv, bv, images, tokens)
    frames = {}
    got = B.map_pool(x, gamma, beta, a, wv, bv, images, tokens, 1, ldx=dim + 12, ldo=dim + 8, frames=strided, out=frames)
    assert same_bits(got, dense)
    assert same_bits(frames["out"].check(), dense)  # nothing outside [images][dim] changed, every element inside was written
    hp = 16 if heads <= 16 else 32
    groups = -(-dim // (256 // hp))                  # the folded queries: four instructions of 64 / hp columns each per group
    assert frames["ws"].shape == (1, groups * 256 + images * -(-(tokens - 1) // TS) * (2 * hp + heads * dim))
    frames["ws"].assert_untouched()


@pytest.mark.parametrize("tokens,dim,heads", [(2, 64, 1), (70, 192, 3), (197, 768, 12), (50, 2048, 16)])
def test_a_nan_row_poisons_only_its_own_image(tokens, dim, heads):
    images = 3
    x, gamma, beta = operands(images, tokens, dim, seed=13 + tokens)
    a, wv, bv = head_operands(dim, heads, 4.0, seed=3)
    clean = B.map_pool(x, gamma, beta, a, wv, bv, images, tokens)
    x[1 * tokens + tokens - 1, dim // 2] = np.nan  # one element of the last key of the middle image
    got = B.map_pool(x, gamma, beta, a, wv, bv, images, tokens)
    assert np.isnan(got[1]).all() and same_bits(got[[0, 2]], clean[[0, 2]])
    x[1 * tokens] = np.nan  # a row in front of first_tok is no key
    x[1 * tokens + tokens - 1, dim // 2] = 0.5
    assert np.isfinite(B.map_pool(x, gamma, beta, a, wv, bv, images, tokens, 1)).all()


def test_every_refusal_is_invalid_value_and_leaves_out_untouched():
    images, tokens, dim, heads = 2, 5, 128, 4
    x, gamma, beta = operands(images, tokens, dim, seed=29)
    a, wv, bv = head_operands(dim, heads, 2.0, seed=1)
    dg = B.DeviceArray.from_numpy(gamma)
    bads = [dict(x=None), dict(out=None), dict(gamma=None), dict(beta=None), dict(a=None), dict(wv=None), dict(bv=None), dict(workspace=None),
            dict(images=0), dict(tokens=1), dict(first_tok=-1), dict(first_tok=tokens), dict(dim=0), dict(dim=126), dict(dim=2052),
            dict(heads=0), dict(heads=33), dict(heads=3), dict(ldx=dim - 4), dict(ldx=dim + 2), dict(ldo=dim - 4), dict(ldo=dim + 2),
            dict(eps=0.0), dict(gamma=dg.ptr + 4), dict(a=dg.ptr + 8), dict(workspace=dg.ptr + 4)]
    for bad in bads:
        frames = {}
        with pytest.raises(B.VitError) as err:
            B.map_pool(x, gamma, beta, a, wv, bv, images, tokens, 1, frames=strided, out=frames, override=bad)
        assert err.value.code == HIP_INVALID_VALUE, bad
        if "out" not in bad:
            assert (strided.as_bits(frames["out"].window()) == strided.SENTINEL[np.dtype(np.float32)]).all(), bad
            frames["out"].assert_untouched()
        frames["ws"].assert_untouched()
    frames = {}
    with pytest.raises(B.VitError) as err:  # an output base that is only element-aligned
        B.map_pool(x, gamma, beta, a, wv, bv, images, tokens, 1, frames=strided, out=frames, out_offset=1)
    assert err.value.code == HIP_INVALID_VALUE
    frames["out"].assert_untouched()


def test_gelu_tanh_over_its_range_against_float64():
    """Over [-100, 100] (the sweep of tests/test_gpu_quickgelu_gemm.py), in units of (ulp of the result + 2^-126) against float64, at that
    test's bar: at most twice what PyTorch's CPU fp32 gelu(approximate="tanh") shows on the same inputs."""
    import torch

    xs = sweep()
    xs = xs.reshape(-1, 1024)
    got = B.gelu_tanh_rows(xs).reshape(-1).astype(np.float64)
    x64 = xs.reshape(-1).astype(np.float64)
    with np.errstate(over="ignore"):  # 0.5 x (1 + tanh u) = x sigmoid(2u): the form whose negative tail does not cancel to zero
        ref = x64 / (1.0 + np.exp(-2.0 * np.sqrt(2.0 / np.pi) * (x64 + 0.044715 * x64 ** 3)))
    unit = np.spacing(np.abs(ref.astype(np.float32))).astype(np.float64) + 2.0 ** -126
    pt = torch.nn.functional.gelu(torch.from_numpy(xs.reshape(-1)), approximate="tanh").numpy().astype(np.float64)
    e_kernel, e_torch = np.abs(got - ref) / unit, np.abs(pt - ref) / unit
    print(f"gelu_tanh: kernel max {e_kernel.max():.2f} units at {x64[e_kernel.argmax()]!r}, PyTorch CPU max {e_torch.max():.2f}")
    assert e_kernel.max() <= 2.0 * e_torch.max()
