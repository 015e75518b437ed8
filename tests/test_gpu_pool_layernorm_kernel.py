"""vithip_pool_layernorm_f32 (csrc/vit_pool.hip): the mean over tokens first, the LayerNorm of the pooled row behind it.

Against float64 within the fp32 op bar of tests/test_gpu_ops.py (REL = 2e-5 of the tensor's magnitude), and bitwise where the
contract says so: the fused call is vithip_layernorm_f32 of the stored pooled mean, an image's row does not depend on the batch it
sits in or on x's padding, and nothing but out[images][dim] and the declared workspace is written.

Inputs: a per-channel pattern of spread 1 plus noise of spread 1 -- the pooled row keeps a spread near 1 whatever the token count,
so the LayerNorm behind it does not amplify the pooling's rounding (a mean of pure noise shrinks with 1 / sqrt(tokens) and 1 / std
would scale its rounding up by as much).
"""
import numpy as np
import pytest

import strided
from engine_helpers import same_bits
from vit_amd import binding as B

pytestmark = pytest.mark.gpu

REL = 2e-5  # tests/test_gpu_ops.py
TOKENS = [2, 17, 18, 50, 197, 257]   # one patch behind a class row; exactly one segment; a full segment and one row; ragged ones
DIMS = [64, 192, 512, 768, 1024, 2048]  # every variant of the kernels: 1, 1, 2, 3, 4, 8 float4 per lane
HIP_INVALID_VALUE = 1


def operands(images, tokens, dim, seed):
    rng = np.random.default_rng(seed)
    pattern = rng.normal(0.0, 1.0, dim)
    x = (pattern[None, :] + rng.normal(0.0, 1.0, (images * tokens, dim))).astype(np.float32)
    gamma = rng.uniform(0.5, 1.5, dim).astype(np.float32)
    beta = rng.uniform(-0.5, 0.5, dim).astype(np.float32)
    return x, gamma, beta


def reference(x, gamma, beta, images, tokens, first_tok):
    """(pooled mean, its LayerNorm) in float64."""
    x64 = np.asarray(x, np.float64).reshape(images, tokens, -1)
    m = x64[:, first_tok:].mean(1)
    mu, var = m.mean(1, keepdims=True), m.var(1, keepdims=True)
    return m, (m - mu) / np.sqrt(var + 1e-6) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)


def close(got, ref, what):
    err, scale = float(np.abs(got.astype(np.float64) - ref).max()), float(np.abs(ref).max())
    print(f"{what}: max |d| = {err:.3e}, max |ref| = {scale:.3e}, ratio {err / scale:.2e}")
    assert np.isfinite(got).all(), what
    assert err <= REL * scale, what


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("tokens", TOKENS)
def test_matches_float64_and_is_the_layernorm_of_the_stored_mean(tokens, dim):
    for images in (1, 3):
        for first_tok in (0, 1):
            x, gamma, beta = operands(images, tokens, dim, seed=tokens + dim + images + first_tok)
            ref_m, ref_y = reference(x, gamma, beta, images, tokens, first_tok)
            what = f"{(images, tokens, dim)} first_tok={first_tok}"
            mean = B.pool_layernorm(x, None, None, images, tokens, first_tok)
            fused = B.pool_layernorm(x, gamma, beta, images, tokens, first_tok)
            assert mean.shape == fused.shape == (images, dim)
            close(mean, ref_m, what + " mean")
            close(fused, ref_y, what + " layernorm")
            assert same_bits(fused, B.layernorm(mean, gamma, beta)), what


@pytest.mark.parametrize("tokens,dim", [(2, 64), (17, 192), (18, 768), (50, 2048), (197, 768), (257, 1024)])
def test_an_image_has_the_same_bits_alone_and_at_every_place_of_a_batch(tokens, dim):
    images = 5
    x, gamma, beta = operands(images, tokens, dim, seed=11 + tokens)
    x = x.reshape(images, tokens, dim)
    for g, b in ((gamma, beta), (None, None)):
        alone = B.pool_layernorm(x[0], g, b, 1, tokens)
        for place in (0, images // 2, images - 1):
            order = [i for i in range(1, images)]
            order.insert(place, 0)
            batch = B.pool_layernorm(x[order].reshape(images * tokens, dim), g, b, images, tokens)
            assert same_bits(batch[place], alone[0]), (place, g is None)


@pytest.mark.parametrize("tokens,dim", [(2, 64), (17, 192), (50, 768), (257, 192), (18, 1024), (18, 2048)])  # frames of a few MB
def test_padding_changes_nothing_and_only_the_output_rows_and_the_workspace_are_written(tokens, dim):
    """x, out and the workspace sit in frames (tests/strided.py): guard rows and pad columns hold a NaN sentinel.  ldx > dim and
    ldo > dim; the pad columns of x are NaN, so a read past dim would show in the result."""
    images = 3
    x, gamma, beta = operands(images, tokens, dim, seed=7 + dim)
    dense = B.pool_layernorm(x, gamma, beta, images, tokens)
    frames = {}
    got = B.pool_layernorm(x, gamma, beta, images, tokens, 1, ldx=dim + 12, ldo=dim + 8, frames=strided, out=frames)
    assert same_bits(got, dense)
    assert same_bits(frames["out"].check(), dense)      # nothing outside [images][dim] changed, every element inside was written
    ws = frames["ws"]
    assert ws.shape == (1, images * -(-(tokens - 1) // 16) * dim)  # exactly the declared floats, between the guards
    ws.assert_untouched()
    frames = {}
    mean = B.pool_layernorm(x, None, None, images, tokens, 0, ldx=dim + 4, ldo=dim + 4, frames=strided, out=frames)
    assert same_bits(mean, B.pool_layernorm(x, None, None, images, tokens, 0))
    frames["out"].check()
    frames["ws"].assert_untouched()


@pytest.mark.parametrize("tokens,dim", [(2, 64), (17, 192), (197, 768), (50, 2048)])
def test_a_nan_row_poisons_only_its_own_image(tokens, dim):
    images = 3
    x, gamma, beta = operands(images, tokens, dim, seed=13 + tokens)
    clean = B.pool_layernorm(x, gamma, beta, images, tokens)
    x[1 * tokens + tokens - 1, dim // 2] = np.nan  # one element of the last token of the middle image
    for g, b in ((gamma, beta), (None, None)):
        got = B.pool_layernorm(x, g, b, images, tokens)
        assert np.isnan(got[1]).any()
        assert np.isfinite(got[[0, 2]]).all()
        if g is not None:
            assert np.isnan(got[1]).all()  # the statistics of the pooled row are NaN
            assert same_bits(got[[0, 2]], clean[[0, 2]])
    x[1 * tokens] = np.nan  # the class row is not pooled (first_tok = 1) ...
    x[1 * tokens + tokens - 1, dim // 2] = 0.5
    assert np.isfinite(B.pool_layernorm(x, gamma, beta, images, tokens, 1)).all()
    assert np.isnan(B.pool_layernorm(x, gamma, beta, images, tokens, 0)[1]).all()  # ... and is with first_tok = 0


def test_a_constant_pooled_row_goes_through_the_epsilon():
    images, tokens, dim = 2, 17, 768
    x, gamma, beta = operands(images, tokens, dim, seed=17)
    x[tokens:] = 1.25  # image 1: every row constant, the pooled row too
    got = B.pool_layernorm(x, gamma, beta, images, tokens)
    assert np.isfinite(got).all()
    assert same_bits(got[1], beta)
    assert same_bits(got, B.layernorm(B.pool_layernorm(x, None, None, images, tokens), gamma, beta))


def test_every_refusal_is_invalid_value_and_leaves_out_untouched():
    images, tokens, dim = 2, 5, 128
    x, gamma, beta = operands(images, tokens, dim, seed=29)
    dg = B.DeviceArray.from_numpy(gamma)
    bads = [dict(x=None), dict(out=None), dict(gamma=None), dict(beta=None), dict(workspace=None), dict(images=0), dict(images=-1),
            dict(tokens=1), dict(first_tok=-1), dict(first_tok=tokens), dict(dim=0), dict(dim=126), dict(dim=2052), dict(ldx=dim - 4),
            dict(ldx=dim + 2), dict(ldo=dim - 4), dict(ldo=dim + 2), dict(gamma=dg.ptr + 4), dict(beta=dg.ptr + 8)]
    for bad in bads:
        frames = {}
        with pytest.raises(B.VitError) as err:
            B.pool_layernorm(x, gamma, beta, images, tokens, 1, frames=strided, out=frames, override=bad)
        assert err.value.code == HIP_INVALID_VALUE, bad
        if "out" not in bad:
            out = frames["out"]
            assert (strided.as_bits(out.window()) == strided.SENTINEL[np.dtype(np.float32)]).all(), bad
            out.assert_untouched()
        frames["ws"].assert_untouched()
    for kw in (dict(out_offset=1), dict(out_offset=2)):  # an output base that is only element-aligned
        frames = {}
        with pytest.raises(B.VitError) as err:
            B.pool_layernorm(x, gamma, beta, images, tokens, 1, frames=strided, out=frames, **kw)
        assert err.value.code == HIP_INVALID_VALUE, kw
        assert (strided.as_bits(frames["out"].window()) == strided.SENTINEL[np.dtype(np.float32)]).all(), kw
        frames["out"].assert_untouched()
    # a misaligned x or workspace, by address
    frames = {}
    B.pool_layernorm(x, gamma, beta, images, tokens, 1, frames=strided, out=frames)
    good = frames["out"].window()
    for name in ("x", "workspace"):
        f2 = {}
        dx = B.DeviceArray.from_numpy(x)
        with pytest.raises(B.VitError) as err:
            B.pool_layernorm(x, gamma, beta, images, tokens, 1, frames=strided, out=f2, override={name: dx.ptr + 4})
        assert err.value.code == HIP_INVALID_VALUE, name
        f2["out"].assert_untouched()
        assert not strided.has_nan(good) and strided.has_sentinel(f2["out"].window())
