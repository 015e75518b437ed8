"""vithip_layernorm_pool_f32 (csrc/vit_pool.hip): LayerNorm + mean over tokens in one pass, and the L2 normalisation of rows.

Against the numpy restatement of the contract (tests/test_features_abi.py pins it to the oracle) within 2e-5 x max |ref| -- the
project's bar for "fp32 accumulation order only" -- and bitwise where the contract says so: an image's row does not depend on
the batch it sits in.
"""
import numpy as np
import pytest

from engine_helpers import same_bits
from test_features_abi import POOL_REL, l2_normalize_f64, pool_reference
from vit_amd import binding as B

pytestmark = pytest.mark.gpu

SHAPES = [(256, 197, 768), (1, 197, 768), (3, 5, 128), (7, 17, 192), (5, 577, 1024), (300, 2, 64), (2, 50, 2048)]


def operands(images, tokens, dim, seed, ldx=None):
    """x [images * tokens][ldx] (columns dim.. are padding the kernel must not read into the result), gamma, beta."""
    rng = np.random.default_rng(seed)
    ldx = dim if ldx is None else ldx
    x = rng.uniform(-1.5, 1.5, size=(images * tokens, ldx)).astype(np.float32)
    if ldx > dim:
        x[:, dim:] = 1e30
    gamma = rng.uniform(0.5, 1.5, size=dim).astype(np.float32)
    beta = rng.uniform(-0.5, 0.5, size=dim).astype(np.float32)
    return x, gamma, beta


def check(got, ref, what):
    err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    print(f"{what}: max |d| = {err:.3e}, max |ref| = {scale:.3e}, ratio {err / scale:.2e}")
    assert np.isfinite(got).all()
    assert err <= POOL_REL * scale, what


@pytest.mark.parametrize("l2", [False, True])
@pytest.mark.parametrize("first_tok", [0, 1])
@pytest.mark.parametrize("images,tokens,dim", SHAPES)
def test_pool_matches_the_restatement(images, tokens, dim, first_tok, l2):
    x, gamma, beta = operands(images, tokens, dim, seed=images + tokens + dim)
    got = B.layernorm_pool(x, gamma, beta, images, tokens, first_tok, l2)
    check(got, pool_reference(x, gamma, beta, images, tokens, first_tok, l2), f"{(images, tokens, dim)} first_tok={first_tok} l2={l2}")


@pytest.mark.parametrize("images,tokens,dim", SHAPES)
def test_pool_takes_a_padded_leading_dimension(images, tokens, dim):
    x, gamma, beta = operands(images, tokens, dim, seed=7 + dim, ldx=dim + 12)
    dense = np.ascontiguousarray(x[:, :dim])
    for l2 in (False, True):
        got = B.layernorm_pool(x, gamma, beta, images, tokens, 1, l2)
        check(got, pool_reference(dense, gamma, beta, images, tokens, 1, l2), f"{(images, tokens, dim)} ldx={dim + 12} l2={l2}")
        assert same_bits(got, B.layernorm_pool(dense, gamma, beta, images, tokens, 1, l2))  # the padding changes nothing


@pytest.mark.parametrize("images,tokens,dim", SHAPES)
def test_row_of_a_batch_equals_the_single_image_call_bit_for_bit(images, tokens, dim):
    x, gamma, beta = operands(images, tokens, dim, seed=11 + tokens)
    for l2 in (False, True):
        batch = B.layernorm_pool(x, gamma, beta, images, tokens, 1, l2)
        for i in range(images):
            one = B.layernorm_pool(x[i * tokens:(i + 1) * tokens], gamma, beta, 1, tokens, 1, l2)
            assert same_bits(one[0], batch[i]), (i, l2)


@pytest.mark.parametrize("images,tokens,dim", [(7, 17, 192), (5, 197, 768), (300, 2, 64)])
def test_an_image_of_nans_poisons_exactly_its_own_row(images, tokens, dim):
    x, gamma, beta = operands(images, tokens, dim, seed=13)
    clean = B.layernorm_pool(x, gamma, beta, images, tokens)
    bad = images // 2
    x[bad * tokens:(bad + 1) * tokens] = np.nan
    for l2 in (False, True):
        got = B.layernorm_pool(x, gamma, beta, images, tokens, 1, l2)
        assert np.isnan(got[bad]).all()
        others = np.delete(np.arange(images), bad)
        assert np.isfinite(got[others]).all()
        if not l2:
            assert same_bits(got[others], clean[others])


@pytest.mark.parametrize("images", [1, 5])
@pytest.mark.parametrize("dim", [64, 192, 768, 1024, 1280, 2048])  # NVEC 1, 1, 3, 4, 8, 8
def test_one_pooled_row_is_the_layernorm_row_bit_for_bit(dim, images):
    """The head of csrc/vit_pool.hip: the row statistics are layernorm_f32_kernel's to the bit.  tokens = 2, first_tok = 1 pools
    exactly one row, and gamma = 1, beta = 0 and the division by 1.0f are exact: the output row is (x - mean) * inv_std of token 1.
    vithip_layernorm_f32 takes the same row straight out of x (leading dimension 2 * dim, from element dim on).  Compared as
    floats: the pooled sum starts from +0 and cannot keep the sign of a zero."""
    rng = np.random.default_rng(31 * dim + images)
    x = rng.uniform(-1.5, 1.5, size=(images * 2, dim)).astype(np.float32)
    one, zero = np.ones(dim, np.float32), np.zeros(dim, np.float32)
    pooled = B.layernorm_pool(x, one, zero, images, 2, 1, False)
    dx, dg, db = B.DeviceArray.from_numpy(x), B.DeviceArray.from_numpy(one), B.DeviceArray.from_numpy(zero)
    dy = B.DeviceArray((images, dim))
    B.hip_check(B.lib().vithip_layernorm_f32(None, dx.ptr + 4 * dim, 2 * dim, dy.ptr, dim, dg.ptr, db.ptr, images, dim), "layernorm")
    rows = dy.numpy()
    print(f"dim {dim}, images {images}: {int((pooled != rows).sum())} of {rows.size} elements differ")
    assert np.isfinite(rows).all() and rows.any()
    assert (pooled == rows).all()


def test_constant_rows_go_through_the_epsilon():
    """var == 0 (tests/test_gpu_ops.py::test_layernorm_constant_row_uses_eps for the plain kernel): x - mean is 0 and the epsilon
    keeps inv_std finite, so a constant row contributes beta's share and nothing else."""
    images, tokens, dim = 3, 17, 768
    x, gamma, beta = operands(images, tokens, dim, seed=17)
    x[tokens + 3] = 1.25      # one constant row inside image 1
    x[2 * tokens:] = 1.25     # image 2: every row constant
    got = B.layernorm_pool(x, gamma, beta, images, tokens)
    check(got, pool_reference(x, gamma, beta, images, tokens), "constant rows")
    assert same_bits(got[2], beta)


def test_l2_of_an_all_zero_pooled_row_is_zero_not_nan():
    images, tokens, dim = 2, 9, 128
    x, gamma, _ = operands(images, tokens, dim, seed=19)
    x[tokens:] = -3.0         # image 1: constant rows, beta = 0: the pooled row is exactly zero
    zero = np.zeros(dim, np.float32)
    got = B.layernorm_pool(x, gamma, zero, images, tokens, 1, True)
    assert np.isfinite(got).all()
    assert not got[1].any()
    assert abs(float(np.sqrt((got[0].astype(np.float64) ** 2).sum())) - 1.0) <= 1e-5


def test_l2_rows_kernel_matches_float64_and_is_independent_of_the_row_count():
    rng = np.random.default_rng(23)
    for rows, dim in [(1, 64), (5, 768), (33, 2048), (256, 192)]:
        x = rng.normal(0, 3.0, size=(rows, dim)).astype(np.float32)
        x[rows // 2] = 0.0
        got = B.l2_normalize_rows(x)
        assert float(np.abs(got - l2_normalize_f64(x)).max()) <= 1e-5  # elements <= 1: a handful of fp32 roundings
        assert not got[rows // 2].any()
        for i in (0, rows - 1):
            assert same_bits(B.l2_normalize_rows(x[i:i + 1])[0], got[i])


def test_launcher_refuses_bad_arguments():
    L = B.lib()
    images, tokens, dim = 2, 5, 128
    x, gamma, beta = operands(images, tokens, dim, seed=29)
    dx, dg, db = B.DeviceArray.from_numpy(x), B.DeviceArray.from_numpy(gamma), B.DeviceArray.from_numpy(beta)
    do, ws = B.DeviceArray((images, dim)), B.DeviceArray((images * tokens * dim,))
    ok = dict(x=dx.ptr, ldx=dim, out=do.ptr, ldo=dim, g=dg.ptr, b=db.ptr, images=images, tokens=tokens, first=1, dim=dim, l2=0, ws=ws.ptr)

    def call(**kw):
        a = dict(ok, **kw)
        return L.vithip_layernorm_pool_f32(None, a["x"], a["ldx"], a["out"], a["ldo"], a["g"], a["b"], a["images"], a["tokens"],
                                           a["first"], a["dim"], a["l2"], a["ws"])

    assert call() == 0
    want = B.DeviceArray.numpy(do)
    for bad in [dict(x=None), dict(out=None), dict(g=None), dict(b=None), dict(ws=None), dict(images=0), dict(tokens=1),
                dict(first=-1), dict(first=tokens), dict(dim=126), dict(dim=2052), dict(ldx=dim - 4), dict(ldx=dim + 2),
                dict(ldo=dim - 4), dict(l2=2), dict(x=dx.ptr + 4), dict(out=do.ptr + 8)]:
        assert call(**bad) == 1, bad  # hipErrorInvalidValue, nothing launched
    assert same_bits(do.numpy(), want)
