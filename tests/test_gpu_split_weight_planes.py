"""Pre-split weight images (vithip_split3_weights_f32, vithip_gemm_args.w_split): the persistent split walk that
stages W's pieces from the image and splits only A must give the bits of the walk that splits both on the fly -- every epilogue,
the hand-over, tiles 0 and 9, the four ViT-B/16 shapes at the metric batch, ragged N and M, hard operands -- and the engine, which
builds the images on upload, must give the bits of an engine held to the on-the-fly kernel (gemm_tile = 10).
The kernel these tests compare with (tile = 10, arith = ARITH_SPLIT3) is itself held to float64 and to a bit-exact host model in
tests/test_gpu_split_gemm_accuracy.py."""
import numpy as np
import pytest

from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

S = B.ARITH_SPLIT3


def u(k, shape, a, seed=4242):
    n = int(np.prod(shape))
    return synth.uniform(seed, k, n, -a, a).reshape(shape)


def hard(k, shape, a):
    """Uniform values over many binades, with subnormals and large magnitudes sprinkled in."""
    rng = np.random.default_rng(k)
    x = (u(k, shape, a) * np.exp2(rng.integers(-20, 8, shape))).astype(np.float32)
    flat = x.reshape(-1)
    pick, n = rng.permutation(flat.size), flat.size // 64
    flat[pick[:n]] = (rng.uniform(-1, 1, n) * 1e-39).astype(np.float32)        # subnormal
    flat[pick[n:2 * n]] = (rng.uniform(-1, 1, n) * 1e12).astype(np.float32)
    return x


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def rne_bf16(x):
    """float32 -> bf16 bit pattern, round to nearest even (finite values)."""
    v = x.view(np.uint32).astype(np.uint64)
    return ((v + 0x7FFF + ((v >> 16) & 1)) >> 16).astype(np.uint16)


def test_image_holds_the_pieces_in_its_layout():
    """The image against a numpy restatement of the pieces (normal values; the subnormals, Inf and NaN are held to the on-the-fly
    split's bits below)."""
    N, K = 200, 96   # a partial last panel: rows 200..255 are zero
    rng = np.random.default_rng(1)
    W = (u(1, (N, K), 1.0) * np.exp2(rng.integers(-20, 40, (N, K)))).astype(np.float32)
    img = B.split3_weights(W)
    assert img.shape == ((N + 127) // 128, K // 16, 3, 128, 16)
    planes = np.zeros((3, img.shape[0] * 128, K), np.uint16)
    for p in range(img.shape[0]):
        for s in range(K // 16):
            planes[:, p * 128:(p + 1) * 128, s * 16:(s + 1) * 16] = img[p, s]
    assert not planes[:, N:].any()
    x = W.copy()
    for piece in range(3):
        want = rne_bf16(x)
        assert np.array_equal(planes[piece, :N], want), piece
        x = (x - (want.astype(np.uint32) << 16).view(np.float32)).astype(np.float32)   # exact remainders
    assert not x.any()
    total = sum((planes[p, :N].astype(np.uint32) << 16).view(np.float32).astype(np.float64) for p in range(3))
    assert np.array_equal(total, W.astype(np.float64))   # hi + mid + lo == W exactly


def test_image_of_inf_nan_and_subnormals_gives_the_bits_of_the_on_the_fly_split():
    M, N, K = 515, 200, 96
    A, W, b = hard(2, (M, K), 1.0), hard(3, (N, K), 0.1), u(4, (N,), 0.1)
    W[5, 7], W[17, 40], W[130, 3], W[199, 95] = np.inf, -np.inf, np.nan, np.float32(1e-45)
    for tile in (9, 0, 10, 11):
        ref = B.gemm(A, W, b, tile=tile, arith=S)
        got = B.gemm(A, W, b, tile=tile, arith=S, w_split=True)
        assert np.array_equal(bits(got), bits(ref)), tile
    assert np.isnan(ref[:, 130]).all() and np.isnan(ref[:, 5]).all()


def fold_rows(k, M):
    rng = np.random.default_rng(k)
    return np.stack([rng.uniform(0.5, 1.5, M), rng.uniform(-1, 1, M)], 1).astype(np.float32)


# (epilogue, residual, fold consumer, row statistics)
EPILOGUES = [("bias", B.EPI_BIAS, False, False, False), ("gelu", B.EPI_BIAS_GELU, False, False, False),
             ("residual", B.EPI_BIAS_RESIDUAL, True, False, False), ("residual+stats", B.EPI_BIAS_RESIDUAL, True, False, True),
             ("fold", B.EPI_BIAS, False, True, False), ("fold+gelu", B.EPI_BIAS_GELU, False, True, False)]


@pytest.mark.parametrize("name,epi,res,fold,stats", EPILOGUES)
@pytest.mark.parametrize("M,N", [(128 * 100 + 77, 768), (128 * 40 + 1, 320)])
def test_every_epilogue_of_the_walk_gives_the_same_bits(name, epi, res, fold, stats, M, N):
    K = 256
    A, W, b = hard(10, (M, K), 1.0), hard(11, (N, K), 0.05), u(12, (N,), 0.1)
    R = u(13, (M, N), 2.0) if res else None
    ln = (fold_rows(14, M), None) if fold else None   # the centred weight: nothing to subtract
    for tile in (9, 0):
        outs = []
        for img in (False, True):
            rs = {} if stats else None
            outs.append((B.gemm(A, W, b, residual=R, epilogue=epi, tile=tile, ln=ln, row_stats=rs, arith=S, w_split=img), rs))
        (ref, rs0), (got, rs1) = outs
        assert np.array_equal(bits(got), bits(ref)), (name, tile)
        if stats:
            assert np.array_equal(bits(rs1["rows"]), bits(rs0["rows"])), (name, tile)


@pytest.mark.parametrize("epi", [B.EPI_BIAS_GELU, B.EPI_BIAS_RESIDUAL])
def test_helper_pieces_with_the_image_give_the_same_bits(epi):
    """600 tiles on 512 workgroups: the hand-over on time and late (handover_test = 1)."""
    M, N, K = 128 * 100, 768, 768
    A, W, b = hard(20, (M, K), 1.0), u(21, (N, K), 0.05), u(22, (N,), 0.1)
    R = u(23, (M, N), 2.0) if epi == B.EPI_BIAS_RESIDUAL else None
    ref = B.gemm(A, W, b, residual=R, epilogue=epi, tile=10, arith=S)
    for late in (0, 1):
        st = {}
        got = B.gemm(A, W, b, residual=R, epilogue=epi, tile=9, workspace=True, handover_test=late, stats=st, arith=S, w_split=True)
        assert np.array_equal(bits(got), bits(ref)), late
        assert st["taken"] + st["recomputed"] > 0, st


# the four encoder GEMMs of the metric batch (256 images x 197 tokens) as the engine calls them
B16_SHAPES = [("qkv", 2304, 768, B.EPI_BIAS, True), ("out_proj", 768, 768, B.EPI_BIAS_RESIDUAL, False),
              ("fc1", 3072, 768, B.EPI_BIAS_GELU, True), ("fc2", 768, 3072, B.EPI_BIAS_RESIDUAL, False)]


@pytest.mark.parametrize("name,N,K,epi,fold", B16_SHAPES)
def test_vit_b16_shapes_at_the_metric_batch_give_the_same_bits(name, N, K, epi, fold):
    M = 256 * 197
    rng = np.random.default_rng(30)
    A = rng.uniform(-1, 1, (M, K)).astype(np.float32)
    W, b = u(31, (N, K), 0.03), u(32, (N,), 0.1)
    R = rng.uniform(-2, 2, (M, N)).astype(np.float32) if epi == B.EPI_BIAS_RESIDUAL else None
    ln = (fold_rows(33, M), None) if fold else None
    outs = []
    for img in (False, True):
        rs = {} if R is not None else None
        outs.append((B.gemm(A, W, b, residual=R, epilogue=epi, workspace=True, ln=ln, row_stats=rs, arith=S, w_split=img), rs))
    (ref, rs0), (got, rs1) = outs
    assert np.array_equal(bits(got), bits(ref)), name
    if R is not None:
        assert rs0["in_epilogue"] == 1 and np.array_equal(bits(rs1["rows"]), bits(rs0["rows"])), name


def test_bad_shape_is_refused():
    W = u(40, (64, 64), 1.0)
    with pytest.raises(B.VitError):
        B.split3_weights(W[:, :48])   # K % 32 != 0


@pytest.mark.parametrize("n", [256, 131])
def test_engine_with_images_gives_the_bits_of_the_on_the_fly_split(n):
    """Default options (the images, built on upload and on copy_weights_from) against gemm_tile = 10 (the one-tile-per-workgroup
    kernel, which splits W on the fly): the metric batch and an odd batch that still takes the persistent walk."""
    W = synth.make_weights(synth.VIT_B16, 1234)
    imgs = synth.make_images(synth.VIT_B16, n, 77)
    eng = B.Engine(synth.VIT_B16, max_batch=n)
    ref_eng = B.Engine(synth.VIT_B16, max_batch=n, gemm_tile=10)
    try:
        eng.load_weights(W)
        ref_eng.copy_weights_from(eng)
        d_in = B.DeviceArray.from_numpy(imgs)
        outs = []
        for e in (eng, ref_eng):
            d_out = B.DeviceArray((n, 1000))
            e.forward_device(d_in.ptr, n, d_out.ptr)
            e.sync()
            outs.append(d_out.numpy())
    finally:
        eng.close()
        ref_eng.close()
    assert np.array_equal(bits(outs[0]), bits(outs[1]))
