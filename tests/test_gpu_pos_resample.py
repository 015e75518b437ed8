"""Position-embedding resampling on the device: vithip_pos_resample_f32 against the numpy restatement (tests/pos_resample_model.py) bit
for bit, its write footprint and refusals, and the engine calls built on it -- a checkpoint of one input size loaded into, or copied
between, engines of another.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import pos_resample_model as M
from conftest import oracle_config
from engine_helpers import same_bits
from test_gpu_bf16 import BF16_PROB_TOL
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

MODES = list(M.MODES)
INVALID = 1  # hipErrorInvalidValue
PATTERN = 0x7FC0DEAD  # a quiet NaN no sum of finite products gives
SRC = synth.VIT_SMALL  # 64 px, a 4 x 4 grid
SEED = 31
_cache = {}


def _pos(g_src, dim, seed=0):
    return np.random.default_rng(seed + 1000 * g_src + dim).uniform(-1.0, 1.0, (1 + g_src * g_src, dim)).astype(np.float32)


def _model(pos, g_dst, mode):
    key = ("model", pos.tobytes(), pos.shape, g_dst, mode)
    if key not in _cache:
        _cache[key] = M.resample(pos, g_dst, mode)
    return _cache[key]


# ---- 1: the kernel ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("g_src,g_dst,dim", [(2, 3, 32), (14, 24, 64), (14, 16, 36), (24, 14, 64), (8, 5, 132), (1, 4, 4), (4, 1, 4),
                                             (7, 7, 128), (14, 32, 2048)])
def test_kernel_gives_the_bits_of_the_model_and_writes_dst_exactly(g_src, g_dst, dim, mode):
    pos = _pos(g_src, dim)
    raw = {}
    got = B.pos_resample(pos, g_dst, mode, guard=64, fill_bits=PATTERN, out=raw)
    want = _model(pos, g_dst, mode)
    assert same_bits(got, want)
    assert same_bits(got[0], pos[0])  # the class row
    if g_src == g_dst:
        assert same_bits(got, pos)
    bits = raw["raw"].view(np.uint32)
    assert bits.size == 128 + want.size
    assert (bits[:64] == PATTERN).all() and (bits[-64:] == PATTERN).all()  # the guards either side
    assert not (bits[64:-64] == PATTERN).any()                                # every element of dst was written


def test_refused_arguments_launch_nothing_and_leave_the_launcher_usable():
    L = B.lib()
    pos = _pos(4, 8)
    d_src = B.DeviceArray.from_numpy(pos)
    d_dst = B.DeviceArray.from_numpy(np.full(2 + 10 * 8, PATTERN, np.uint32).view(np.float32))

    def call(src=None, g_src=4, dst=None, g_dst=3, dim=8, mode=0):
        return L.vithip_pos_resample_f32(None, d_src.ptr if src is None else src, g_src, d_dst.ptr if dst is None else dst, g_dst, dim, mode)

    cases = {"dim 6": dict(dim=6), "dim 0": dict(dim=0), "dim 2052": dict(dim=2052), "source grid 0": dict(g_src=0),
             "source grid 257": dict(g_src=257), "grid 0": dict(g_dst=0), "grid 257": dict(g_dst=257), "mode 2": dict(mode=2),
             "mode -1": dict(mode=-1), "misaligned dst": dict(dst=d_dst.ptr + 4), "misaligned src": dict(src=d_src.ptr + 8),
             "null src": dict(src=0), "null dst": dict(dst=0)}
    for name, kw in cases.items():
        assert call(**kw) == INVALID, name
        assert (d_dst.numpy().view(np.uint32) == PATTERN).all(), name  # nothing was launched
        for mode in MODES:  # a valid call behind every refusal
            assert call(mode=M.MODES[mode]) == 0, (name, mode)
            assert same_bits(d_dst.numpy()[:10 * 8].reshape(10, 8), _model(pos, 3, mode)), (name, mode)
        B.hip_check(L.vithip_memcpy_h2d(d_dst.ptr, np.full(82, PATTERN, np.uint32).ctypes.data, 82 * 4, None), "h2d")
        B.hip_check(L.vithip_device_sync(), "sync")
    for kw in (dict(g_dst=0), dict(g_dst=257), dict(mode=2), dict(g_src=0), dict(dst_offset=1)):  # the wrapper reports the code
        with pytest.raises(B.VitError) as err:
            B.pos_resample(pos, kw.pop("g_dst", 3), kw.pop("mode", 0), **kw)
        assert err.value.code == INVALID, kw


# ---- 2: the engine ------------------------------------------------------------------------------------------------------------

def _cfg(size):
    return dataclasses.replace(SRC, img_size=size)


def _w_src():
    if "w_src" not in _cache:
        _cache["w_src"] = synth.make_weights(SRC, SEED)
    return _cache["w_src"]


def _w_dst(size, mode):
    """The 64-px weights with tensor 3 exchanged for the model's resampling to `size`."""
    key = ("w_dst", size, mode)
    if key not in _cache:
        W = list(_w_src())
        W[3] = _model(np.ascontiguousarray(W[3], np.float32).reshape(SRC.tokens, SRC.embed_dim), size // SRC.patch_size, mode)
        _cache[key] = W
    return _cache[key]


def _images(size, n=3):
    key = ("images", size, n)
    if key not in _cache:
        _cache[key] = synth.make_images(_cfg(size), n, 500 + size)
    return _cache[key]


def _outputs(eng, imgs):
    return {"forward": eng.forward(imgs), "features": eng.features(imgs, "mean"), "attention": eng.cls_attention(imgs, "heads"),
            "map": eng.intermediate(imgs, [0, eng.cfg.depth - 1], kind="map")}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", [96, 32, 256])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_engine_resamples_on_load_to_the_bits_of_weights_resampled_by_the_model(oracle, dtype, size, mode):
    cfg = _cfg(size)
    assert cfg.tokens == {96: 37, 32: 5, 256: 257}[size]
    imgs = _images(size)
    a, b = B.Engine(cfg, max_batch=2, dtype=dtype), B.Engine(cfg, max_batch=2, dtype=dtype)
    try:
        a.load_weights(_w_src(), pos_from=SRC.img_size, pos_mode=mode)
        b.load_weights(_w_dst(size, mode))
        got, want = _outputs(a, imgs), _outputs(b, imgs)
        for k in want:
            assert same_bits(got[k], want[k]), k
        assert got["map"].shape == (3, 2, cfg.embed_dim, size // 16, size // 16)  # [n][K][D][g][g] at the engine's own grid
    finally:
        a.close()
        b.close()
    key = ("oracle", size, mode)
    if key not in _cache:
        _cache[key] = oracle.forward(oracle_config(cfg), imgs, _w_dst(size, mode))
    ref = _cache[key]
    err = float(np.abs(got["forward"] - ref).max())
    print(f"{dtype} {size} px {mode}: max |dprob| vs the oracle = {err:.3e}")
    assert err <= (1e-4 if dtype == "f32" else BF16_PROB_TOL)
    if dtype == "bf16":
        assert (got["forward"].argmax(1) == ref.argmax(1)).all()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_same_size_is_the_plain_load_and_the_plain_copy(dtype):
    imgs = _images(64)
    a, b, c, d = (B.Engine(SRC, max_batch=2, dtype=dtype) for _ in range(4))
    try:
        a.load_weights(_w_src())
        want = a.forward(imgs)
        for mode in MODES:
            b.load_weights(_w_src(), pos_from=64, pos_mode=mode)
            assert same_bits(b.forward(imgs), want), mode
            assert same_bits(b.read_weight_image().f32_section(), a.read_weight_image().f32_section()), mode
            c.copy_weights_from(a, pos_mode=mode)
            assert same_bits(c.forward(imgs), want), mode
        d.copy_weights_from(a)
        assert same_bits(d.forward(imgs), want)
        with pytest.raises(B.VitError, match="unknown mode"):
            c.copy_weights_from(a, pos_mode=5)
        assert same_bits(c.forward(imgs), want)
    finally:
        for e in (a, b, c, d):
            e.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_weight_image_of_a_resampled_engine_loads_into_a_fresh_one(dtype, mode):
    cfg, imgs = _cfg(96), _images(96)
    a, b = B.Engine(cfg, max_batch=2, dtype=dtype), B.Engine(cfg, max_batch=2, dtype=dtype)
    try:
        a.load_weights(_w_src(), pos_from=64, pos_mode=mode)
        img = a.read_weight_image()
        pos = np.asarray(img.tensors()[3], np.float32).reshape(cfg.tokens, cfg.embed_dim)
        assert same_bits(pos, _w_dst(96, mode)[3])  # the image holds the resampled tensor, for the engine's own configuration
        b.load_weight_image(img)
        assert same_bits(b.forward(imgs), a.forward(imgs))
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_copy_across_resolutions_is_a_load_with_pos_from(dtype, mode):
    cfg, imgs = _cfg(96), _images(96)
    src, a, b = B.Engine(SRC, max_batch=2, dtype=dtype), B.Engine(cfg, max_batch=2, dtype=dtype), B.Engine(cfg, max_batch=2, dtype=dtype)
    other = B.Engine(dataclasses.replace(cfg, num_classes=10), max_batch=2, dtype=dtype)
    try:
        src.load_weights(_w_src())
        before = src.forward(_images(64))
        a.copy_weights_from(src, pos_mode=mode)
        b.load_weights(_w_src(), pos_from=64, pos_mode=mode)
        assert same_bits(a.forward(imgs), b.forward(imgs))
        assert same_bits(a.read_weight_image().f32_section(), b.read_weight_image().f32_section())
        assert same_bits(src.forward(_images(64)), before)  # the source is read, not changed
        with pytest.raises(B.VitError, match="differ"):  # a plain copy still wants equal configurations
            a.copy_weights_from(src)
        with pytest.raises(B.VitError, match="differ in more than img_size"):
            other.copy_weights_from(src, pos_mode=mode)
        assert same_bits(a.forward(imgs), b.forward(imgs))
    finally:
        for e in (src, a, b, other):
            e.close()


@pytest.mark.parametrize("use_graph", [False, True])
def test_refused_loads_leave_the_engine_and_its_graph_usable(use_graph):
    cfg, n = _cfg(96), 2
    imgs = _images(96)[:n]
    eng, fresh = B.Engine(cfg, max_batch=2, use_graph=use_graph), B.Engine(cfg, max_batch=2)
    d_images, d_probs = B.DeviceArray.from_numpy(imgs), B.DeviceArray((n, cfg.num_classes))
    L = B.lib()

    def forward():
        eng.forward_device(d_images.ptr, n, d_probs.ptr)  # on the engine's own stream: captured and replayed with use_graph
        eng.sync()
        return d_probs.numpy()

    def load(weights, size, mode, reserved=0, rs=True):
        arr, keep = B.networks_from(weights)
        spec = B.CPosResample(size, mode, reserved)
        rc = L.vit_engine_load_weights_resampled(eng._h, arr, len(weights), C.byref(spec) if rs else None)
        return rc, L.vit_engine_last_error(eng._h).decode()

    try:
        eng.load_weights(_w_src(), pos_from=64, pos_mode="bicubic")
        want = forward()
        assert same_bits(forward(), want)  # with use_graph: the replay
        ARG, WEIGHTS = 1, 2  # VIT_ERR_*
        native = _w_dst(96, "bicubic")  # tensor 3 for 96 px: the wrong size for a checkpoint said to be of 64 px
        rc, msg = load(native, 64, 0)
        assert rc == WEIGHTS and str(37 * 192) in msg and str(17 * 192) in msg and "4 x 4" in msg and "6 x 6" in msg, msg
        assert same_bits(forward(), want)
        for what, args in {"reserved": (_w_src(), 64, 0, 1), "mode": (_w_src(), 64, 7), "size": (_w_src(), 72, 0), "zero": (_w_src(), 0, 0),
                           "negative": (_w_src(), -64, 0)}.items():
            rc, msg = load(*args)
            assert rc == ARG and msg, what
            assert same_bits(forward(), want), what
        rc, msg = load(_w_src(), 64, 0, rs=False)
        assert rc == ARG
        rc, msg = load(_w_src()[:-1], 64, 0)
        assert rc == WEIGHTS
        assert same_bits(forward(), want)
        # an accepted load replaces the weights, and with them whatever was captured for the old ones
        rc, msg = load(_w_src(), 64, 1)
        assert rc == 0, msg
        fresh.load_weights(_w_dst(96, "bicubic_aa"))
        assert same_bits(forward(), fresh.forward(imgs))
        assert not same_bits(forward(), want)
    finally:
        eng.close()
        fresh.close()
