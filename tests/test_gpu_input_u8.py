"""8-bit HWC input normalised on the device (vithip_images_u8_to_f32, vit_engine_forward_device_u8 / _host_u8).

Every comparison here is bitwise: the kernel against the host restatement of torchvision's arithmetic
(tests/test_input_u8_model.py), and every u8 forward against the fp32 forward of the same images normalised on the host.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from engine_helpers import cfloats, device_forward, engines, same_bits, weights  # noqa: F401 (fixtures)
from test_input_u8_model import normalise_u8
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

VIT_ERR_ARG = 1
CONSTS_A = (B.IMAGENET_MEAN, B.IMAGENET_STD)
CONSTS_B = ((0.5, 0.25, 0.125), (0.3, -0.6, 0.9))


def u8_images(cfg, n, seed, chans=None):
    """Random bytes, plus a row of 0 and a row of 255 in every image."""
    c = cfg.in_chans if chans is None else chans
    imgs = np.random.default_rng(seed).integers(0, 256, size=(n, cfg.img_size, cfg.img_size, c), dtype=np.uint8)
    imgs[:, 0] = 0
    imgs[:, -1] = 255
    return imgs


# ---- the kernel ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chans", [1, 3, 4])
@pytest.mark.parametrize("S", [32, 224])
def test_kernel_matches_the_host_formula(chans, S):
    imgs = np.random.default_rng(chans * 1000 + S).integers(0, 256, size=(5, S, S, chans), dtype=np.uint8)
    imgs[:, 1] = 0
    imgs[:, S // 2] = 255
    for mean, std in [((0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, 0.5)), ((-0.3, 1.5, 0.0, 7.0), (-0.7, 3.0, 1e-3, 2.0))]:
        mean, std = mean[:chans], std[:chans]
        got = B.images_u8_to_f32(imgs, mean, std)
        assert same_bits(got, normalise_u8(imgs, mean, std))


def test_kernel_takes_a_source_offset_by_whole_images_and_refuses_bad_arguments():
    L = B.lib()
    S, chans, n = 32, 3, 5
    imgs = np.random.default_rng(9).integers(0, 256, size=(n + 2, S, S, chans), dtype=np.uint8)
    mean, std = cfloats(B.IMAGENET_MEAN), cfloats(B.IMAGENET_STD)
    d_src, d_dst = B.DeviceArray.from_numpy(imgs), B.DeviceArray((n, chans, S, S))
    img_bytes = S * S * chans
    assert L.vithip_images_u8_to_f32(None, d_src.ptr + 2 * img_bytes, d_dst.ptr, n, S, chans, mean, std) == 0
    assert same_bits(d_dst.numpy(), normalise_u8(imgs[2:], B.IMAGENET_MEAN, B.IMAGENET_STD))
    bad = [
        (d_src.ptr + 1, d_dst.ptr, n, S, chans, mean, std),                                   # source not 4-byte aligned
        (d_src.ptr, d_dst.ptr, n, S, 5, cfloats((0.5,) * 5), cfloats((0.5,) * 5)),           # C = 5
        (d_src.ptr, d_dst.ptr, n, S, chans, mean, cfloats((0.229, 0.0, 0.225))),              # std = 0
        (d_src.ptr, d_dst.ptr, n, S, chans, mean, cfloats((0.229, float("inf"), 0.225))),     # std not finite
        (d_src.ptr, d_dst.ptr, n, S, chans, cfloats((0.485, float("nan"), 0.406)), std),     # mean not finite
        (d_src.ptr, d_dst.ptr, 0, S, chans, mean, std),                                       # n = 0
    ]
    for args in bad:
        assert L.vithip_images_u8_to_f32(None, *args) == 1  # hipErrorInvalidValue, nothing launched
    assert same_bits(d_dst.numpy(), normalise_u8(imgs[2:], B.IMAGENET_MEAN, B.IMAGENET_STD))


# ---- engines ---------------------------------------------------------------------------------------------------------

def check_device_path(eng, n, seed, consts=CONSTS_A):
    imgs = u8_images(eng.cfg, n, seed)
    ref = device_forward(eng, B.DeviceArray.from_numpy(normalise_u8(imgs, *consts)), n)
    got = device_forward(eng, B.DeviceArray.from_numpy(imgs), n, consts)
    for g, r in zip(got, ref):
        assert same_bits(g, r)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_device_path_b16_equals_fp32_forward_of_host_normalised_images(engines, dtype):
    eng = engines("b16", max_batch=16, dtype=dtype)
    check_device_path(eng, 7, 11)
    check_device_path(eng, 1, 12, CONSTS_B)
    check_device_path(eng, 2 * 16 + 3, 13)  # three chunks, a ragged tail


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_device_path_b16_two_lanes_and_pruned_last_layer(engines, dtype):
    eng = engines("b16", max_batch=16, dtype=dtype)
    eng.set_lanes(2)
    try:
        check_device_path(eng, 7, 21)
    finally:
        eng.set_lanes(1)
    check_device_path(engines("b16", max_batch=16, dtype=dtype, prune_last_layer=True), 7, 22)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("opt", [{}, {"lanes": 2}, {"prune_last_layer": True}, {"ln_fold": -1}, {"fp32_split": -1},
                                 {"lanes": 2, "prune_last_layer": True}])
def test_device_path_every_option_with_chunks(engines, dtype, opt):
    eng = engines("tiny", max_batch=4, dtype=dtype, **opt)
    for n, seed in [(2 * 4 + 3, 31), (1, 32), (4, 33)]:
        check_device_path(eng, n, seed)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("first_piece", [0, 5])
def test_host_path_equals_fp32_host_path(engines, dtype, first_piece):
    eng = engines("b16", max_batch=16, dtype=dtype, **({"host_first_piece": first_piece} if first_piece else {}))
    imgs = u8_images(eng.cfg, 37, 41)  # first piece, full pieces and a tail
    for consts in (CONSTS_A, CONSTS_B):
        ref = eng.forward(normalise_u8(imgs, *consts))
        assert same_bits(eng.forward_u8(imgs, *consts), ref)


def test_host_path_after_device_path_and_back(engines):
    """The device path normalises into the host path's staging: alternate the two (and the input kinds) on one engine."""
    eng = engines("tiny", max_batch=4)
    imgs = u8_images(eng.cfg, 11, 51)
    x = normalise_u8(imgs, *CONSTS_A)
    ref = eng.forward(x)
    d_u8 = B.DeviceArray.from_numpy(imgs)
    for _ in range(2):
        assert same_bits(device_forward(eng, d_u8, 11, CONSTS_A)[0], ref)
        assert same_bits(eng.forward_u8(imgs, *CONSTS_A), ref)
        assert same_bits(eng.forward(x), ref)


# ---- the graph cache -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_graph_replays_only_for_the_same_input_kind_and_constants(engines, dtype):
    plain = engines("tiny", max_batch=4, dtype=dtype)
    graph = engines("tiny", max_batch=4, dtype=dtype, use_graph=True)
    cfg, n = plain.cfg, 6
    imgs, other = u8_images(cfg, n, 61), u8_images(cfg, n, 62)
    fp32_bytes = n * cfg.in_chans * cfg.img_size * cfg.img_size * 4
    buf = B.DeviceArray((fp32_bytes,), np.uint8)  # one buffer, large enough for the fp32 images, for both input kinds
    NC = cfg.num_classes
    d_p, d_l, d_q = B.DeviceArray((n, NC)), B.DeviceArray((n,), np.int32), B.DeviceArray((n,))

    def run(eng, host, consts):
        data = np.ascontiguousarray(host)
        assert B.lib().vithip_memcpy_h2d(buf.ptr, data.ctypes.data, data.nbytes, None) == 0
        assert B.lib().vithip_device_sync() == 0  # the engine's streams do not wait for the NULL stream
        if consts is None:
            eng.forward_device(buf.ptr, n, d_p.ptr, d_l.ptr, d_q.ptr)
        else:
            eng.forward_device_u8(buf.ptr, n, d_p.ptr, consts[0], consts[1], d_l.ptr, d_q.ptr)
        eng.sync()
        return d_p.numpy(), d_l.numpy(), d_q.numpy()

    for consts in (CONSTS_A, CONSTS_B, CONSTS_A):
        want = run(plain, imgs, consts)
        got = run(graph, imgs, consts)
        assert all(same_bits(g, w) for g, w in zip(got, want))
    # an fp32 call at the address of the last u8 call: its own result, not a replay of the u8 graph
    x = normalise_u8(other, *CONSTS_B)
    want = run(plain, x, None)
    got = run(graph, x, None)
    assert all(same_bits(g, w) for g, w in zip(got, want))
    assert not same_bits(want[0], run(plain, imgs, CONSTS_A)[0])
    # and back to the u8 call
    assert all(same_bits(g, w) for g, w in zip(run(graph, imgs, CONSTS_A), run(plain, imgs, CONSTS_A)))


# ---- profile ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_profile_counts_the_conversion_as_an_embed_launch(engines, lanes, dtype):
    eng = engines("tiny", max_batch=4, dtype=dtype, lanes=lanes, profile=True)
    n = 4
    imgs = u8_images(eng.cfg, n, 71)
    eng.reset_stage_times()
    device_forward(eng, B.DeviceArray.from_numpy(normalise_u8(imgs, *CONSTS_A)), n)
    f32 = {s: v["launches"] for s, v in eng.stage_times()["stages"].items()}
    eng.reset_stage_times()
    device_forward(eng, B.DeviceArray.from_numpy(imgs), n, CONSTS_A)
    u8 = eng.stage_times()
    assert u8["images"] == n
    counts = {s: v["launches"] for s, v in u8["stages"].items()}
    assert f32["embed"] == lanes and counts["embed"] == 2 * lanes
    assert {s: k for s, k in counts.items() if s != "embed"} == {s: k for s, k in f32.items() if s != "embed"}
    eng.reset_stage_times()
    eng.forward_u8(imgs, *CONSTS_A)
    assert eng.stage_times()["stages"]["embed"]["launches"] == 2 * lanes


# ---- errors ----------------------------------------------------------------------------------------------------------

def test_invalid_arguments_return_vit_err_arg_and_leave_the_engine_usable(engines):
    L = B.lib()
    eng = engines("tiny", max_batch=4)
    cfg, n = eng.cfg, 3
    imgs = u8_images(cfg, n, 81)
    d_u8 = B.DeviceArray.from_numpy(np.concatenate([imgs.reshape(-1), np.zeros(16, np.uint8)]))
    d_p = B.DeviceArray((n, cfg.num_classes))
    mean, std = cfloats(B.IMAGENET_MEAN), cfloats(B.IMAGENET_STD)
    nan, inf = float("nan"), float("inf")
    bad = [
        (d_u8.ptr, n, None, std),
        (d_u8.ptr, n, mean, None),
        (d_u8.ptr, n, cfloats((0.485, nan, 0.406)), std),
        (d_u8.ptr, n, cfloats((inf, 0.456, 0.406)), std),
        (d_u8.ptr, n, mean, cfloats((0.229, 0.224, -inf))),
        (d_u8.ptr, n, mean, cfloats((0.229, 0.0, 0.225))),
        (d_u8.ptr, 0, mean, std),
        (d_u8.ptr, -2, mean, std),
        (d_u8.ptr + 1, n, mean, std),
        (None, n, mean, std),
    ]
    ref = eng.forward(normalise_u8(imgs, *CONSTS_A))
    for d_images, nn, m, s in bad:
        assert L.vit_engine_forward_device_u8(eng._h, d_images, nn, m, s, d_p.ptr, None, None, None) == VIT_ERR_ARG
        assert L.vit_engine_last_error(eng._h)
        got = device_forward(eng, d_u8, n, CONSTS_A)[0]
        assert same_bits(got, ref)
    ptrs = (C.c_void_p * n)(*[imgs[i].ctypes.data for i in range(n)])
    probs = np.empty((n, cfg.num_classes), np.float32)
    rows = (B.f32p * n)(*[probs[i].ctypes.data_as(B.f32p) for i in range(n)])
    for nn, m, s, p in [(n, None, std, ptrs), (n, mean, cfloats((0.229, 0.224, 0.0)), ptrs), (0, mean, std, ptrs),
                        (n, cfloats((nan, 0.456, 0.406)), std, ptrs), (n, mean, std, None)]:
        assert L.vit_engine_forward_host_u8(eng._h, p, nn, m, s, rows) == VIT_ERR_ARG
        assert same_bits(eng.forward_u8(imgs, *CONSTS_A), ref)
    # more than 4 channels
    cfg5 = dataclasses.replace(synth.VIT_TINY, in_chans=5)
    eng5 = B.Engine(cfg5, max_batch=4)
    try:
        five = cfloats((0.5,) * 5)
        assert L.vit_engine_forward_device_u8(eng5._h, d_u8.ptr, 1, five, five, d_p.ptr, None, None, None) == VIT_ERR_ARG
        assert b"channels" in L.vit_engine_last_error(eng5._h)
    finally:
        eng5.close()
