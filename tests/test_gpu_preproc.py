"""Resize + CenterCrop + normalisation on the device (vithip_images_u8_resize_crop_to_f32, vit_engine_*_images).

Every comparison is bitwise, no tolerances: the kernel against the numpy restatement of Pillow's arithmetic (tests/preproc_model.py,
itself held against Pillow in tests/test_preproc_model.py), and every _images call against the matching _u8 call on the bytes that
restatement gives.  The refusals are argument checks on the host: nothing here launches a kernel with bad arguments.
"""
import ctypes as C

import numpy as np
import pytest

import preproc_model as M
from engine_helpers import CONSTS, cfloats, engines, same_bits, weights  # noqa: F401 (fixtures)
from test_input_u8_model import normalise_u8
from vit_amd import binding as B

pytestmark = pytest.mark.gpu

VIT_ERR_ARG = 1
HIP_INVALID = 1  # hipErrorInvalidValue
MEAN4, STD4 = (0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, -0.25)


def random_images(sizes, chans, seed):
    rng = np.random.default_rng(seed)
    out = []
    for k, (h, w) in enumerate(sizes):
        im = rng.integers(0, 256, size=(h, w, chans), dtype=np.uint8)
        if k % 3 == 1:  # some smooth ones: ramps and a few saturated rows
            im[:] = (np.add.outer(np.arange(h) * 3, np.arange(w) * 5)[:, :, None] + np.arange(chans) * 40) % 256
            im[: max(h // 8, 1)] = 255
        out.append(im)
    return out


class DeviceImages:
    """Images packed back to back in one device buffer, the first at an odd address: (ptr, H, W) triples in .triples."""

    def __init__(self, images, lead=1):
        sizes = [im.size for im in images]
        buf = np.zeros(lead + sum(sizes) + 16, np.uint8)
        self.triples, off = [], lead
        for im, sz in zip(images, sizes):
            buf[off:off + sz] = np.ascontiguousarray(im).reshape(-1)
            self.triples.append((off, im.shape[0], im.shape[1]))
            off += sz
        self.buf = B.DeviceArray.from_numpy(buf)
        self.triples = [(self.buf.ptr + o, h, w) for o, h, w in self.triples]
        self.records = B.image_records(self.triples)


def run_kernel(dev, dst, S, chans, R, mean, std, n=None):
    n = len(dev.triples) if n is None else n
    return B.lib().vithip_images_u8_resize_crop_to_f32(None, dev.records, n, dst.ptr, S, chans, R, cfloats(mean[:chans]), cfloats(std[:chans]))


def mixed_sizes(S, R):
    """Up-scaled, down-scaled, portrait, landscape, square, H == W == R, one pixel wide / high, strongly down-scaled, odd widths."""
    big = 64 * R if R <= 40 else 8 * R  # 64 x is the launcher's limit; kept for the small crops, where the source stays a few MB
    return [(R, R), (R // 3 + 1, R // 2 + 2), (3 * R + 1, 2 * R + 5), (2 * R - 1, 5 * R + 3), (R + 1, R - 1), (R + 17, R + 17),
            (1, 9), (11, 1), (big, big + 7), (big + 3, big), (2 * R, R), (R, 7 * R + 2)]


# ---- the kernel ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chans", [1, 3, 4])
@pytest.mark.parametrize("S,R", [(32, 36), (32, 32), (64, 72), (224, 256), (224, 224)])
def test_kernel_matches_the_restatement(S, R, chans):
    sizes = mixed_sizes(S, R)
    imgs = random_images(sizes, chans, 1000 * S + 10 * R + chans)
    dev = DeviceImages(imgs)
    assert any(p % 2 for p, _, _ in dev.triples) and any(p % 4 for p, _, _ in dev.triples)
    dst = B.DeviceArray((len(imgs), chans, S, S))
    assert run_kernel(dev, dst, S, chans, R, MEAN4, STD4) == 0
    got, ref = dst.numpy(), M.preprocess(imgs, R, S, MEAN4[:chans], STD4[:chans])
    for i in range(len(imgs)):
        assert same_bits(got[i], ref[i]), (i, sizes[i])
    if R == S:  # nothing to resize in image 0: the bits of the plain 8-bit conversion
        assert same_bits(got[0], B.images_u8_to_f32(imgs[0][None], MEAN4[:chans], STD4[:chans])[0])
    assert same_bits(B.images_u8_resize_crop_to_f32(imgs[1:4], S, R, MEAN4[:chans], STD4[:chans]), ref[1:4])  # the binding's own op


def test_kernel_batch_larger_than_one_launch_and_position_independence():
    S, R, chans, n = 32, 36, 3, 150
    rng = np.random.default_rng(77)
    sizes = [(int(h), int(w)) for h, w in rng.integers(9, 90, size=(n, 2))]
    imgs = random_images(sizes, chans, 78)
    for pos in (0, 63, 64, n - 1):
        imgs[pos] = imgs[0]
    dev = DeviceImages(imgs)
    dst = B.DeviceArray((n, chans, S, S))
    assert run_kernel(dev, dst, S, chans, R, *CONSTS) == 0
    got = dst.numpy()
    assert same_bits(got, M.preprocess(imgs, R, S, *CONSTS))
    for pos in (63, 64, n - 1):
        assert same_bits(got[pos], got[0])


def test_kernel_refuses_bad_arguments_and_writes_nothing():
    L = B.lib()
    S, R, chans = 32, 36, 3
    imgs = random_images([(40, 50), (50, 40), (36, 36)], chans, 5)
    dev = DeviceImages(imgs, lead=0)
    n = len(imgs)
    poison = np.full((n, chans, S, S), 0x7FC0BEEF, np.uint32).view(np.float32)
    dst = B.DeviceArray.from_numpy(poison)
    mean, std = cfloats(B.IMAGENET_MEAN), cfloats(B.IMAGENET_STD)
    nan, inf = float("nan"), float("inf")

    def recs(*triples):
        return B.image_records(triples)

    t = dev.triples
    good = dev.records
    bad = [
        (None, n, dst.ptr, S, chans, R, mean, std),                                            # no records
        (good, n, None, S, chans, R, mean, std),                                               # no destination
        (good, n, dst.ptr, S, chans, R, None, std),
        (good, n, dst.ptr, S, chans, R, mean, None),
        (good, 0, dst.ptr, S, chans, R, mean, std),                                            # n < 1
        (good, n, dst.ptr, S, 0, R, mean, std),                                                # chans outside 1..4
        (good, n, dst.ptr, S, 5, R, cfloats((0.5,) * 5), cfloats((0.5,) * 5)),
        (good, n, dst.ptr, 0, chans, R, mean, std),                                            # img_size < 4
        (good, n, dst.ptr, 30, chans, R, mean, std),                                           # img_size not a multiple of 4
        (good, n, dst.ptr, S, chans, S - 1, mean, std),                                        # resize_shorter < img_size
        (good, n, dst.ptr, S, chans, 4097, mean, std),                                         # resize_shorter > 4096
        (recs(t[0], (t[1][0], 0, 40), t[2]), n, dst.ptr, S, chans, R, mean, std),              # height 0
        (recs(t[0], (t[1][0], 40, 16385), t[2]), n, dst.ptr, S, chans, R, mean, std),          # width > 16384
        (recs(t[0], t[1], (t[2][0], -3, 36)), n, dst.ptr, S, chans, R, mean, std),             # negative height
        (recs(t[0], (t[1][0], 64 * R + 1, 64 * R + 1), t[2]), n, dst.ptr, S, chans, R, mean, std),  # shorter side > 64 x resize_shorter
        (recs(t[0], (0, 50, 40), t[2]), n, dst.ptr, S, chans, R, mean, std),                   # a NULL source
        (good, n, dst.ptr + 4, S, chans, R, mean, std),                                        # dst not 16-byte aligned
        (good, n, dst.ptr, S, chans, R, cfloats((0.485, nan, 0.406)), std),
        (good, n, dst.ptr, S, chans, R, mean, cfloats((0.229, inf, 0.225))),
        (good, n, dst.ptr, S, chans, R, mean, cfloats((0.229, 0.224, 0.0))),
    ]
    for args in bad:
        assert L.vithip_images_u8_resize_crop_to_f32(None, *args) == HIP_INVALID, args
    assert same_bits(dst.numpy(), poison)
    assert L.vithip_images_u8_resize_crop_to_f32(None, good, n, dst.ptr, S, chans, R, mean, std) == 0
    assert same_bits(dst.numpy(), M.preprocess(imgs, R, S, *CONSTS))


# ---- engines ---------------------------------------------------------------------------------------------------------

def resize_for(cfg):
    return {32: 36, 224: 256}[cfg.img_size]


def engine_sizes(cfg, n, seed):
    R = resize_for(cfg)
    base = [(R, R), (R + R // 2, 2 * R - 1), (2 * R + 1, R + 3), (R // 2, R // 2 + 5), (R + 1, R + 1), (3 * R, R), (cfg.img_size, cfg.img_size)]
    rng = np.random.default_rng(seed)
    extra = [(int(h), int(w)) for h, w in rng.integers(R // 3, 2 * R, size=(max(n - len(base), 0), 2))]
    return (base + extra)[:n]


def model_bytes(cfg, imgs):
    """What torchvision's Resize + CenterCrop make of the images: uint8 [n][S][S][C]."""
    return np.stack([M.resize_crop(im, resize_for(cfg), cfg.img_size) for im in imgs])


def device_forward_images(eng, dev, consts=CONSTS, stream=0):
    n, NC = len(dev.triples), eng.cfg.num_classes
    d_p, d_l, d_q = B.DeviceArray((n, NC)), B.DeviceArray((n,), np.int32), B.DeviceArray((n,))
    eng.forward_device_images(dev.triples, d_p.ptr, resize_for(eng.cfg), consts[0], consts[1], d_l.ptr, d_q.ptr, stream)
    eng.sync()
    return d_p.numpy(), d_l.numpy(), d_q.numpy()


def device_forward_u8(eng, u8, consts=CONSTS):
    n, NC = u8.shape[0], eng.cfg.num_classes
    d_in = B.DeviceArray.from_numpy(u8)
    d_p, d_l, d_q = B.DeviceArray((n, NC)), B.DeviceArray((n,), np.int32), B.DeviceArray((n,))
    eng.forward_device_u8(d_in.ptr, n, d_p.ptr, consts[0], consts[1], d_l.ptr, d_q.ptr)
    eng.sync()
    return d_p.numpy(), d_l.numpy(), d_q.numpy()


def check_device_path(eng, n, seed, consts=CONSTS):
    imgs = random_images(engine_sizes(eng.cfg, n, seed), eng.cfg.in_chans, seed)
    dev = DeviceImages(imgs)
    u8 = model_bytes(eng.cfg, imgs)
    for g, r in zip(device_forward_images(eng, dev, consts), device_forward_u8(eng, u8, consts)):
        assert same_bits(g, r)
    for kind in ("cls", "mean"):
        shape = eng.feature_shape(n, kind)
        d_a, d_b, d_in = B.DeviceArray(shape), B.DeviceArray(shape), B.DeviceArray.from_numpy(u8)
        eng.features_device_images(dev.triples, d_a.ptr, resize_for(eng.cfg), kind, False, consts[0], consts[1])
        eng.features_device_u8(d_in.ptr, n, d_b.ptr, kind, False, consts[0], consts[1])
        eng.sync()
        assert same_bits(d_a.numpy(), d_b.numpy()), kind


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_device_path_tiny_equals_u8_forward_of_the_restatements_bytes(engines, dtype, lanes):
    eng = engines("tiny", max_batch=4, dtype=dtype, lanes=lanes)
    for n, seed in [(2 * 4 + 3, 101), (1, 102), (4, 103)]:
        check_device_path(eng, n, seed)
    check_device_path(eng, 5, 104, ((0.5, 0.25, 0.125), (0.3, -0.6, 0.9)))


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_device_path_b16_equals_u8_forward_of_the_restatements_bytes(engines, dtype, lanes):
    eng = engines("b16", max_batch=8, dtype=dtype)
    eng.set_lanes(lanes)
    try:
        check_device_path(eng, 2 * 8 + 3, 111 + lanes)  # three chunks, a ragged tail
    finally:
        eng.set_lanes(1)


def budget_sizes():
    """VIT_TINY, max_batch 16: a slot holds 16 * 3 * 32 * 32 * 4 = 196608 bytes.  Images of 40 .. 70 KB: three or four to a piece."""
    return [(120, 130), (150, 110), (128, 128), (100, 200), (36, 36), (140, 160), (90, 250), (130, 170), (160, 120), (40, 50), (150, 150),
            (125, 175), (110, 210), (37, 41), (170, 130), (145, 155), (200, 100), (120, 120), (135, 165), (50, 36), (155, 145), (180, 120)]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("first_piece", [0, 8])
def test_host_path_equals_device_path_when_the_byte_budget_cuts_the_pieces(engines, dtype, first_piece):
    eng = engines("tiny", max_batch=16, dtype=dtype, **({"host_first_piece": first_piece} if first_piece else {}))
    sizes = budget_sizes()
    cap = 16 * 3 * 32 * 32 * 4
    assert sum(h * w * 3 for h, w in sizes) > 5 * cap and max(h * w * 3 for h, w in sizes) < cap / 2  # many pieces, all shorter than 16
    imgs = random_images(sizes, 3, 201)
    ref = device_forward_images(eng, DeviceImages(imgs))[0]
    assert same_bits(eng.forward_images(imgs, 36), ref)
    assert same_bits(ref, eng.forward_u8(model_bytes(eng.cfg, imgs)))
    # host call -> _u8 host call -> host call again on one engine, features too
    assert same_bits(eng.forward_images(imgs, 36), ref)
    for kind in ("cls", "mean"):
        assert same_bits(eng.features_images(imgs, 36, kind), eng.features_u8(model_bytes(eng.cfg, imgs), kind))


def test_host_path_b16(engines):
    eng = engines("b16", max_batch=8)
    imgs = random_images(engine_sizes(eng.cfg, 11, 301), 3, 301)
    assert same_bits(eng.forward_images(imgs, 256), eng.forward_u8(model_bytes(eng.cfg, imgs)))


# ---- the graph cache -------------------------------------------------------------------------------------------------

def test_a_captured_graph_survives_an_images_call(engines):
    plain = engines("tiny", max_batch=4)
    graph = engines("tiny", max_batch=4, use_graph=True)
    cfg, n = plain.cfg, 4
    x = normalise_u8(np.random.default_rng(401).integers(0, 256, size=(n, 32, 32, 3), dtype=np.uint8), *CONSTS)
    d_x, d_p = B.DeviceArray.from_numpy(x), B.DeviceArray((n, cfg.num_classes))
    imgs = random_images(engine_sizes(cfg, n, 402), 3, 402)
    dev = DeviceImages(imgs)

    def fp32(eng):
        eng.forward_device(d_x.ptr, n, d_p.ptr)
        eng.sync()
        return d_p.numpy()

    want = fp32(plain)
    assert same_bits(fp32(graph), want)   # captured
    assert same_bits(fp32(graph), want)   # replayed
    got = device_forward_images(graph, dev)
    for g, w in zip(got, device_forward_images(plain, dev)):
        assert same_bits(g, w)
    assert not same_bits(got[0], want)
    assert same_bits(fp32(graph), want)   # the old graph, its old bits
    assert same_bits(device_forward_images(graph, dev)[0], got[0])


# ---- profile ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", [1, 2])
def test_profile_counts_the_preprocessing_as_embed_launches(engines, lanes):
    eng = engines("tiny", max_batch=4, lanes=lanes, profile=True)
    n = 4
    imgs = random_images(engine_sizes(eng.cfg, n, 501), 3, 501)
    u8 = model_bytes(eng.cfg, imgs)
    eng.reset_stage_times()
    device_forward_u8(eng, u8)
    ref = {s: v["launches"] for s, v in eng.stage_times()["stages"].items()}
    eng.reset_stage_times()
    device_forward_images(eng, DeviceImages(imgs))
    t = eng.stage_times()
    assert t["images"] == n
    counts = {s: v["launches"] for s, v in t["stages"].items()}
    assert counts == ref and counts["embed"] == 2 * lanes  # one bracket per lane, as for the 8-bit conversion
    eng.reset_stage_times()
    eng.forward_images(imgs, 36)
    assert eng.stage_times()["stages"]["embed"]["launches"] == 2 * lanes


# ---- errors ----------------------------------------------------------------------------------------------------------

def test_invalid_arguments_return_vit_err_arg_and_leave_the_engine_usable(engines):
    L = B.lib()
    eng = engines("tiny", max_batch=4)
    cfg, n = eng.cfg, 6
    imgs = random_images(engine_sizes(cfg, n, 601), 3, 601)
    dev = DeviceImages(imgs)
    ref = device_forward_u8(eng, model_bytes(cfg, imgs))[0]
    poison = np.full((n, cfg.num_classes), 0x7FC0BEEF, np.uint32).view(np.float32)
    t = dev.triples
    pp = B.preproc_params(36, *CONSTS, 3)

    def with_record(i, rec):
        return B.image_records(t[:i] + [rec] + t[i + 1:])

    def params(R=36, mean=B.IMAGENET_MEAN, std=B.IMAGENET_STD):
        p = B.preproc_params(R, (0.0,) * 3, (1.0,) * 3, 3)
        for c in range(3):
            p.mean[c], p.std[c] = mean[c], std[c]
        return C.byref(p)

    nan = float("nan")
    bad = [
        (dev.records, n, None),                                        # NULL pp
        (None, n, params()),
        (dev.records, 0, params()),
        (dev.records, n, params(R=31)),                                # R < S
        (dev.records, n, params(R=4097)),
        (dev.records, n, params(mean=(0.5, nan, 0.5))),
        (dev.records, n, params(std=(0.5, 0.0, 0.5))),
        (with_record(3, (t[3][0], 0, 20)), n, params()),               # a bad record in the middle of the batch
        (with_record(4, (0, 20, 20)), n, params()),                    # NULL pixels
        (with_record(5, (t[5][0], 64 * 36 + 1, 64 * 36 + 1)), n, params()),
        (with_record(2, (t[2][0], 16385, 40)), n, params()),
    ]
    for recs, nn, p in bad:
        d_p = B.DeviceArray.from_numpy(poison)
        assert L.vit_engine_forward_device_images(eng._h, recs, nn, p, d_p.ptr, None, None, None) == VIT_ERR_ARG
        assert L.vit_engine_last_error(eng._h)
        eng.sync()
        assert same_bits(d_p.numpy(), poison)
        assert same_bits(device_forward_images(eng, dev)[0], ref)
    d_p = B.DeviceArray.from_numpy(poison)
    assert L.vit_engine_forward_device_images(eng._h, bad[7][0], n, params(), d_p.ptr, None, None, None) == VIT_ERR_ARG
    assert b"image 3" in L.vit_engine_last_error(eng._h)  # the message names the record
    # host path: the same refusals, and an image that does not fit a staging slot alone (4 * 3 * 32 * 32 * 4 = 49152 bytes)
    probs = poison.copy()
    rows = (B.f32p * n)(*[probs[i].ctypes.data_as(B.f32p) for i in range(n)])
    keep, hrecs = B.host_image_records(imgs, 3)
    huge = np.zeros((130, 130, 3), np.uint8)  # 50700 bytes
    keep2, hrecs_huge = B.host_image_records(imgs[:4] + [huge] + imgs[5:], 3)
    for recs, nn, p, r in [(hrecs, n, None, rows), (hrecs, n, params(R=31), rows), (hrecs, n, params(), None), (hrecs_huge, n, params(), rows),
                           (B.image_records([(keep[0].ctypes.data, 0, 5)] * n), n, params(), rows)]:
        assert L.vit_engine_forward_host_images(eng._h, recs, nn, p, r) == VIT_ERR_ARG
        assert same_bits(probs, poison)
        assert same_bits(eng.forward_images(imgs, 36), ref)
    assert L.vit_engine_forward_host_images(eng._h, hrecs_huge, n, params(), rows) == VIT_ERR_ARG
    assert b"image 4" in L.vit_engine_last_error(eng._h)
    assert L.vit_engine_features_device_images(eng._h, dev.records, n, C.byref(pp), None, None, None) == VIT_ERR_ARG
    assert same_bits(eng.forward_u8(model_bytes(cfg, imgs)), ref)
