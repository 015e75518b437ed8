"""Resize with Pillow's bicubic filter on the device (vithip_images_u8_resize_crop_to_f32_filter, vit_engine_set_resize_filter).

Every comparison is bitwise, as in tests/test_gpu_preproc.py: the kernel against the numpy restatement (tests/preproc_filter_model.py,
itself held against Pillow in tests/test_preproc_filter_model.py), and every _images call of an engine set to bicubic against the
matching _u8 call on the bytes that restatement gives.  Every third source is binary 0 / 255 noise: the sums of a bicubic pass then
leave [0, 255] on both sides (counted here), so a kernel that clamps only above fails.  The refusals are argument checks on the host.
"""
import ctypes as C

import numpy as np
import pytest

import preproc_filter_model as F
from engine_helpers import CONSTS, cfloats, engines, same_bits, weights  # noqa: F401 (fixtures)
from test_gpu_preproc import DeviceImages, budget_sizes, engine_sizes, mixed_sizes, resize_for
from vit_amd import binding as B

pytestmark = pytest.mark.gpu

VIT_ERR_ARG = 1
HIP_INVALID = 1  # hipErrorInvalidValue
BILINEAR, BICUBIC = 0, 1
LIMIT = 64  # shorter side <= LIMIT x resize_shorter, for both filters
MEAN4, STD4 = (0.485, 0.456, 0.406, 0.5), (0.229, 0.224, 0.225, -0.25)


def random_images(sizes, chans, seed):
    """Uniform random bytes; k % 3 == 1: ramps with saturated rows; k % 3 == 2: binary 0 / 255 noise."""
    rng = np.random.default_rng(seed)
    out = []
    for k, (h, w) in enumerate(sizes):
        im = rng.integers(0, 256, size=(h, w, chans), dtype=np.uint8)
        if k % 3 == 1:
            im[:] = (np.add.outer(np.arange(h) * 3, np.arange(w) * 5)[:, :, None] + np.arange(chans) * 40) % 256
            im[: max(h // 8, 1)] = 255
        elif k % 3 == 2:
            im = ((im & 1) * 255).astype(np.uint8)
        out.append(im)
    return out


def run_kernel(dev, dst, S, chans, R, flt, mean, std, n=None):
    n = len(dev.triples) if n is None else n
    return B.lib().vithip_images_u8_resize_crop_to_f32_filter(None, dev.records, n, dst.ptr, S, chans, R, flt, cfloats(mean[:chans]),
                                                              cfloats(std[:chans]))


def assert_both_clamps_ran(clamps):
    for direction in ("h", "v"):
        assert clamps[direction]["low"] >= 1 and clamps[direction]["high"] >= 1, clamps


# ---- the kernel ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chans", [1, 3, 4])
@pytest.mark.parametrize("S,R", [(32, 36), (32, 32), (64, 72)])
def test_kernel_matches_the_restatement(S, R, chans):
    sizes = mixed_sizes(S, R)  # `big` is LIMIT x R for the two small crops
    assert R > 40 or (LIMIT * R, LIMIT * R + 7) in sizes
    imgs = random_images(sizes, chans, 2000 * S + 10 * R + chans)
    dev = DeviceImages(imgs)
    assert any(p % 2 for p, _, _ in dev.triples) and any(p % 4 for p, _, _ in dev.triples)
    dst = B.DeviceArray((len(imgs), chans, S, S))
    assert run_kernel(dev, dst, S, chans, R, BICUBIC, MEAN4, STD4) == 0
    clamps = {}
    got, ref = dst.numpy(), F.preprocess(imgs, R, S, MEAN4[:chans], STD4[:chans], F.BICUBIC, clamps)
    assert_both_clamps_ran(clamps)
    for i in range(len(imgs)):
        assert same_bits(got[i], ref[i]), (i, sizes[i])
    if R == S:  # nothing to resize in image 0: the bits of the plain 8-bit conversion
        assert same_bits(got[0], B.images_u8_to_f32(imgs[0][None], MEAN4[:chans], STD4[:chans])[0])
    assert same_bits(B.images_u8_resize_crop_to_f32(imgs[1:4], S, R, MEAN4[:chans], STD4[:chans], filter="bicubic"), ref[1:4])
    assert not same_bits(B.images_u8_resize_crop_to_f32(imgs[1:4], S, R, MEAN4[:chans], STD4[:chans]), ref[1:4])  # the default: bilinear


def test_kernel_production_tile_shape():
    S, R, chans = 224, 256, 3
    sizes = [(375, 500), (500, 333), (200, 170), (1080, 1920)]
    imgs = random_images(sizes, chans, 31)
    dev = DeviceImages(imgs)
    dst = B.DeviceArray((len(imgs), chans, S, S))
    assert run_kernel(dev, dst, S, chans, R, BICUBIC, *CONSTS) == 0
    clamps = {}
    got, ref = dst.numpy(), F.preprocess(imgs, R, S, *CONSTS, F.BICUBIC, clamps)
    assert_both_clamps_ran(clamps)
    for i in range(len(imgs)):
        assert same_bits(got[i], ref[i]), (i, sizes[i])


def test_kernel_batch_larger_than_one_launch_and_position_independence():
    S, R, chans, n = 32, 36, 3, 150
    rng = np.random.default_rng(79)
    sizes = [(int(h), int(w)) for h, w in rng.integers(9, 90, size=(n, 2))]
    imgs = random_images(sizes, chans, 80)
    for pos in (0, 63, 64, n - 1):
        imgs[pos] = imgs[2]  # a binary one
    dev = DeviceImages(imgs)
    dst = B.DeviceArray((n, chans, S, S))
    assert run_kernel(dev, dst, S, chans, R, BICUBIC, *CONSTS) == 0
    got = dst.numpy()
    assert same_bits(got, F.preprocess(imgs, R, S, *CONSTS, F.BICUBIC))
    for pos in (63, 64, n - 1):
        assert same_bits(got[pos], got[0])


def test_filter_entry_with_bilinear_gives_the_bits_of_the_old_entry():
    L = B.lib()
    for S, R, chans in [(32, 36, 3), (64, 72, 4), (32, 32, 1)]:
        imgs = random_images(mixed_sizes(S, R), chans, 7 * S + chans)
        dev = DeviceImages(imgs)
        old, new = B.DeviceArray((len(imgs), chans, S, S)), B.DeviceArray((len(imgs), chans, S, S))
        mean, std = cfloats(MEAN4[:chans]), cfloats(STD4[:chans])
        assert L.vithip_images_u8_resize_crop_to_f32(None, dev.records, len(imgs), old.ptr, S, chans, R, mean, std) == 0
        assert run_kernel(dev, new, S, chans, R, BILINEAR, MEAN4, STD4) == 0
        assert same_bits(old.numpy(), new.numpy())
        assert same_bits(new.numpy(), F.preprocess(imgs, R, S, MEAN4[:chans], STD4[:chans], F.BILINEAR))


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
    over = LIMIT * R + 1
    bad = [
        (good, n, dst.ptr, S, chans, R, 2, mean, std),                                                  # an unknown filter
        (good, n, dst.ptr, S, chans, R, -1, mean, std),
        (recs(t[0], (t[1][0], over, over), t[2]), n, dst.ptr, S, chans, R, BICUBIC, mean, std),         # one pixel over the limit
        (recs(t[0], t[1], (t[2][0], over + 40, over)), n, dst.ptr, S, chans, R, BICUBIC, mean, std),
        # each refusal of the old entry, once
        (None, n, dst.ptr, S, chans, R, BICUBIC, mean, std),
        (good, n, None, S, chans, R, BICUBIC, mean, std),
        (good, n, dst.ptr, S, chans, R, BICUBIC, None, std),
        (good, n, dst.ptr, S, chans, R, BICUBIC, mean, None),
        (good, 0, dst.ptr, S, chans, R, BICUBIC, mean, std),
        (good, n, dst.ptr, S, 0, R, BICUBIC, mean, std),
        (good, n, dst.ptr, S, 5, R, BICUBIC, cfloats((0.5,) * 5), cfloats((0.5,) * 5)),
        (good, n, dst.ptr, 0, chans, R, BICUBIC, mean, std),
        (good, n, dst.ptr, 30, chans, R, BICUBIC, mean, std),
        (good, n, dst.ptr, S, chans, S - 1, BICUBIC, mean, std),
        (good, n, dst.ptr, S, chans, 4097, BICUBIC, mean, std),
        (recs(t[0], (t[1][0], 0, 40), t[2]), n, dst.ptr, S, chans, R, BICUBIC, mean, std),
        (recs(t[0], (t[1][0], 40, 16385), t[2]), n, dst.ptr, S, chans, R, BICUBIC, mean, std),
        (recs(t[0], t[1], (t[2][0], -3, 36)), n, dst.ptr, S, chans, R, BICUBIC, mean, std),
        (recs(t[0], (0, 50, 40), t[2]), n, dst.ptr, S, chans, R, BICUBIC, mean, std),
        (good, n, dst.ptr + 4, S, chans, R, BICUBIC, mean, std),
        (good, n, dst.ptr, S, chans, R, BICUBIC, cfloats((0.485, nan, 0.406)), std),
        (good, n, dst.ptr, S, chans, R, BICUBIC, mean, cfloats((0.229, inf, 0.225))),
        (good, n, dst.ptr, S, chans, R, BICUBIC, mean, cfloats((0.229, 0.224, 0.0))),
    ]
    for args in bad:
        assert L.vithip_images_u8_resize_crop_to_f32_filter(None, *args) == HIP_INVALID, args
    assert L.vithip_images_u8_resize_crop_check_filter(good, n, S, chans, R, 2) == -1
    assert L.vithip_images_u8_resize_crop_check_filter(bad[2][0], n, S, chans, R, BICUBIC) == 2
    assert same_bits(dst.numpy(), poison)
    assert L.vithip_images_u8_resize_crop_to_f32_filter(None, good, n, dst.ptr, S, chans, R, BICUBIC, mean, std) == 0
    assert same_bits(dst.numpy(), F.preprocess(imgs, R, S, *CONSTS, F.BICUBIC))


# ---- engines ---------------------------------------------------------------------------------------------------------

def model_bytes(cfg, imgs, flt=F.BICUBIC):
    return np.stack([F.resize_crop(im, resize_for(cfg), cfg.img_size, flt) for im in imgs])


def device_rows(eng, shape, call):
    """The rows a device call writes: call(d_out pointer) enqueues it."""
    d_out = B.DeviceArray(shape)
    call(d_out.ptr)
    eng.sync()
    return d_out.numpy()


def forward_images(eng, dev):
    return device_rows(eng, (len(dev.triples), eng.cfg.num_classes), lambda d: eng.forward_device_images(dev.triples, d, resize_for(eng.cfg)))


def forward_u8(eng, u8):
    d_in = B.DeviceArray.from_numpy(u8)
    return device_rows(eng, (u8.shape[0], eng.cfg.num_classes), lambda d: eng.forward_device_u8(d_in.ptr, u8.shape[0], d))


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_engine_set_to_bicubic_equals_u8_calls_on_the_restatements_bytes(engines, dtype, lanes):
    eng = engines("tiny", max_batch=4, dtype=dtype, lanes=lanes)
    other = engines("tiny", max_batch=4, dtype=dtype, lanes=lanes, profile=True)  # another engine: its filter stays bilinear
    cfg, n, R = eng.cfg, 2 * 4 + 3, resize_for(eng.cfg)
    imgs = random_images(engine_sizes(cfg, n, 701), cfg.in_chans, 701 + lanes)
    dev = DeviceImages(imgs)
    cubic, linear = model_bytes(cfg, imgs), model_bytes(cfg, imgs, F.BILINEAR)
    d_cubic = B.DeviceArray.from_numpy(cubic)
    assert eng.get_resize_filter() == other.get_resize_filter() == "bilinear"
    bilinear_probs = forward_images(eng, dev)
    assert same_bits(bilinear_probs, forward_u8(eng, linear))
    eng.set_resize_filter("bicubic")
    try:
        assert eng.get_resize_filter() == "bicubic" and other.get_resize_filter() == "bilinear"
        probs = forward_images(eng, dev)
        assert same_bits(probs, forward_u8(eng, cubic))
        assert not same_bits(probs, bilinear_probs)
        assert same_bits(forward_images(other, dev), bilinear_probs)  # the filter of one engine does not reach another
        shape = eng.feature_shape(n, "mean")
        assert same_bits(device_rows(eng, shape, lambda d: eng.features_device_images(dev.triples, d, R, "mean")),
                         device_rows(eng, shape, lambda d: eng.features_device_u8(d_cubic.ptr, n, d, "mean")))
        shape = eng.attention_shape(n, "heads")
        assert same_bits(device_rows(eng, shape, lambda d: eng.cls_attention_device_images(dev.triples, d, R, "heads")),
                         device_rows(eng, shape, lambda d: eng.cls_attention_device_u8(d_cubic.ptr, n, d, "heads")))
        layers = [0, -1]
        shape = eng.intermediate_shape(n, layers, "cls")
        assert same_bits(device_rows(eng, shape, lambda d: eng.intermediate_device_images(dev.triples, d, R, layers, "cls")),
                         device_rows(eng, shape, lambda d: eng.intermediate_device_u8(d_cubic.ptr, n, d, layers, "cls")))
        assert same_bits(eng.forward_images(imgs, R), probs)  # the host path, one piece
        eng.set_resize_filter("bilinear")
        assert eng.get_resize_filter() == "bilinear"
        assert same_bits(forward_images(eng, dev), bilinear_probs)
        assert same_bits(eng.forward_images(imgs, R), bilinear_probs)
    finally:
        eng.set_resize_filter("bilinear")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_host_path_with_a_byte_budget_cut(engines, dtype):
    eng = engines("tiny", max_batch=16, dtype=dtype)
    sizes = budget_sizes()
    cap = 16 * 3 * 32 * 32 * 4
    assert sum(h * w * 3 for h, w in sizes) > 5 * cap  # many pieces
    imgs = random_images(sizes, 3, 801)
    cubic = model_bytes(eng.cfg, imgs)
    bilinear_probs = eng.forward_images(imgs, 36)
    eng.set_resize_filter("bicubic")
    try:
        ref = eng.forward_u8(cubic)
        probs = eng.forward_images(imgs, 36)
        assert same_bits(probs, ref) and not same_bits(probs, bilinear_probs)
        assert same_bits(forward_images(eng, DeviceImages(imgs)), ref)
        assert same_bits(eng.features_images(imgs, 36, "cls"), eng.features_u8(cubic, "cls"))
        assert same_bits(eng.cls_attention_images(imgs, 36, "head_mean"), eng.cls_attention_u8(cubic, "head_mean"))
        assert same_bits(eng.intermediate_images(imgs, 36, [1], "tokens"), eng.intermediate_u8(cubic, [1], "tokens"))
    finally:
        eng.set_resize_filter("bilinear")
    assert same_bits(eng.forward_images(imgs, 36), bilinear_probs)


def test_setter_refuses_unknown_values_and_an_over_limit_record_names_the_image(engines):
    L = B.lib()
    eng = engines("tiny", max_batch=4)
    cfg, n = eng.cfg, 6
    imgs = random_images(engine_sizes(cfg, n, 901), 3, 901)
    dev = DeviceImages(imgs)
    t = dev.triples
    poison = np.full((n, cfg.num_classes), 0x7FC0BEEF, np.uint32).view(np.float32)
    pp = B.preproc_params(36, *CONSTS, 3)
    try:
        for start in (BILINEAR, BICUBIC):
            assert L.vit_engine_set_resize_filter(eng._h, start) == 0
            for bad in (2, -1, 7):
                assert L.vit_engine_set_resize_filter(eng._h, bad) == VIT_ERR_ARG
                assert L.vit_engine_last_error(eng._h)
                assert L.vit_engine_get_resize_filter(eng._h) == start
        with pytest.raises(KeyError):
            eng.set_resize_filter("lanczos")
        assert eng.get_resize_filter() == "bicubic"
        ref = forward_u8(eng, model_bytes(cfg, imgs))
        over = B.image_records(t[:3] + [(t[3][0], LIMIT * 36 + 1, LIMIT * 36 + 1)] + t[4:])
        d_p = B.DeviceArray.from_numpy(poison)
        assert L.vit_engine_forward_device_images(eng._h, over, n, C.byref(pp), d_p.ptr, None, None, None) == VIT_ERR_ARG
        assert b"image 3" in L.vit_engine_last_error(eng._h)
        eng.sync()
        assert same_bits(d_p.numpy(), poison)
        assert same_bits(forward_images(eng, dev), ref)  # the engine goes on working, still bicubic
    finally:
        eng.set_resize_filter("bilinear")
