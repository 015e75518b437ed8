"""Resize + CenterCrop on the host (no GPU): the numpy restatement (tests/preproc_model.py) that tests/test_gpu_preproc.py compares
the device against, held bit for bit against Pillow itself (where Pillow is installed) and against Pillow's recorded output
(tests/golden/preproc_pillow.npz, written by tools/gen_preproc_golden.py); the geometry against torchvision's formulas worked out
by hand; the C-ABI symbols of the feature.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import preproc_model as M
from vit_amd import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "preproc_pillow.npz")

SOURCES = [(480, 640), (640, 480), (375, 500), (500, 333), (256, 256), (224, 224), (100, 130), (31, 517), (1080, 1920), (257, 255),
           (300, 256), (2000, 300), (17, 17), (511, 513)]
PAIRS = [(256, 224), (224, 224), (438, 384), (232, 224)]

NEW_SYMBOLS = ("vithip_images_u8_resize_crop_to_f32", "vit_engine_forward_device_images", "vit_engine_forward_host_images",
               "vit_engine_features_device_images", "vit_engine_features_host_images")


def random_image(h, w, seed, chans=3):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, chans), dtype=np.uint8)


def gradient_image(h, w):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    chans = [255.0 * x / max(w - 1, 1), 255.0 * y / max(h - 1, 1), 127.5 + 127.5 * np.sin(x / 11.0 + y / 7.0)]
    return np.clip(np.rint(np.stack(chans, -1)), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("R,S", PAIRS)
@pytest.mark.parametrize("h,w", SOURCES)
def test_restatement_equals_pillow(h, w, R, S):
    Image = pytest.importorskip("PIL.Image")
    oh, ow = M.resized_size(h, w, R)
    top, left = M.crop_origin(oh, ow, S)
    for src in (random_image(h, w, h * 10007 + w + R), gradient_image(h, w)):
        ref = np.asarray(Image.fromarray(src).resize((ow, oh), Image.BILINEAR))
        assert np.array_equal(M.resize(src, oh, ow), ref)
        assert np.array_equal(M.resize_crop(src, R, S), ref[top:top + S, left:left + S])


def test_restatement_equals_the_recorded_pillow_output():
    g = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 300 * 1024
    n = sum(1 for k in g.files if k.startswith("src_"))
    assert n >= 10
    seen_identity = False
    for i in range(n):
        src = g[f"src_{i}"]
        assert 9 <= min(src.shape[:2]) and max(src.shape[:2]) <= 120
        for R, S in g["pairs"]:
            ref = g[f"out_{i}_{R}"]
            oh, ow = M.resized_size(src.shape[0], src.shape[1], int(R))
            assert ref.shape == (oh, ow, 3)
            assert np.array_equal(M.resize(src, oh, ow), ref), (i, int(R))
            if src.shape[0] == src.shape[1] == R:
                seen_identity = True
                assert np.array_equal(ref, src)  # nothing to resize: the bytes pass through
    assert seen_identity


def test_geometry_is_torchvisions():
    assert M.resized_size(375, 500, 256) == (256, 341) and M.crop_origin(256, 341, 224) == (16, 58)  # 58.5 rounds to even
    assert M.resized_size(500, 333, 256) == (384, 256) and M.crop_origin(384, 256, 224) == (80, 16)
    assert M.resized_size(257, 255, 224) == (225, 224) and M.crop_origin(225, 224, 224) == (0, 0)    # 0.5 rounds to 0
    assert M.resized_size(31, 517, 256) == (256, 4269)
    assert M.resized_size(224, 224, 224) == (224, 224) and M.crop_origin(224, 224, 224) == (0, 0)
    # torchvision computes int(R * long / short) in Python floats: the same integers over a sweep of sizes
    rng = np.random.default_rng(3)
    for _ in range(20000):
        short, long_ = sorted(int(v) for v in rng.integers(1, 16385, size=2))
        R = int(rng.integers(4, 4097))
        assert (R * long_) // short == int(R * long_ / short)


def test_a_float_blend_with_one_rounding_differs():
    """The comparison can fail: both axes blended in floating point and rounded once are other bits than Pillow's two byte passes."""
    g = np.load(GOLDEN)
    differs = 0
    for i in range(sum(1 for k in g.files if k.startswith("src_"))):
        src = g[f"src_{i}"]
        for R, _ in g["pairs"]:
            ref = g[f"out_{i}_{R}"]
            oh, ow = ref.shape[:2]
            acc = np.zeros((oh, ow, 3), np.float64)
            for y, (ymin, ky) in enumerate(M.coeffs(src.shape[0], oh)):
                rows = np.tensordot(ky / 4194304.0, src[ymin:ymin + len(ky)].astype(np.float64), axes=(0, 0))  # [W][3]
                for x, (xmin, kx) in enumerate(M.coeffs(src.shape[1], ow)):
                    acc[y, x] = (kx / 4194304.0) @ rows[xmin:xmin + len(kx)]
            one = np.clip(np.floor(acc + 0.5), 0, 255).astype(np.uint8)
            differs += int(not np.array_equal(one, ref))
    assert differs > 0


def test_preprocess_is_the_u8_normalisation_when_nothing_is_resized():
    from test_input_u8_model import normalise_u8
    imgs = [random_image(32, 32, 5), random_image(32, 32, 6)]
    got = M.preprocess(imgs, 32, 32, B.IMAGENET_MEAN, B.IMAGENET_STD)
    assert np.array_equal(got.view(np.uint32), normalise_u8(np.stack(imgs), B.IMAGENET_MEAN, B.IMAGENET_STD).view(np.uint32))


def test_product_library_exports_the_preprocessing_entry_points():
    product = os.path.join(os.path.dirname(B.LIB_PATH), "libvit_mi355x.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", product], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
    assert set(NEW_SYMBOLS) <= names
    L = B.lib()
    for fn in NEW_SYMBOLS:
        assert getattr(L, fn).argtypes, fn


def test_record_mirrors_have_the_layout_of_the_headers(tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "vit_engine.h"', '#include "vit_hip_kernels.h"', "int main(void) {",
             '    printf("image %zu %zu %zu %zu\\n", sizeof(vit_image_u8), offsetof(vit_image_u8, pixels), offsetof(vit_image_u8, height), '
             "offsetof(vit_image_u8, width));",
             '    printf("kimage %zu %zu %zu %zu\\n", sizeof(vithip_image_u8), offsetof(vithip_image_u8, pixels), '
             "offsetof(vithip_image_u8, height), offsetof(vithip_image_u8, width));",
             '    printf("preproc %zu %zu %zu %zu\\n", sizeof(vit_preproc), offsetof(vit_preproc, resize_shorter), offsetof(vit_preproc, mean), '
             "offsetof(vit_preproc, std));",
             "    return 0;", "}"]
    src, exe = tmp_path / "rec.c", tmp_path / "rec"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True,
                   text=True)
    out = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in
           subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()}
    I, P = B.CImageU8, B.CPreproc
    assert out["image"] == out["kimage"] == [C.sizeof(I), I.pixels.offset, I.height.offset, I.width.offset]
    assert out["preproc"] == [C.sizeof(P), P.resize_shorter.offset, P.mean.offset, P.std.offset]
