"""Resize with a chosen filter on the host (no GPU): the numpy restatement (tests/preproc_filter_model.py) that
tests/test_gpu_preproc_bicubic.py compares the device against.  Its bicubic case is held bit for bit against Pillow's recorded output
(tests/golden/preproc_pillow_bicubic.npz, written by tools/gen_preproc_bicubic_golden.py) and against Pillow itself where it is
installed; its bilinear case against tests/preproc_model.py; the tap bound the kernel sizes its tables by against the tables; and
the sources are shown to drive both passes out of [0, 255] on both sides, without which a kernel that forgot the low clamp would pass.
"""
import os

import numpy as np
import pytest

import preproc_filter_model as F
import preproc_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "preproc_pillow_bicubic.npz")
OLD_GOLDEN = os.path.join(ROOT, "tests", "golden", "preproc_pillow.npz")
LIMIT = 64  # a source's shorter side is at most LIMIT x resize_shorter, for both filters (include/vit_hip_kernels.h)

# (H, W, kind, (oh, ow)): up- and down-scale on either axis, one axis kept, 1-pixel-wide sources, a large one
PILLOW_CASES = [(375, 500, "random", (256, 341)), (500, 333, "binary", (384, 256)), (100, 130, "binary", (256, 332)),
                (31, 517, "random", (36, 600)), (257, 255, "binary", (225, 224)), (17, 17, "binary", (72, 72)),
                (1, 9, "binary", (36, 324)), (11, 1, "random", (396, 36)), (300, 256, "binary", (300, 224)),
                (224, 300, "random", (256, 300)), (1153, 1200, "binary", (36, 37)), (64, 48, "binary", (700, 525))]


def source(h, w, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "binary":
        return (rng.integers(0, 2, size=(h, w, 3), dtype=np.uint8) * 255).astype(np.uint8)
    return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def golden_sources(g):
    return [g[f"src_{i}"] for i in range(sum(1 for k in g.files if k.startswith("src_")))]


def is_binary(src):
    return bool(np.isin(src, (0, 255)).all()) and src.min() != src.max()


def test_bicubic_restatement_equals_the_recorded_pillow_output():
    g = np.load(GOLDEN)
    # the ten sources and two pairs of preproc_pillow.npz (292 KB: resized bytes barely compress) plus two binary ones: 13 / 10 of it
    assert os.path.getsize(GOLDEN) < 390 * 1024 and str(g["pillow_version"])
    srcs = golden_sources(g)
    old = np.load(OLD_GOLDEN)
    assert np.array_equal(g["pairs"], old["pairs"])
    for i, s in enumerate(golden_sources(old)):  # the sources of the bilinear file first, then the binary ones
        assert np.array_equal(srcs[i], s)
    binary = [s for s in srcs[len(golden_sources(old)):] if is_binary(s)]
    Rs = [int(R) for R, _ in g["pairs"]]
    assert any(min(s.shape[:2]) < min(Rs) for s in binary) and any(min(s.shape[:2]) > max(Rs) for s in binary)  # up- and down-scaled
    differs = 0
    for i, src in enumerate(srcs):
        for R in Rs:
            ref = g[f"out_{i}_{R}"]
            oh, ow = M.resized_size(src.shape[0], src.shape[1], R)
            assert ref.shape == (oh, ow, 3)
            assert np.array_equal(F.resize(src, oh, ow, F.BICUBIC), ref), (i, R)
            differs += int(not np.array_equal(ref, M.resize(src, oh, ow)))
            if src.shape[0] == src.shape[1] == R:
                assert np.array_equal(ref, src)  # nothing to resize: the bytes pass through
    assert differs >= len(srcs)  # the comparison can fail: bilinear gives other bytes


@pytest.mark.parametrize("h,w,kind,size", PILLOW_CASES)
def test_bicubic_restatement_equals_pillow(h, w, kind, size):
    Image = pytest.importorskip("PIL.Image")
    src = source(h, w, kind, 7 * h + w)
    ref = np.asarray(Image.fromarray(src).resize((size[1], size[0]), Image.BICUBIC))
    assert np.array_equal(F.resize(src, size[0], size[1], F.BICUBIC), ref)


def test_bilinear_case_is_the_old_restatement():
    old = np.load(OLD_GOLDEN)
    for i, src in enumerate(golden_sources(old)):
        for R, S in old["pairs"]:
            oh, ow = M.resized_size(src.shape[0], src.shape[1], int(R))
            assert np.array_equal(F.resize(src, oh, ow, F.BILINEAR), M.resize(src, oh, ow)), (i, int(R))
            assert np.array_equal(F.resize_crop(src, int(R), int(S)), M.resize_crop(src, int(R), int(S)))
    for inn, out in [(50, 36), (36, 72), (17, 23), (120, 36), (9, 40)]:
        for (a, ka), (b, kb) in zip(F.coeffs(inn, out, F.BILINEAR), M.coeffs(inn, out)):
            assert a == b and np.array_equal(ka, kb)
    imgs = [source(40, 50, "random", 1), source(33, 37, "binary", 2)]
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    assert np.array_equal(F.preprocess(imgs, 36, 32, mean, std).view(np.uint32), M.preprocess(imgs, 36, 32, mean, std).view(np.uint32))


def limit_pairs():
    """(in, out) of both axes of sources at the size limit: the shorter side LIMIT x R, the longer one where its scale is largest
    (just below the length that gives the resized longer side one more pixel)."""
    out = []
    for R in (4, 32, 36, 224):
        short = LIMIT * R
        if short <= 16384:
            out.append((short, R))
            long_ = min((short * (R + 1) - 1) // R, 16384)
            out.append((long_, (R * long_) // short))
    return out


@pytest.mark.parametrize("filter", [F.BILINEAR, F.BICUBIC])
def test_no_index_has_more_taps_than_the_bound(filter):
    most = 0.0
    pairs = [(i, o) for i in range(1, 41) for o in range(1, 41) if i != o] + limit_pairs()
    for inn, out in pairs:
        bound = F.tap_bound(inn, out, filter)
        if filter == F.BICUBIC:
            assert bound == int(4 * max(inn / out, 1.0)) + 2
        worst = max(len(k) for _, k in F.coeffs(inn, out, filter))
        assert worst <= bound, (inn, out)
        most = max(most, worst / bound)
    assert most > 0.8  # and the bound is not idle
    # the largest bound the launcher's limit allows is what the kernel's coefficient tables are sized for: 6 columns of 322 in 2048
    assert max(F.tap_bound(i, o, F.BICUBIC) for i, o in limit_pairs()) <= 322 and F.tap_bound(4 * 80 - 1, 4, F.BICUBIC) <= 322


def test_the_sources_clamp_low_and_high_in_both_passes():
    """A source set that never leaves [0, 255] would hide a kernel without the low clamp: the golden sources and the binary sources
    of the GPU test (every third image of random_images there) do, in each pass direction, thousands of times."""
    g = np.load(GOLDEN)
    counts = {}
    for src in golden_sources(g):
        for R, _ in g["pairs"]:
            oh, ow = M.resized_size(src.shape[0], src.shape[1], int(R))
            F.resize(src, oh, ow, F.BICUBIC, counts)
    for direction in ("h", "v"):
        assert counts[direction]["low"] >= 1000 and counts[direction]["high"] >= 1000, counts
    c = {}  # one up-scaled binary source alone does (a down-scaled one averages its noise away before the vertical pass)
    F.resize(source(24, 31, "binary", 3), 36, 46, F.BICUBIC, c)
    assert min(c["h"]["low"], c["h"]["high"], c["v"]["low"], c["v"]["high"]) >= 100, c
    # bilinear never does: its coefficients are non-negative and sum to 2^22 within a rounding
    c = {}
    F.resize(source(110, 87, "binary", 3), 45, 36, F.BILINEAR, c)
    assert c["h"]["low"] == c["v"]["low"] == 0
