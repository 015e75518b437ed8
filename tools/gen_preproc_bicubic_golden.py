"""Writes tests/golden/preproc_pillow_bicubic.npz: small 8-bit sources and Pillow's own BICUBIC resize of each, for the two (resize, crop)
pairs of the small test models.  CPU only; needs Pillow.  tests/test_preproc_filter_model.py holds the numpy restatement
(tests/preproc_filter_model.py) against this file, so that a machine without Pillow still checks the restatement against Pillow's bits.

    python tools/gen_preproc_bicubic_golden.py [out.npz]

The layout of preproc_pillow.npz (tools/gen_preproc_golden.py), its (R, S) pairs and its sources, plus binary 0 / 255 noise sources:
the bicubic coefficients are signed, and only hard edges drive the sums of a pass below 0 and above 255 often (thousands of times in
these; smooth and uniformly random sources barely do).  One of them is up-scaled by both pairs, one down-scaled by both.
Size: the outputs are bytes that barely compress (the bilinear file with the same ten sources has 292 KB), so the file has about 350 KB.
Keys: src_<i> uint8 [H][W][3]; out_<i>_<R> uint8 [oh][ow][3] = Image.resize((ow, oh), BICUBIC) with (oh, ow) torchvision's Resize(R)
geometry; pairs int32 [[R, S], ...]; pillow_version.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from gen_preproc_golden import PAIRS, SOURCES, make_source, resized_size  # noqa: E402

# (H, W): up-scaled by both pairs, down-scaled by both
BINARY_SOURCES = [(24, 31), (110, 87)]


def binary_source(h, w, seed):
    return (np.random.default_rng(seed).integers(0, 2, size=(h, w, 3), dtype=np.uint8) * 255).astype(np.uint8)


def sources():
    out = [make_source(h, w, kind, 1000 + i) for i, (h, w, kind) in enumerate(SOURCES)]
    return out + [binary_source(h, w, 2000 + i) for i, (h, w) in enumerate(BINARY_SOURCES)]


def main(out_path):
    import PIL
    from PIL import Image

    arrays = {"pairs": np.asarray(PAIRS, np.int32), "pillow_version": np.asarray(PIL.__version__)}
    for i, src in enumerate(sources()):
        arrays[f"src_{i}"] = src
        for R, _ in PAIRS:
            oh, ow = resized_size(src.shape[0], src.shape[1], R)
            arrays[f"out_{i}_{R}"] = np.asarray(Image.fromarray(src).resize((ow, oh), Image.BICUBIC))
    np.savez_compressed(out_path, **arrays)
    print(f"{out_path}: {len(arrays) - 2} arrays, {os.path.getsize(out_path)} bytes, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "preproc_pillow_bicubic.npz"))
