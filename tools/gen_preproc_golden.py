"""Writes tests/golden/preproc_pillow.npz: small 8-bit sources and Pillow's own bilinear resize of each, for the two (resize, crop)
pairs of the small test models.  CPU only; needs Pillow.  tests/test_preproc_model.py holds the numpy restatement
(tests/preproc_model.py) against this file, so that a machine without Pillow still checks the restatement against Pillow's bits.

    python tools/gen_preproc_golden.py [out.npz]

Keys: src_<i> uint8 [H][W][3]; out_<i>_<R> uint8 [oh][ow][3] = Image.resize((ow, oh), BILINEAR) with (oh, ow) torchvision's
Resize(R) geometry; pairs int32 [[R, S], ...]; pillow_version.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(36, 32), (72, 64)]  # VIT_TINY / VIT_SMALL crops
# (H, W, kind): both orientations, a square, H == W == R for each pair, up- and down-scaling, odd sizes, a thin one each way
# (random bytes do not compress: most of the larger ones are smooth, so that the file stays small)
SOURCES = [(50, 70, "random"), (36, 36, "random"), (72, 72, "gradient"), (40, 30, "gradient"), (120, 90, "gradient"),
           (33, 50, "gradient"), (9, 12, "random"), (17, 23, "random"), (23, 17, "gradient"), (20, 20, "gradient")]


def resized_size(h, w, R):
    short, long = (w, h) if w <= h else (h, w)
    new_long = int(R * long / short)  # torchvision's own expression
    return (new_long, R) if w <= h else (R, new_long)


def make_source(h, w, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    chans = [255.0 * x / max(w - 1, 1), 255.0 * y / max(h - 1, 1), 127.5 + 127.5 * np.sin(x / 23.0 + y / 17.0)]
    return np.clip(np.rint(np.stack(chans, -1)), 0, 255).astype(np.uint8)


def main(out_path):
    import PIL
    from PIL import Image

    arrays = {"pairs": np.asarray(PAIRS, np.int32), "pillow_version": np.asarray(PIL.__version__)}
    for i, (h, w, kind) in enumerate(SOURCES):
        src = make_source(h, w, kind, 1000 + i)
        arrays[f"src_{i}"] = src
        for R, _ in PAIRS:
            oh, ow = resized_size(h, w, R)
            arrays[f"out_{i}_{R}"] = np.asarray(Image.fromarray(src).resize((ow, oh), Image.BILINEAR))
    np.savez_compressed(out_path, **arrays)
    print(f"{out_path}: {len(SOURCES)} sources, {os.path.getsize(out_path)} bytes, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "preproc_pillow.npz"))
