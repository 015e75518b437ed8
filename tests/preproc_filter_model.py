"""Resize(R, interpolation=filter) + CenterCrop(S) + ToTensor() + Normalize(mean, std) restated in numpy, the filter chosen (helper, no
tests in it).

Pillow's Image.resize(..., BILINEAR | BICUBIC) on 8 bits per channel: a coefficient table in double precision, 2^22 fixed-point
coefficients, int32 accumulation, the horizontal pass rounded to bytes before the vertical one.  The bilinear case is
tests/preproc_model.py to the bit (that file stays as it is); bicubic has twice the support, Keys' cubic with a = -0.5, signed
coefficients rounded away from zero, and passes that leave [0, 255] on both sides.  tests/test_preproc_filter_model.py proves it
against Pillow; tests/test_gpu_preproc_bicubic.py compares the device against it.
"""
import numpy as np

from preproc_model import PRECISION_BITS, crop_origin, resized_size  # noqa: F401 (the geometry does not depend on the filter)
from test_input_u8_model import normalise_u8

BILINEAR, BICUBIC = "bilinear", "bicubic"
FILTER_SUPPORT = {BILINEAR: 1.0, BICUBIC: 2.0}


def bilinear_weight(x: float) -> float:
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def bicubic_weight(x: float) -> float:
    """Pillow's bicubic_filter: every operation a double one, in this order."""
    a = -0.5
    t = abs(x)
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    if t < 2.0:
        return (((t - 5) * t + 8) * t - 4) * a
    return 0.0


FILTER_WEIGHT = {BILINEAR: bilinear_weight, BICUBIC: bicubic_weight}


def tap_bound(in_size: int, out_size: int, filter: str = BILINEAR) -> int:
    """The most taps an output index may have: (int)(2 * support) + 2, support = FILTER_SUPPORT * max(scale, 1)."""
    fs = max(float(in_size) / float(out_size), 1.0)
    return int(2.0 * FILTER_SUPPORT[filter] * fs) + 2


def coeffs(in_size: int, out_size: int, filter: str = BILINEAR):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc: per output index (xmin, int32 coefficients k[0..cnt))."""
    weight = FILTER_WEIGHT[filter]
    scale = float(in_size) / float(out_size)
    fs = max(scale, 1.0)
    support = FILTER_SUPPORT[filter] * fs
    ss = 1.0 / fs
    table = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        cnt = xmax - xmin
        w = []
        ww = 0.0
        for x in range(cnt):
            v = weight((x + xmin - center + 0.5) * ss)
            w.append(v)
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        one = float(1 << PRECISION_BITS)
        table.append((xmin, np.array([int(-0.5 + v * one) if v < 0 else int(0.5 + v * one) for v in w], np.int32)))
    return table


def _pass(src: np.ndarray, table, axis: int, clamps=None) -> np.ndarray:
    """One fixed-point pass along `axis` (0: vertical, 1: horizontal) of src [H][W][C] uint8.  clamps: a dict that counts the sums
    below 0 ("low") and above 255 ("high")."""
    src = np.moveaxis(src, axis, 0)
    out = np.empty((len(table),) + src.shape[1:], np.uint8)
    for i, (xmin, k) in enumerate(table):
        # summed in double, which is exact here (every partial sum is an integer below 2^53), then as integers
        dot = np.tensordot(k.astype(np.float64), src[xmin:xmin + len(k)].astype(np.float64), axes=(0, 0))
        acc = (1 << (PRECISION_BITS - 1)) + dot.astype(np.int64)
        assert -2 ** 31 <= acc.min() and acc.max() < 2 ** 31  # Pillow and the kernel sum in int32
        b = acc >> PRECISION_BITS
        if clamps is not None:
            clamps["low"] = clamps.get("low", 0) + int((b < 0).sum())
            clamps["high"] = clamps.get("high", 0) + int((b > 255).sum())
        out[i] = np.clip(b, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(src: np.ndarray, oh: int, ow: int, filter: str = BILINEAR, clamps=None) -> np.ndarray:
    """Pillow's Image.resize((ow, oh), filter) of src [H][W][C] uint8: horizontal pass, bytes, vertical pass; an axis whose size
    does not change is skipped.  clamps: {"h": {}, "v": {}} to count the clamped sums of each pass."""
    src = np.ascontiguousarray(src, np.uint8)
    h, w = src.shape[:2]
    if ow != w:
        src = _pass(src, coeffs(w, ow, filter), 1, None if clamps is None else clamps.setdefault("h", {}))
    if oh != h:
        src = _pass(src, coeffs(h, oh, filter), 0, None if clamps is None else clamps.setdefault("v", {}))
    return np.ascontiguousarray(src)


def resize_crop(src: np.ndarray, R: int, S: int, filter: str = BILINEAR, clamps=None) -> np.ndarray:
    """uint8 [H][W][C] -> uint8 [S][S][C]: Resize(R, filter), CenterCrop(S).  clamps: as for resize (of the whole resized image)."""
    oh, ow = resized_size(src.shape[0], src.shape[1], R)
    top, left = crop_origin(oh, ow, S)
    return np.ascontiguousarray(resize(src, oh, ow, filter, clamps)[top:top + S, left:left + S])


def preprocess(images, R: int, S: int, mean, std, filter: str = BILINEAR, clamps=None) -> np.ndarray:
    """list of uint8 [H][W][C] -> fp32 [n][C][S][S], the whole transform."""
    return normalise_u8(np.stack([resize_crop(im, R, S, filter, clamps) for im in images]), mean, std)
