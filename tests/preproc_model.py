"""Resize(R) + CenterCrop(S) + ToTensor() + Normalize(mean, std) restated in numpy (helper, no tests in it).

The arithmetic of torchvision's evaluation transform on 8-bit images, i.e. Pillow's Image.resize(..., BILINEAR): a coefficient table
in double precision, 2^22 fixed-point coefficients, int32 accumulation, the horizontal pass rounded to bytes before the vertical one.
tests/test_preproc_model.py proves it against Pillow; tests/test_gpu_preproc.py compares the device against it.
"""
import numpy as np

from test_input_u8_model import normalise_u8

PRECISION_BITS = 22


def resized_size(h: int, w: int, R: int):
    """(oh, ow) of torchvision's Resize(R) with an int: the shorter side becomes R, the longer one floor(R * long / short)."""
    short, long = (w, h) if w <= h else (h, w)
    new_long = (R * long) // short
    return (new_long, R) if w <= h else (R, new_long)


def crop_origin(oh: int, ow: int, S: int):
    """(top, left) of torchvision's CenterCrop(S): int(round((o - S) / 2.0)), Python's round (half to even)."""
    return int(round((oh - S) / 2.0)), int(round((ow - S) / 2.0))


def coeffs(in_size: int, out_size: int):
    """Pillow's precompute_coeffs for the bilinear filter: per output index (xmin, int32 coefficients k[0..cnt))."""
    scale = float(in_size) / float(out_size)
    fs = max(scale, 1.0)
    support = fs
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
            a = abs((x + xmin - center + 0.5) * ss)
            v = 1.0 - a if a < 1.0 else 0.0
            w.append(v)
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        table.append((xmin, np.array([int(0.5 + v * float(1 << PRECISION_BITS)) for v in w], np.int32)))
    return table


def _pass(src: np.ndarray, table, axis: int) -> np.ndarray:
    """One fixed-point pass along `axis` (0: vertical, 1: horizontal) of src [H][W][C] uint8."""
    src = np.moveaxis(src, axis, 0).astype(np.int32)
    out = np.empty((len(table),) + src.shape[1:], np.uint8)
    for i, (xmin, k) in enumerate(table):
        acc = np.int32(1 << (PRECISION_BITS - 1)) + np.tensordot(k, src[xmin:xmin + len(k)], axes=(0, 0)).astype(np.int32)
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(src: np.ndarray, oh: int, ow: int) -> np.ndarray:
    """Pillow's Image.resize((ow, oh), BILINEAR) of src [H][W][C] uint8: horizontal pass, bytes, vertical pass; an axis whose
    size does not change is skipped."""
    src = np.ascontiguousarray(src, np.uint8)
    h, w = src.shape[:2]
    if ow != w:
        src = _pass(src, coeffs(w, ow), 1)
    if oh != h:
        src = _pass(src, coeffs(h, oh), 0)
    return np.ascontiguousarray(src)


def resize_crop(src: np.ndarray, R: int, S: int) -> np.ndarray:
    """uint8 [H][W][C] -> uint8 [S][S][C]: Resize(R), CenterCrop(S)."""
    oh, ow = resized_size(src.shape[0], src.shape[1], R)
    top, left = crop_origin(oh, ow, S)
    return np.ascontiguousarray(resize(src, oh, ow)[top:top + S, left:left + S])


def preprocess(images, R: int, S: int, mean, std) -> np.ndarray:
    """list of uint8 [H][W][C] -> fp32 [n][C][S][S], the whole transform."""
    return normalise_u8(np.stack([resize_crop(im, R, S) for im in images]), mean, std)
