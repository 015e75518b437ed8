#!/usr/bin/env python3
"""Digests of everything the row kernels write, over a grid of shapes: two builds computed the same bits iff they print the same
tables (GPU box only).

    python3 tools/row_kernel_digests.py [--out FILE.md]
    VIT_HIP_LIBRARY=/path/to/another/libvit_mi355x.so python3 tools/row_kernel_digests.py      (that build's tables)

Every extern "C" launcher of csrc/vit_rowops.hip, vit_tap.hip, vit_pool.hip, vit_lnfold.hip (the row statistics and both finalizes)
and vit_topk.hip runs on inputs from a fixed seed; a table entry is the first 16 hex digits of the SHA-256 over the output buffers
of one group of launches on one cell, workspaces excluded, pad columns of a padded output excluded (they are preset to zero and not
the launch's to write).

row table   dim x tokens x images, dense and with every leading dimension = dim + 12 (rows = images * tokens):
    ln       vithip_layernorm_f32, vithip_layernorm_f32_bf16out
    tap      vithip_tap_f32: CLS, TOKENS, PATCHES, MAP, each with and without the LayerNorm
    lnpool   vithip_layernorm_pool_f32: first_tok 0 and 1, l2_normalize 0 and 1
    poolln   vithip_pool_layernorm_f32: first_tok 0 and 1, with gamma / beta and without
    l2       vithip_l2_normalize_rows_f32
    rs_f32   vithip_rowstats_f32 (dim % 64 == 0 only)
    rs_bf16  vithip_rowstats_bf16: the bf16 copy and the statistics
    fin      vithip_rowstats_finalize on 4 * ceil(dim / 256) strips, vithip_rowstats_finalize_f32 on dim / 64 (dim % 64 == 0 only)
softmax table   classes x rows, dense and with ld_logits = ld_probs = classes + 12:
    top1     vithip_softmax_top1_f32: probabilities, labels, top-1 probabilities
    prob_kK / logit_kK   vithip_softmax_topk_f32 (k <= classes); 4099 classes take the path that recomputes a row per round
"""
import argparse
import ctypes as C
import hashlib
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DIMS = (64, 132, 192, 768, 1024, 1280, 2048)
TOKENS = (2, 17, 18, 50, 197)
IMAGES = (1, 3, 7)
CLASSES = (5, 257, 1000, 4099)
KS = (1, 5, 64)
PAD = 12
SEED = 20

P, Z, I = C.c_void_p, C.c_size_t, C.c_int
ARGTYPES = {
    "vithip_layernorm_f32": [P, P, Z, P, Z, P, P, I, I],
    "vithip_layernorm_f32_bf16out": [P, P, Z, P, Z, P, P, I, I],
    "vithip_tap_f32": [P, P, Z, P, Z, P, P, I, I, I, I],
    "vithip_layernorm_pool_f32": [P, P, Z, P, Z, P, P, I, I, I, I, I, P],
    "vithip_pool_layernorm_f32": [P, P, Z, P, Z, P, P, I, I, I, I, P],
    "vithip_l2_normalize_rows_f32": [P, P, Z, I, I],
    "vithip_rowstats_f32": [P, P, Z, P, I, I],
    "vithip_rowstats_bf16": [P, P, Z, P, Z, P, I, I],
    "vithip_rowstats_finalize": [P, P, I, I, I, P],
    "vithip_rowstats_finalize_f32": [P, P, I, I, P],
    "vithip_softmax_top1_f32": [P, P, I, P, I, P, P, I, I],
    "vithip_softmax_topk_f32": [P, P, I, P, I, I, I, I, I],
}


class Run:
    """Launches and the digest of what they wrote: out(...) makes an output (zeroed, or holding the rows of `init` for a launch that
    works in place), call(...) launches, digest() reads them all back."""

    def __init__(self, B):
        self.B, self.L, self.outs = B, B.lib(), []

    def out(self, rows, width, ld=None, dtype=np.float32, init=None):
        img = np.zeros((rows, width if ld is None else ld), dtype)
        if init is not None:
            img[:, :width] = init
        d = self.B.DeviceArray.from_numpy(img)
        self.outs.append((d, width))
        return d

    def call(self, name, *args):
        self.B.hip_check(getattr(self.L, name)(None, *args), name)

    def digest(self):
        h = hashlib.sha256()
        for d, width in self.outs:
            h.update(np.ascontiguousarray(d.numpy()[:, :width]).tobytes())
            d.free()
        self.outs = []
        return h.hexdigest()[:16]


def padded(B, a, ld):
    """a [rows][width] on the device with leading dimension ld; the pad columns hold a value no result survives."""
    img = np.full((a.shape[0], ld), 1e30, a.dtype)
    img[:, :a.shape[1]] = a
    return B.DeviceArray.from_numpy(img)


def row_cell(B, dim, tokens, images, pad):
    R, L = Run(B), B.lib()
    rng = np.random.default_rng([SEED, dim, tokens, images])
    rows, ld = images * tokens, dim + pad
    x = (rng.uniform(-1.5, 1.5, size=(rows, dim)) + rng.uniform(-1, 1, size=(rows, 1))).astype(np.float32)
    d_x = padded(B, x, ld)
    d_g = B.DeviceArray.from_numpy(rng.uniform(0.5, 1.5, dim).astype(np.float32))
    d_b = B.DeviceArray.from_numpy(rng.uniform(-0.5, 0.5, dim).astype(np.float32))
    res = {}

    R.call("vithip_layernorm_f32", d_x.ptr, ld, R.out(rows, dim, ld).ptr, ld, d_g.ptr, d_b.ptr, rows, dim)
    R.call("vithip_layernorm_f32_bf16out", d_x.ptr, ld, R.out(rows, dim, ld, np.uint16).ptr, ld, d_g.ptr, d_b.ptr, rows, dim)
    res["ln"] = R.digest()

    for layout, per_image in ((0, 1), (1, tokens), (2, tokens - 1), (3, tokens - 1)):  # VITHIP_TAP_CLS, _TOKENS, _PATCHES, _MAP
        for g, b in ((d_g.ptr, d_b.ptr), (None, None)):
            block = per_image * dim
            R.call("vithip_tap_f32", d_x.ptr, ld, R.out(images, block, block + pad).ptr, block + pad, g, b, images, tokens, dim, layout)
    res["tap"] = R.digest()

    d_ws = B.DeviceArray((max(1, L.vithip_layernorm_pool_f32_workspace_floats(images, tokens, 0, dim)),))
    for first_tok in (0, 1):
        for l2 in (0, 1):
            R.call("vithip_layernorm_pool_f32", d_x.ptr, ld, R.out(images, dim, ld).ptr, ld, d_g.ptr, d_b.ptr, images, tokens, first_tok,
                   dim, l2, d_ws.ptr)
    res["lnpool"] = R.digest()
    for first_tok in (0, 1):
        for g, b in ((d_g.ptr, d_b.ptr), (None, None)):
            R.call("vithip_pool_layernorm_f32", d_x.ptr, ld, R.out(images, dim, ld).ptr, ld, g, b, images, tokens, first_tok, dim, d_ws.ptr)
    res["poolln"] = R.digest()

    R.call("vithip_l2_normalize_rows_f32", R.out(rows, dim, ld, init=x).ptr, ld, rows, dim)
    res["l2"] = R.digest()

    res["rs_f32"] = "-"
    if dim % 64 == 0:
        R.call("vithip_rowstats_f32", d_x.ptr, ld, R.out(rows, 2).ptr, rows, dim)
        res["rs_f32"] = R.digest()
    R.call("vithip_rowstats_bf16", d_x.ptr, ld, R.out(rows, dim, ld, np.uint16).ptr, ld, R.out(rows, 2).ptr, rows, dim)
    res["rs_bf16"] = R.digest()

    # partials as a residual GEMM's epilogue leaves them: [strips][rows][2] = the sum and the sum of squares of a strip of columns
    strips = 4 * ((dim + 255) // 256)
    parts = np.stack([rng.uniform(-8, 8, (strips, rows)), rng.uniform(8, 40, (strips, rows))], axis=-1).astype(np.float32)
    d_p = B.DeviceArray.from_numpy(parts)
    R.call("vithip_rowstats_finalize", d_p.ptr, strips, rows, dim, R.out(rows, 2).ptr)
    if dim % 64 == 0:
        R.call("vithip_rowstats_finalize_f32", d_p.ptr, rows, dim, R.out(rows, 2).ptr)  # reads the first dim / 64 <= strips of them
    res["fin"] = R.digest()
    for d in (d_x, d_g, d_b, d_ws, d_p):
        d.free()
    return res


def softmax_cell(B, classes, rows, pad):
    R = Run(B)
    rng = np.random.default_rng([SEED, classes, rows])
    logits = (rng.standard_normal((rows, classes)) * 3).astype(np.float32)
    logits[:, classes // 2] = logits[:, 0]  # a tie per row
    ld = classes + pad
    d_l = padded(B, logits, ld)
    res = {}
    R.call("vithip_softmax_top1_f32", d_l.ptr, ld, R.out(rows, classes, ld).ptr, ld, R.out(rows, 1, dtype=np.int32).ptr, R.out(rows, 1).ptr,
           rows, classes)
    res["top1"] = R.digest()
    for name, score in (("prob", 0), ("logit", 1)):  # VITHIP_SCORE_PROB, VITHIP_SCORE_LOGIT
        for k in KS:
            res[f"{name}_k{k}"] = "-"
            if k <= classes:
                R.call("vithip_softmax_topk_f32", d_l.ptr, ld, R.out(rows, 2 * k, 2 * k + pad, np.int32).ptr, 2 * k + pad, rows, classes, k, score)
                res[f"{name}_k{k}"] = R.digest()
    d_l.free()
    return res


def table(emit, head, cells):
    cols = None
    for key, res in cells:
        if cols is None:
            cols = list(res)
            emit("| " + " | ".join(head + cols) + " |")
            emit("|" + "---|" * (len(head) + len(cols)))
        emit("| " + " | ".join([str(k) for k in key] + [res[c] for c in cols]) + " |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    a = ap.parse_args()
    B = importlib.import_module("vision-transformer-opencl_amd.binding")
    L = B.lib()
    for name, types in ARGTYPES.items():
        getattr(L, name).argtypes = types
    out = open(a.out, "w") if a.out else None

    def emit(line):
        print(line, flush=True)
        if out:
            out.write(line + "\n")

    table(emit, ["dim", "tokens", "images", "ld"],
          (((dim, tokens, images, dim + pad), row_cell(B, dim, tokens, images, pad))
           for dim in DIMS for tokens in TOKENS for images in IMAGES for pad in (0, PAD)))
    emit("")
    table(emit, ["classes", "rows", "ld"],
          (((classes, rows, classes + pad), softmax_cell(B, classes, rows, pad)) for classes in CLASSES for rows in IMAGES for pad in (0, PAD)))


if __name__ == "__main__":
    main()
