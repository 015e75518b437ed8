#!/usr/bin/env python3
"""Digests of everything the attention entries write, over a grid that reaches every route and edge of the kernels: two builds
computed the same bits, and refuse the same calls, iff they print the same tables (GPU box only).

    python3 tools/attention_digests.py [--out FILE.md]
    VIT_HIP_LIBRARY=/path/to/another/libvit_mi355x.so python3 tools/attention_digests.py      (that build's tables)

Inputs come from a fixed seed, U(-1.5, 1.5), bf16 inputs are the same values rounded; q_scaled calls read the same bits.  A table
entry is the first 16 hex digits of the SHA-256 over the whole output buffers of one group of calls on one cell (preset to a
sentinel, so what a call leaves unwritten counts too); a call that is refused puts its return code into the digest instead, and
the entry ends in /rN when N calls of its group were refused.  heads = 3 everywhere.

P.V, head_dim 64   tokens x images; q_rows = tokens and 1 where the entry takes it
    f32 f32_rows bf16io bf16io_rows qscaled f32math   the vithip_attention_* entry of that name
    f32_hd bf16io_hd                                  the _hd entries with head_dim 64 (bf16io_hd: q_scaled 0 and 1)
P.V, head dims 72..128   head_dim x tokens x images; q_rows = tokens and 1
    f32 bf16 bf16_qs   vithip_attention_f32_hd, vithip_attention_bf16io_hd with q_scaled 0 and 1
class row   head_dim x tokens x images x ld_out (dense, and the row + 12); head_mean 0 and 1
    f32 bf16 bf16_qs   vithip_cls_attention_f32_hd, vithip_cls_attention_bf16_hd with q_scaled 0 and 1; at head_dim 64 also
                       vithip_cls_attention_f32 / _bf16
refusals   every call of a list of bad arguments (head dims 0, 32, 56, 68, 136; q_rows 0 and tokens + 1; q_scaled 2; q_rows < tokens,
    and the _rows entries, at 225 tokens and head_dim 64; heads = 65536 at head_dim 80; null pointers; pointers off by 4 bytes) must
    return hipErrorInvalidValue: the line counts them and names those that returned something else.
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

HEADS = 3
IMAGES = (1, 3)
TOKENS_64 = (1, 17, 33, 197, 224, 225, 577, 704, 705)
DIMS_HD, TOKENS_HD = (72, 80, 104, 128), (1, 33, 65, 257)
DIMS_CLS, TOKENS_CLS = (64, 72, 104, 128), (1, 17, 197, 4099)  # 4099: past the 4096 scores the class-row kernel keeps in LDS
PAD = 12
SEED = 22
INVALID_VALUE = 1  # hipErrorInvalidValue

P, Z, I = C.c_void_p, C.c_size_t, C.c_int
PV, CLS = [P, P, P], [P, P, Z, P, Z]
ARGTYPES = {
    "vithip_attention_f32": PV + [I] * 3, "vithip_attention_bf16io": PV + [I] * 3, "vithip_attention_bf16io_f32math": PV + [I] * 3,
    "vithip_attention_f32_rows": PV + [I] * 4, "vithip_attention_bf16io_rows": PV + [I] * 4, "vithip_attention_bf16io_qscaled": PV + [I] * 4,
    "vithip_attention_f32_hd": PV + [I] * 5, "vithip_attention_bf16io_hd": PV + [I] * 6,
    "vithip_cls_attention_f32": CLS + [I] * 4, "vithip_cls_attention_bf16": CLS + [I] * 5,
    "vithip_cls_attention_f32_hd": CLS + [I] * 5, "vithip_cls_attention_bf16_hd": CLS + [I] * 6,
}


class Group:
    """The calls of one table entry: call(...) launches into a fresh sentinel-filled output, digest() closes the entry."""

    def __init__(self, B):
        self.B, self.L, self.h, self.refused = B, B.lib(), hashlib.sha256(), 0

    def call(self, name, d_qkv, mid, shape, dtype, *ints):
        """name(stream, qkv, *mid[0], out, *mid[1], *ints) into an output of `shape`."""
        d_out = self.B.DeviceArray.from_numpy(np.full(shape, -7.0 if dtype == np.float32 else 0xC0E0, dtype))
        rc = getattr(self.L, name)(None, d_qkv.ptr, *mid[0], d_out.ptr, *mid[1], *ints)
        if rc == 0:
            self.h.update(d_out.numpy().tobytes())
        else:
            self.h.update(b"refused %d" % rc)
            self.refused += 1
        d_out.free()

    def digest(self):
        return self.h.hexdigest()[:16] + (f"/r{self.refused}" if self.refused else "")


def operands(B, key, rows, width):
    vals = np.random.default_rng([SEED] + list(key)).uniform(-1.5, 1.5, (rows, width)).astype(np.float32)
    return B.DeviceArray.from_numpy(vals), B.DeviceArray.from_numpy(B.to_bf16_bits(vals))


def pv_cell(B, hd, tokens, images):
    rows, D = images * tokens, HEADS * hd
    d_f, d_b = operands(B, (0, hd, tokens, images), rows, 3 * D)
    f32, b16, none = (d_f, np.float32), (d_b, np.uint16), ()
    res = {}

    def entry(col, calls):
        g = Group(B)
        for name, (d_qkv, dtype), ints in calls:
            g.call(name, d_qkv, ((), ()), (rows, D), dtype, images, tokens, HEADS, *ints)
        res[col] = g.digest()

    qr = (tokens, 1)
    if hd == 64:
        entry("f32", [("vithip_attention_f32", f32, none)])
        entry("f32_rows", [("vithip_attention_f32_rows", f32, (q,)) for q in qr])
        entry("bf16io", [("vithip_attention_bf16io", b16, none)])
        entry("bf16io_rows", [("vithip_attention_bf16io_rows", b16, (q,)) for q in qr])
        entry("qscaled", [("vithip_attention_bf16io_qscaled", b16, (q,)) for q in qr])
        entry("f32math", [("vithip_attention_bf16io_f32math", b16, none)])
        entry("f32_hd", [("vithip_attention_f32_hd", f32, (64, q)) for q in qr])
        entry("bf16io_hd", [("vithip_attention_bf16io_hd", b16, (64, q, qs)) for qs in (0, 1) for q in qr])
    else:
        entry("f32", [("vithip_attention_f32_hd", f32, (hd, q)) for q in qr])
        entry("bf16", [("vithip_attention_bf16io_hd", b16, (hd, q, 0)) for q in qr])
        entry("bf16_qs", [("vithip_attention_bf16io_hd", b16, (hd, q, 1)) for q in qr])
    d_f.free()
    d_b.free()
    return res


def cls_cell(B, hd, tokens, images, pad):
    rows, width = images * tokens, 3 * HEADS * hd
    d_f, d_b = operands(B, (1, hd, tokens, images), rows, width)
    res = {}
    for col, d_q, bf16, qs in (("f32", d_f, False, ()), ("bf16", d_b, True, (0,)), ("bf16_qs", d_b, True, (1,))):
        g = Group(B)
        for head_mean in (0, 1):
            ld = (tokens if head_mean else HEADS * tokens) + pad
            names = ["vithip_cls_attention_bf16" if bf16 else "vithip_cls_attention_f32"]
            for name, dim in [(names[0] + "_hd", (hd,))] + ([(names[0], ())] if hd == 64 else []):
                g.call(name, d_q, ((width,), (ld,)), (images, ld), np.float32, images, tokens, HEADS, *dim, head_mean, *qs)
        res[col] = g.digest()
    d_f.free()
    d_b.free()
    return res


def refusals(B):
    """(calls made, [those that did not return hipErrorInvalidValue]).  No call here may reach a launch: the buffers are one small
    allocation whatever the arguments claim."""
    L = B.lib()
    T, n = 33, 2
    d_q, d_o = B.DeviceArray((n * 225, 3 * HEADS * 128)), B.DeviceArray((n * 225, HEADS * 128))
    q, o = d_q.ptr, d_o.ptr
    made, wrong = 0, []

    def bad(name, *args):
        nonlocal made
        made += 1
        rc = getattr(L, name)(None, *args)
        if rc != INVALID_VALUE:
            wrong.append(f"{name}{args[2:]} -> {rc}")

    def pv(name, qp, op, tokens, heads, tail):
        bad(name, qp, op, n, tokens, heads, *tail)

    def cls(name, qp, op, hd, tail):
        bad(name, qp, 3 * HEADS * hd, op, HEADS * T, n, T, HEADS, *tail)

    for hd in (0, 32, 56, 68, 136):
        pv("vithip_attention_f32_hd", q, o, T, HEADS, (hd, T))
        pv("vithip_attention_bf16io_hd", q, o, T, HEADS, (hd, T, 0))
        cls("vithip_cls_attention_f32_hd", q, o, hd, (hd, 0))
        cls("vithip_cls_attention_bf16_hd", q, o, hd, (hd, 0, 0))
    for qr in (0, T + 1):
        for name in ("vithip_attention_f32_rows", "vithip_attention_bf16io_rows", "vithip_attention_bf16io_qscaled"):
            pv(name, q, o, T, HEADS, (qr,))
        for hd in (64, 80):
            pv("vithip_attention_f32_hd", q, o, T, HEADS, (hd, qr))
            pv("vithip_attention_bf16io_hd", q, o, T, HEADS, (hd, qr, 0))
    for hd in (64, 80):
        pv("vithip_attention_bf16io_hd", q, o, T, HEADS, (hd, T, 2))
        cls("vithip_cls_attention_bf16_hd", q, o, hd, (hd, 0, 2))
    cls("vithip_cls_attention_bf16", q, o, 64, (0, 2))
    for qr in (1, 224):  # head_dim 64, 225 tokens: only the kernels for up to 224 tokens stop at q_rows
        for name in ("vithip_attention_f32_rows", "vithip_attention_bf16io_rows", "vithip_attention_bf16io_qscaled"):
            pv(name, q, o, 225, HEADS, (qr,))
        pv("vithip_attention_f32_hd", q, o, 225, HEADS, (64, qr))
        for qs in (0, 1):
            pv("vithip_attention_bf16io_hd", q, o, 225, HEADS, (64, qr, qs))
    pv("vithip_attention_f32_rows", q, o, 225, HEADS, (225,))
    pv("vithip_attention_bf16io_rows", q, o, 225, HEADS, (225,))
    pv("vithip_attention_f32_hd", q, o, 1, 65536, (80, 1))
    pv("vithip_attention_bf16io_hd", q, o, 1, 65536, (80, 1, 0))
    for qp, op in ((None, o), (q, None), (q + 4, o), (q, o + 4)):
        for name, tail in (("vithip_attention_f32", ()), ("vithip_attention_bf16io", ()), ("vithip_attention_bf16io_f32math", ()),
                           ("vithip_attention_f32_rows", (T,)), ("vithip_attention_bf16io_rows", (T,)),
                           ("vithip_attention_bf16io_qscaled", (T,)), ("vithip_attention_f32_hd", (64, T)),
                           ("vithip_attention_f32_hd", (80, T)), ("vithip_attention_bf16io_hd", (64, T, 0)),
                           ("vithip_attention_bf16io_hd", (80, T, 1))):
            pv(name, qp, op, T, HEADS, tail)
    for qp, op in ((None, o), (q, None), (q + 4, o)):  # a class row's output is fp32 and needs 4-byte alignment only
        cls("vithip_cls_attention_f32", qp, op, 64, (0,))
        cls("vithip_cls_attention_bf16", qp, op, 64, (0, 0))
        for hd in (64, 80):
            cls("vithip_cls_attention_f32_hd", qp, op, hd, (hd, 0))
            cls("vithip_cls_attention_bf16_hd", qp, op, hd, (hd, 0, 0))
    d_q.free()
    d_o.free()
    return made, wrong


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

    table(emit, ["tokens", "images"], (((t, n), pv_cell(B, 64, t, n)) for t in TOKENS_64 for n in IMAGES))
    emit("")
    table(emit, ["head_dim", "tokens", "images"], (((hd, t, n), pv_cell(B, hd, t, n)) for hd in DIMS_HD for t in TOKENS_HD for n in IMAGES))
    emit("")
    table(emit, ["head_dim", "tokens", "images", "ld_out - row"],
          (((hd, t, n, pad), cls_cell(B, hd, t, n, pad)) for hd in DIMS_CLS for t in TOKENS_CLS for n in IMAGES for pad in (0, PAD)))
    emit("")
    made, wrong = refusals(B)
    emit(f"refusals: {made} calls, {made - len(wrong)} returned hipErrorInvalidValue" + "".join(f"; NOT {w}" for w in wrong))


if __name__ == "__main__":
    main()
