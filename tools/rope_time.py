#!/usr/bin/env python3
"""The rotary-embedding launch against an HBM-bound in-place kernel of equal traffic, and its cost inside the engine (GPU box only).

    python3 tools/rope_time.py [--steps K] [--warmup W] [--parts kernel,engine] [--out FILE.jsonl]

kernel  vithip_rope_f32 / _bf16 at DINOv3 ViT-B/16, batch 256 (n T = 256 x 201 rows, D = 768, 12 heads; QK and K alone) beside
        vithip_swiglu_f32 / _bf16 on rows of 2H = 2048 columns with H = 1024: per row both read and write 3072 elements in all.
        Device events round `reps` back-to-back launches, the legs alternated.  GB/s = bytes read + written / median.
engine  features_device("cls") on synth.DINOV3_B16 at batch 256, fp32 and bf16, the rotation on and off on the same engine, host
        clock round a window of calls.

One JSON line per leg: median, min, max ms, the window-to-window spread (max - min) / median.
"""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from map_head_time import emit, stats, timed  # noqa: E402

N, PREFIX, P, HEADS, HD, H = 256, 5, 196, 12, 64, 1024


def kernel_part(B, a, out):
    L = B.lib()
    T, D = PREFIX + P, HEADS * HD
    rng = np.random.default_rng(36)
    ang = rng.uniform(-np.pi, np.pi, (P, HD // 2))
    d_cos, d_sin = B.DeviceArray.from_numpy(np.cos(ang).astype(np.float32)), B.DeviceArray.from_numpy(np.sin(ang).astype(np.float32))
    for bf16 in (False, True):
        dt = np.uint16 if bf16 else np.float32
        esz = np.dtype(dt).itemsize
        make = (lambda shape: B.to_bf16_bits(rng.uniform(-4, 4, shape).astype(np.float32)).reshape(shape)) if bf16 else \
               (lambda shape: rng.uniform(-4, 4, shape).astype(np.float32))
        d_qkv, d_u, d_h = B.DeviceArray.from_numpy(make((N * T, 3 * D))), B.DeviceArray.from_numpy(make((N * P, 2 * H))), B.DeviceArray((N * P, H), dt)
        legs = {f"rope_{w}": (lambda w=w: B.hip_check(B.rope_raw(d_qkv.ptr, 3 * D, d_cos.ptr, d_sin.ptr, N, T, PREFIX, HEADS, HD,
                                                                 B.ROPE_WHICH[w], bf16), "rope")) for w in ("qk", "k")}
        legs["swiglu"] = lambda: B.hip_check(B.swiglu_raw(d_u.ptr, 2 * H, d_h.ptr, H, N * P, H, bf16), "swiglu")
        moved = {"rope_qk": 2 * N * P * 2 * D * esz, "rope_k": 2 * N * P * D * esz, "swiglu": N * P * 3 * H * esz}
        ms = timed(B, legs, a, 20)
        for leg in legs:
            emit(out, dict({"part": "kernel", "leg": leg, "dtype": "bf16" if bf16 else "f32", "bytes_moved": moved[leg],
                            "GB_per_s": round(moved[leg] / statistics.median(ms[leg]) / 1e6, 1)}, **stats(ms[leg])))
        for d in (d_qkv, d_u, d_h):
            d.free()


def engine_part(pkg, B, a, out):
    cfg = pkg.DINOV3_B16
    W = pkg.synth.make_weights(cfg, 1234)
    d_x, d_o = B.DeviceArray.from_numpy(pkg.synth.make_images(cfg, N, 7)), B.DeviceArray((N, cfg.embed_dim))
    for dtype in ("f32", "bf16"):
        eng = B.Engine(cfg, max_batch=N, dtype=dtype)
        eng.set_layernorm_eps(1e-5)
        eng.load_weights(W)
        ms = {"off": [], "on": []}
        for step in range(a.warmup + a.steps):
            for leg in (("off", "on") if step % 2 == 0 else ("on", "off")):
                eng.set_rope(100.0 if leg == "on" else 0.0)   # synchronises the device
                eng.features_device(d_x.ptr, N, d_o.ptr, "cls")
                eng.sync()
                t0 = time.perf_counter()
                for _ in range(2):
                    eng.features_device(d_x.ptr, N, d_o.ptr, "cls")
                eng.sync()
                if step >= a.warmup:
                    ms[leg].append(1e3 * (time.perf_counter() - t0) / 2)
        off = statistics.median(ms["off"])
        for leg in ms:
            med = statistics.median(ms[leg])
            emit(out, dict({"part": "engine", "call": "features_device cls", "rope": leg, "dtype": dtype, "batch": N,
                            "over_off_ms": round(med - off, 4), "over_off_percent": round(100 * (med - off) / off, 3)}, **stats(ms[leg])))
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parts", default="kernel,engine")
    ap.add_argument("--out")
    a = ap.parse_args()
    pkg = importlib.import_module("vision-transformer-opencl_amd")
    B = importlib.import_module("vision-transformer-opencl_amd.binding")
    out = open(a.out, "a") if a.out else None
    if "kernel" in a.parts.split(","):
        kernel_part(B, a, out)
    if "engine" in a.parts.split(","):
        engine_part(pkg, B, a, out)


if __name__ == "__main__":
    main()
