#!/usr/bin/env python3
"""vithip_gemm_mxfp8 beside vithip_gemm_bf16 at the encoder's layer shapes, and the mxfp8 engine beside the bf16 engines (GPU box only).

    python3 tools/mxfp8_time.py [--steps K] [--warmup W] [--parts kernel,engine] [--out FILE.jsonl]

kernel  QKV, out_proj, fc1 and fc2 of ViT-B/16 at batch 256 and 2,048 and of ViT-L/16-384 at batch 1,024: the two GEMMs alternated in one
        process on the same A (bf16, U(-1, 1)) and W (fp32 U(-0.05, 0.05), as its bf16 copy and as its MXFP8 image), device events
        round windows of at least 0.5 s of back-to-back launches.  TFLOP/s = 2 M N K over the median time.
engine  features_device("cls") of ViT-B/16 at batch 2,048: bf16 default (fold on), bf16 ln_fold = -1 and mxfp8 = 1, same weights and
        images, the legs alternated, host clock round windows of at least 0.5 s.

One JSON line per leg: median, min, max ms, the window-to-window spread (max - min) / median.
"""
import argparse
import ctypes as C
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

MODELS = {"ViT-B/16 batch 256": (256 * 197, 768, 3072), "ViT-B/16 batch 2048": (2048 * 197, 768, 3072),
          "ViT-L/16-384 batch 1024": (1024 * 577, 1024, 4096)}   # rows, D, H
EPI_BF16, EPI_GELU, EPI_RES = 0, 1, 2


def kernel_part(B, a, out):
    L = B.lib()
    L.vithip_gemm_bf16.argtypes = [C.c_void_p, C.POINTER(B.CGemmBf16Args)]
    L.vithip_gemm_mxfp8.argtypes = [C.c_void_p, C.POINTER(B.CGemmMxfp8Args)]
    L.vithip_memset.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    rng = np.random.default_rng(38)
    for model, (M, D, H) in MODELS.items():
        for name, N, K, epi in (("qkv", 3 * D, D, EPI_BF16), ("out_proj", D, D, EPI_RES), ("fc1", H, D, EPI_GELU), ("fc2", D, H, EPI_RES)):
            block = B.to_bf16_bits(rng.uniform(-1, 1, (4096, K)).astype(np.float32))
            d_a = B.DeviceArray.from_numpy(np.tile(block, ((M + 4095) // 4096, 1))[:M])
            W = rng.uniform(-0.05, 0.05, (N, K)).astype(np.float32)
            d_w16, d_img = B.DeviceArray.from_numpy(B.to_bf16_bits(W)), B.mxfp8_weights_device(B.DeviceArray.from_numpy(W), N, K)
            d_b = B.DeviceArray.from_numpy(np.zeros(N, np.float32))
            d_c = B.DeviceArray((M, N), np.float32 if epi == EPI_RES else np.uint16)
            res = d_c.ptr if epi == EPI_RES else None
            a16 = B.CGemmBf16Args(d_a.ptr, K, d_w16.ptr, K, d_b.ptr, res, N, d_c.ptr, N, M, N, K, epi, 0, None, None, None, N, None)
            a8 = B.CGemmMxfp8Args(d_a.ptr, K, d_img.ptr, d_b.ptr, res, N, d_c.ptr, N, M, N, K, epi)
            B.hip_check(L.vithip_memset(d_c.ptr, 0, d_c.nbytes, None), "memset")   # the residual legs accumulate from zero
            legs = {"bf16": lambda: B.hip_check(L.vithip_gemm_bf16(None, C.byref(a16)), "bf16"),
                    "mxfp8": lambda: B.hip_check(L.vithip_gemm_mxfp8(None, C.byref(a8)), "mxfp8")}
            one = max(statistics.median(v) for v in timed(B, legs, argparse.Namespace(warmup=1, steps=1), 2).values())
            ms = timed(B, legs, a, max(2, int(500.0 / one) + 1))
            for leg in legs:
                med = statistics.median(ms[leg])
                emit(out, dict({"part": "kernel", "model": model, "gemm": name, "leg": leg, "M": M, "N": N, "K": K,
                                "tflops": round(2.0 * M * N * K / (med * 1e-3) / 1e12, 1),
                                "over_bf16": round(med / statistics.median(ms["bf16"]), 4)}, **stats(ms[leg])))
            for d in (d_a, d_w16, d_img, d_b, d_c):
                d.free()


def engine_part(pkg, B, a, out):
    cfg, n = pkg.VIT_B16, 2048
    W = pkg.synth.make_weights(cfg, 1234)
    d_x, d_o = B.DeviceArray.from_numpy(pkg.synth.make_images(cfg, n, 7)), B.DeviceArray((n, cfg.embed_dim))
    engines = {"bf16 fold": dict(), "bf16 ln_fold=-1": dict(ln_fold=-1), "mxfp8": dict(mxfp8=1)}
    for leg, opt in engines.items():
        engines[leg] = B.Engine(cfg, max_batch=n, dtype="bf16", **opt)
        engines[leg].load_weights(W)
    ms, reps = {leg: [] for leg in engines}, 1
    for step in range(a.warmup + a.steps):
        for leg in (list(engines) if step % 2 == 0 else list(engines)[::-1]):
            eng = engines[leg]
            eng.features_device(d_x.ptr, n, d_o.ptr, "cls")
            eng.sync()
            t0 = time.perf_counter()
            for _ in range(reps):
                eng.features_device(d_x.ptr, n, d_o.ptr, "cls")
            eng.sync()
            dt = time.perf_counter() - t0
            if step >= a.warmup:
                ms[leg].append(1e3 * dt / reps)
            elif dt / reps * reps < 0.5:
                reps = max(reps, int(0.5 / (dt / reps)) + 1)
    base = statistics.median(ms["bf16 fold"])
    for leg in engines:
        med = statistics.median(ms[leg])
        emit(out, dict({"part": "engine", "call": "features_device cls", "leg": leg, "model": "ViT-B/16", "batch": n,
                        "images_per_s": round(n / (med * 1e-3), 1), "over_bf16_fold": round(med / base, 4)}, **stats(ms[leg])))
        engines[leg].close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
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
