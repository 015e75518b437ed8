#!/usr/bin/env python3
"""The biased attention launch against the unbiased launches of equal shape, and its cost inside the engine (GPU box only).

    python3 tools/attention_bias_time.py [--steps K] [--warmup W] [--parts kernel,engine] [--out FILE.jsonl]

kernel  batch 256, 197 tokens, head_dim 64, 12 heads (ViT-B) and 16 heads (ViT-L); the bias [heads][197][200] fp32, U(-4, 4).
        fp32: vithip_attention_f32_bias beside vithip_attention_f32_hd and vithip_attention_f32_split; bf16: vithip_attention_bf16io_bias
        beside vithip_attention_bf16io_hd.  Device events round `reps` back-to-back launches, the legs alternated in one process.
engine  features_device("cls") on synth.BEIT_B16 at batch 256, fp32 and bf16, every layer's bias on and off on the same engine, host
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

N, T, LD, HD = 256, 197, 200, 64


def kernel_part(B, a, out):
    L = B.lib()
    rng = np.random.default_rng(37)
    for heads in (12, 16):
        D = heads * HD
        d_bias = B.DeviceArray.from_numpy(rng.uniform(-4, 4, (heads * T, LD)).astype(np.float32))
        for bf16 in (False, True):
            dt = np.uint16 if bf16 else np.float32
            qkv = rng.uniform(-1.5, 1.5, (N * T, 3 * D)).astype(np.float32)
            d_qkv, d_o = B.DeviceArray.from_numpy(B.to_bf16_bits(qkv).reshape(qkv.shape) if bf16 else qkv), B.DeviceArray((N * T, D), dt)
            shape = (N, T, heads, HD, T)
            if bf16:
                legs = {"bias": lambda: B.hip_check(L.vithip_attention_bf16io_bias(None, d_qkv.ptr, d_o.ptr, d_bias.ptr, LD, *shape, 0), "bias"),
                        "hd": lambda: B.hip_check(L.vithip_attention_bf16io_hd(None, d_qkv.ptr, d_o.ptr, *shape, 0), "hd")}
            else:
                legs = {"bias": lambda: B.hip_check(L.vithip_attention_f32_bias(None, d_qkv.ptr, d_o.ptr, d_bias.ptr, LD, *shape), "bias"),
                        "hd": lambda: B.hip_check(L.vithip_attention_f32_hd(None, d_qkv.ptr, d_o.ptr, *shape), "hd"),
                        "split": lambda: B.hip_check(L.vithip_attention_f32_split(None, d_qkv.ptr, d_o.ptr, *shape), "split")}
            ms = timed(B, legs, a, 10)
            base = statistics.median(ms["hd"])
            for leg in legs:
                emit(out, dict({"part": "kernel", "leg": leg, "dtype": "bf16" if bf16 else "f32", "heads": heads, "batch": N, "tokens": T,
                                "over_hd": round(statistics.median(ms[leg]) / base, 4)}, **stats(ms[leg])))
            for d in (d_qkv, d_o):
                d.free()
        d_bias.free()


def engine_part(pkg, B, a, out):
    cfg = pkg.BEIT_B16
    W = pkg.synth.make_weights(cfg, 1234)
    bias = B.rel_pos_bias(np.random.default_rng(38).uniform(-2, 2, ((2 * 14 - 1) ** 2 + 3, cfg.num_heads)), 14)
    d_x, d_o = B.DeviceArray.from_numpy(pkg.synth.make_images(cfg, N, 7)), B.DeviceArray((N, cfg.embed_dim))
    for dtype in ("f32", "bf16"):
        eng = B.Engine(cfg, max_batch=N, dtype=dtype)
        eng.load_weights(W)
        ms = {"off": [], "on": []}
        for step in range(a.warmup + a.steps):
            for leg in (("off", "on") if step % 2 == 0 else ("on", "off")):
                eng.set_attention_bias(-1, bias if leg == "on" else None)   # synchronises the device
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
            emit(out, dict({"part": "engine", "call": "features_device cls", "bias": leg, "dtype": dtype, "batch": N,
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
