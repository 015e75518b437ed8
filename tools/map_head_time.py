#!/usr/bin/env python3
"""The attention-pool head against its plain form and against the mean pooling (GPU box only).

    python3 tools/map_head_time.py [--steps K] [--warmup W] [--parts kernel,sweep,engine] [--out FILE.jsonl]

kernel  vithip_map_pool_f32 (its three launches) at (n, T, D, H) = (256, 197, 768, 12), (256, 729, 1152, 16), (1, 197, 768, 12), beside
        the plain form on the same rows -- vithip_layernorm_f32, then vithip_gemm_f32 for the [n T][2D] K/V projection -- and
        vithip_layernorm_pool_f32 (one read of x): device events round `reps` back-to-back launches, the legs alternated.
sweep   the same launcher at segment lengths 16 .. 256 (needs the probe library: VIT_HIP_LIBRARY=.../libvit_mi355x_probe.so).
engine  the fp32 ViT-B/16 engine at batch 256: features_device "map" against "mean", host clock round a window of calls.

One JSON line per leg: median, min, max ms, the window-to-window spread (max - min) / median, and x's bytes over the median.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(256, 197, 768, 12), (256, 729, 1152, 16), (1, 197, 768, 12)]


def stats(ms):
    med = statistics.median(ms)
    return {"median_ms": round(med, 5), "min_ms": round(min(ms), 5), "max_ms": round(max(ms), 5),
            "spread_over_median": round((max(ms) - min(ms)) / med, 4), "steps": len(ms)}


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def timed(B, legs, a, reps):
    L = B.lib()
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        B.hip_check(L.vithip_event_create(C.byref(e)), "event_create")
    ms, order = {leg: [] for leg in legs}, list(legs)
    for step in range(a.warmup + a.steps):
        for leg in (order if step % 2 == 0 else order[::-1]):
            B.hip_check(L.vithip_event_record(ev[0], None), "record")
            for _ in range(reps):
                legs[leg]()
            B.hip_check(L.vithip_event_record(ev[1], None), "record")
            B.hip_check(L.vithip_event_sync(ev[1]), "event_sync")
            t = C.c_float()
            B.hip_check(L.vithip_event_elapsed_ms(C.byref(t), ev[0], ev[1]), "elapsed")
            if step >= a.warmup:
                ms[leg].append(t.value / reps)
    for e in ev:
        L.vithip_event_destroy(e)
    return ms


def kernel_part(B, a, out, sweep):
    L = B.lib()
    for n, T, D, H in SHAPES:
        rng = np.random.default_rng(D)
        d_x = B.DeviceArray.from_numpy(rng.normal(0, 1, (n * T, D)).astype(np.float32))
        d_g, d_b = B.DeviceArray.from_numpy(np.ones(D, np.float32)), B.DeviceArray.from_numpy(np.zeros(D, np.float32))
        d_a = B.DeviceArray.from_numpy(rng.normal(0, 2 / np.sqrt(D), (H, D)).astype(np.float32))
        d_w = B.DeviceArray.from_numpy(rng.normal(0, D ** -0.5, (2 * D, D)).astype(np.float32))
        d_bias, d_o = B.DeviceArray.from_numpy(np.zeros(2 * D, np.float32)), B.DeviceArray((n, D))
        reps = 20 if n > 1 else 200

        def map_pool(ws):
            B.hip_check(L.vithip_map_pool_f32(None, d_x.ptr, D, d_g.ptr, d_b.ptr, 1e-6, d_a.ptr, d_w.ptr, d_bias.ptr, d_o.ptr, D, n, T, 1, D, H,
                                              ws.ptr), "map_pool")

        if sweep:
            legs = {}
            for ts in (16, 32, 64, 128, 256):
                B.hip_check(L.vithip_map_pool_set_ts(ts), "set_ts")
                ws = B.DeviceArray((L.vithip_map_pool_f32_workspace_floats(n, T, 1, D, H),))
                legs[f"ts{ts}"] = lambda ts=ts, ws=ws: (B.hip_check(L.vithip_map_pool_set_ts(ts), "set_ts"), map_pool(ws))
        else:
            ws = B.DeviceArray((L.vithip_map_pool_f32_workspace_floats(n, T, 1, D, H),))
            d_y, d_kv = B.DeviceArray((n * T, D)), B.DeviceArray((n * T, 2 * D))
            d_pw = B.DeviceArray((max(1, L.vithip_layernorm_pool_f32_workspace_floats(n, T, 1, D)),))
            g = B.CGemmArgs()
            g.A, g.lda, g.W, g.ldw, g.bias, g.C, g.ldc, g.M, g.N, g.K = d_y.ptr, D, d_w.ptr, D, d_bias.ptr, d_kv.ptr, 2 * D, n * T, 2 * D, D

            def plain():
                B.hip_check(L.vithip_layernorm_f32(None, d_x.ptr, D, d_y.ptr, D, d_g.ptr, d_b.ptr, n * T, D), "layernorm")
                B.hip_check(L.vithip_gemm_f32(None, C.byref(g)), "gemm")

            legs = {"map_pool": lambda: map_pool(ws), "layernorm_then_kv_gemm": plain,
                    "layernorm_pool_mean": lambda: B.hip_check(L.vithip_layernorm_pool_f32(None, d_x.ptr, D, d_o.ptr, D, d_g.ptr, d_b.ptr, n, T, 1,
                                                                                           D, 0, d_pw.ptr), "pool")}
        ms = timed(B, legs, a, reps)
        for leg in legs:
            med = statistics.median(ms[leg])
            emit(out, dict({"part": "sweep" if sweep else "kernel", "leg": leg, "n": n, "T": T, "D": D, "H": H, "reps_per_sample": reps,
                            "x_GB_per_s": round(n * (T - 1) * D * 4 / med / 1e6, 1)}, **stats(ms[leg])))
    if sweep:
        B.hip_check(L.vithip_map_pool_set_ts(0), "set_ts")


def engine_part(pkg, B, a, out):
    cfg, n = pkg.VIT_B16, 256
    eng = B.Engine(cfg, max_batch=n)
    eng.load_weights(pkg.synth.make_weights(cfg, 1234))
    eng.set_map_head(B.map_head_spec(12, 3072, "gelu_tanh"), pkg.synth.make_map_head(768, 12, 3072))
    d_x, d_o = B.DeviceArray.from_numpy(pkg.synth.make_images(cfg, n, 7)), B.DeviceArray((n, 768))
    legs = {k: (lambda k=k: eng.features_device(d_x.ptr, n, d_o.ptr, k)) for k in ("mean", "map")}
    ms, order = {k: [] for k in legs}, list(legs)
    for step in range(a.warmup + a.steps):
        for leg in (order if step % 2 == 0 else order[::-1]):
            eng.sync()
            t0 = time.perf_counter()
            for _ in range(2):
                legs[leg]()
            eng.sync()
            if step >= a.warmup:
                ms[leg].append(1e3 * (time.perf_counter() - t0) / 2)
    for leg in legs:
        emit(out, dict({"part": "engine", "call": f"features_device {leg}", "dtype": "f32", "batch": n,
                        "over_mean_median": round(statistics.median(ms[leg]) / statistics.median(ms["mean"]), 5)}, **stats(ms[leg])))
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
    parts = a.parts.split(",")
    if "kernel" in parts:
        kernel_part(B, a, out, False)
    if "sweep" in parts:
        B.lib().vithip_map_pool_set_ts.argtypes = [C.c_int]
        kernel_part(B, a, out, True)
    if "engine" in parts:
        engine_part(pkg, B, a, out)


if __name__ == "__main__":
    main()
