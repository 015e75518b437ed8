#!/usr/bin/env python3
"""Embedding outputs against the probabilities, ViT-B/16, device resident: ms per call, the legs alternated in one process (GPU box only).

    python3 tools/features_time.py [--steps K] [--warmup W] [--configs f32,bf16] [--parts engine,kernel] [--out FILE.jsonl] [--label NAME]
    python3 tools/features_time.py --summarize KERNEL_STATS_CSV     (no GPU)

engine  the fp32 engine at batch 256 and the bf16 engine at batch 2,048 (BASELINE.json configs[1], configs[2]):
        vit_engine_forward_device (probabilities) against vit_engine_features_device for CLS, MEAN and TOKENS on the same images,
        host clock around the call and a stream sync; steps alternate the order of the legs (A B C D, D C B A, ...).
        With VIT_HIP_LIBRARY pointing at another build of the library that has no features entry points (an earlier commit), only the
        `probs` leg runs: that is the yardstick leg of "features(CLS) against the previous build's forward" -- run the two processes
        alternately, the other build's with --label (e.g. --label parent): the records carry it as their `library` field.
kernel  vithip_layernorm_pool_f32 (one pass over x, [n][D] out) against vithip_layernorm_f32 over the same n * T rows (reads the
        same bytes and writes them back), at (n, 197, 768) for n = 1, 8, 256, 2048; device events round `reps` back-to-back launches.
        Effective bytes/s: pool = n*T*D*4 read (+ nothing counted for the 1/16 partial rows), layernorm = 2 * n*T*D*4.

One JSON line per measurement (median, min, mean ms).  --summarize prints the per-kernel rows of a `rocprofv3 --kernel-trace --stats`
run of this tool for the pooling, LayerNorm and L2 kernels.
"""
import argparse
import csv
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

CONFIGS = {"f32": 256, "bf16": 2048}
KERNELS = ("pool_partial_kernel","layernorm_pool_finish_kernel", "l2_normalize_rows_kernel", "layernorm_f32_kernel")
POOL_SHAPES = [(1, 197, 768), (8, 197, 768), (256, 197, 768), (2048, 197, 768)]


def summarize(path):
    with open(path) as f:
        for r in csv.DictReader(f):
            if any(k in r.get("Name", "") for k in KERNELS):
                print(json.dumps({"kernel": r["Name"], "calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 2),
                                  "min_us": round(float(r["MinNs"]) / 1e3, 2), "max_us": round(float(r["MaxNs"]) / 1e3, 2)}))


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "mean_ms": round(statistics.fmean(ms), 4),
            "steps": len(ms)}


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def engine_part(pkg, B, a, out):
    cfg = pkg.VIT_B16
    W = pkg.synth.make_weights(cfg, 1234)
    have_features = hasattr(B, "CFeatureSpec") and hasattr(B.lib(), "vit_engine_features_device")
    for name in a.configs.split(","):
        n = CONFIGS[name]
        eng = B.Engine(cfg, max_batch=n, dtype=name)
        eng.load_weights(W)
        d_x = B.DeviceArray.from_numpy(pkg.synth.make_images(cfg, n, 7))
        d_probs = B.DeviceArray((n, cfg.num_classes))
        legs = {"probs": lambda: eng.forward_device(d_x.ptr, n, d_probs.ptr)}
        extra = {"probs": 0}
        if have_features:
            d_row = B.DeviceArray((n, cfg.embed_dim))
            d_tok = B.DeviceArray((n, cfg.tokens, cfg.embed_dim))
            legs["cls"] = lambda: eng.features_device(d_x.ptr, n, d_row.ptr, "cls")
            legs["mean"] = lambda: eng.features_device(d_x.ptr, n, d_row.ptr, "mean")
            legs["tokens"] = lambda: eng.features_device(d_x.ptr, n, d_tok.ptr, "tokens")
            extra.update(cls=0, mean=0, tokens=n * cfg.tokens * cfg.embed_dim * 4)
        order = list(legs)
        ms = {leg: [] for leg in legs}
        for step in range(a.warmup + a.steps):
            for leg in (order if step % 2 == 0 else order[::-1]):
                eng.sync()
                t0 = time.perf_counter()
                legs[leg]()
                eng.sync()
                if step >= a.warmup:
                    ms[leg].append(1e3 * (time.perf_counter() - t0))
        base = statistics.median(ms["probs"])
        for leg in order:
            emit(out, dict({"part": "engine", "library": a.label, "dtype": name,
                            "batch": n, "output": leg, "output_bytes_beyond_rows": extra[leg],
                            "over_probs_median": round(statistics.median(ms[leg]) / base, 4)}, **stats(ms[leg])))
        eng.close()


def kernel_part(B, a, out):
    L = B.lib()
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        B.hip_check(L.vithip_event_create(C.byref(e)), "event_create")
    for n, T, D in POOL_SHAPES:
        rng = np.random.default_rng(n)
        d_x = B.DeviceArray.from_numpy(rng.uniform(-1.5, 1.5, size=(n * T, D)).astype(np.float32))
        d_g, d_b = B.DeviceArray.from_numpy(rng.uniform(0.5, 1.5, D).astype(np.float32)), B.DeviceArray.from_numpy(np.zeros(D, np.float32))
        d_y, d_o = B.DeviceArray((n * T, D)), B.DeviceArray((n, D))
        d_ws = B.DeviceArray((L.vithip_layernorm_pool_f32_workspace_floats(n, T, 1, D),))
        legs = {"pool": lambda: L.vithip_layernorm_pool_f32(None, d_x.ptr, D, d_o.ptr, D, d_g.ptr, d_b.ptr, n, T, 1, D, 0, d_ws.ptr),
                "layernorm": lambda: L.vithip_layernorm_f32(None, d_x.ptr, D, d_y.ptr, D, d_g.ptr, d_b.ptr, n * T, D)}
        nbytes = {"pool": n * T * D * 4, "layernorm": 2 * n * T * D * 4}
        reps = 20 if n >= 256 else 100
        ms = {leg: [] for leg in legs}
        order = list(legs)
        for step in range(a.warmup + a.steps):
            for leg in (order if step % 2 == 0 else order[::-1]):
                B.hip_check(L.vithip_event_record(ev[0], None), "record")
                for _ in range(reps):
                    B.hip_check(legs[leg](), leg)
                B.hip_check(L.vithip_event_record(ev[1], None), "record")
                B.hip_check(L.vithip_event_sync(ev[1]), "event_sync")
                t = C.c_float()
                B.hip_check(L.vithip_event_elapsed_ms(C.byref(t), ev[0], ev[1]), "elapsed")
                if step >= a.warmup:
                    ms[leg].append(t.value / reps)
        for leg in order:
            med = statistics.median(ms[leg])
            emit(out, dict({"part": "kernel", "launch": leg, "images": n, "tokens": T, "dim": D, "reps_per_sample": reps,
                            "bytes": nbytes[leg], "effective_TBps": round(nbytes[leg] / (med * 1e-3) / 1e12, 3)}, **stats(ms[leg])))
        emit(out, {"part": "kernel", "images": n, "pool_over_layernorm_median": round(statistics.median(ms["pool"]) / statistics.median(ms["layernorm"]), 4)})
        for d in (d_x, d_y, d_o, d_ws, d_g, d_b):
            d.free()
    for e in ev:
        L.vithip_event_destroy(e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--configs", default="f32,bf16")
    ap.add_argument("--parts", default="engine,kernel")
    ap.add_argument("--out")
    ap.add_argument("--label", default="this build", help="the `library` field of the engine records (name the build VIT_HIP_LIBRARY points at)")
    ap.add_argument("--summarize")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize)
    pkg = importlib.import_module("vision-transformer-opencl_amd")
    B = importlib.import_module("vision-transformer-opencl_amd.binding")
    out = open(a.out, "a") if a.out else None
    parts = a.parts.split(",")
    if "kernel" in parts:
        kernel_part(B, a, out)
    if "engine" in parts:
        engine_part(pkg, B, a, out)


if __name__ == "__main__":
    main()
