#!/usr/bin/env python3
"""Intermediate-layer outputs against features(tokens), ViT-B/16 fp32, batch 256, device resident (GPU box only).

    python3 tools/intermediate_time.py [--steps K] [--warmup W] [--parts engine,kernel] [--out FILE.jsonl] [--label NAME]
    python3 tools/intermediate_time.py --parts trace --leg LEG [--steps K]        under rocprofv3 --kernel-trace --stats, one leg per run
    python3 tools/intermediate_time.py --summarize KERNEL_STATS_CSV [--leg LEG]   (no GPU)

engine  ms per call, host clock around the call and a stream sync, the legs alternated in one process (A B C D, D C B A, ...):
        features(tokens) -- the yardstick: a full encoder and one LayerNorm pass over every token -- against
        intermediate(layers=(2, 5, 8, 11)) for tokens and map (a full encoder and four passes: three more than the yardstick) and
        intermediate(layers=(5,)) for tokens and map (six of the twelve layers and one pass).  With VIT_HIP_LIBRARY pointing at a
        build without the intermediate calls only the yardstick leg runs (--label names that build in the records).
kernel  vithip_tap_f32 for the four layouts, norm on and off, against vithip_layernorm_f32 over the same n * T rows at
        (256, 197, 768): device events round `reps` back-to-back launches; effective bytes/s = (bytes read + bytes written) / time.
trace   what a rocprofv3 --kernel-trace --stats run should see and nothing else: the engine at batch 256 making --steps calls of ONE
        leg -- features_tokens (its last launch of layernorm_f32_kernel per call is the pass over n * T rows; works on a build
        without the intermediate calls too), tokens, patches or map (one tap of the last layer, norm = 1: one tap kernel per call).
        The kernel's rows in the statistics then belong to that launch alone.

One JSON line per measurement.  --summarize prints the rows of the tap and LayerNorm kernels of a kernel-statistics CSV.
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

BATCH = 256
KERNELS = ("tap_rows_kernel", "tap_map_kernel", "layernorm_f32_kernel")
TRACE_LEGS = ("features_tokens", "tokens", "patches", "map")


def summarize(path, leg):
    with open(path) as f:
        for r in csv.DictReader(f):
            if any(k in r.get("Name", "") for k in KERNELS):
                print(json.dumps({"leg": leg, "kernel": r["Name"], "calls": int(r["Calls"]), "average_us": round(float(r["AverageNs"]) / 1e3, 2),
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


def make_engine(pkg, B):
    cfg = pkg.VIT_B16
    eng = B.Engine(cfg, max_batch=BATCH, dtype="f32")
    eng.load_weights(pkg.synth.make_weights(cfg, 1234))
    return cfg, eng, B.DeviceArray.from_numpy(pkg.synth.make_images(cfg, BATCH, 7))


def have_intermediate(B):
    return hasattr(B, "CIntermediateSpec") and hasattr(B.lib(), "vit_engine_intermediate_device")


def engine_part(pkg, B, a, out):
    cfg, eng, d_x = make_engine(pkg, B)
    n, row = BATCH, cfg.tokens * cfg.embed_dim
    d_out = B.DeviceArray((n, 4 * row))
    legs = {"features_tokens": lambda: eng.features_device(d_x.ptr, n, d_out.ptr, "tokens")}
    if have_intermediate(B):
        for name, layers in (("2_5_8_11", (2, 5, 8, 11)), ("5", (5,))):
            for kind in ("tokens", "map"):
                legs[f"{kind}_{name}"] = lambda layers=layers, kind=kind: eng.intermediate_device(d_x.ptr, n, d_out.ptr, layers, kind, True)
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
    base = statistics.median(ms["features_tokens"])
    for leg in order:
        emit(out, dict({"part": "engine", "library": a.label, "dtype": "f32", "batch": n, "call": leg,
                        "over_features_tokens_median": round(statistics.median(ms[leg]) / base, 4)}, **stats(ms[leg])))
    eng.close()


def trace_part(pkg, B, a, out):
    cfg, eng, d_x = make_engine(pkg, B)
    n = BATCH
    d_out = B.DeviceArray((n, cfg.tokens * cfg.embed_dim))
    if a.leg == "features_tokens":
        call = lambda: eng.features_device(d_x.ptr, n, d_out.ptr, "tokens")
    else:
        call = lambda: eng.intermediate_device(d_x.ptr, n, d_out.ptr, (cfg.depth - 1,), a.leg, True)
    for _ in range(a.steps):
        call()
        eng.sync()
    emit(out, {"part": "trace", "library": a.label, "leg": a.leg, "calls": a.steps})
    eng.close()


def kernel_part(B, a, out):
    L = B.lib()
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        B.hip_check(L.vithip_event_create(C.byref(e)), "event_create")
    n, T, D = BATCH, 197, 768
    rng = np.random.default_rng(n)
    d_x = B.DeviceArray.from_numpy(rng.uniform(-1.5, 1.5, size=(n * T, D)).astype(np.float32))
    d_g, d_b = B.DeviceArray.from_numpy(rng.uniform(0.5, 1.5, D).astype(np.float32)), B.DeviceArray.from_numpy(np.zeros(D, np.float32))
    d_y = B.DeviceArray((n * T, D))
    legs = {"layernorm": lambda: L.vithip_layernorm_f32(None, d_x.ptr, D, d_y.ptr, D, d_g.ptr, d_b.ptr, n * T, D)}
    rows = {"layernorm": T}
    for layout, k in B.TAP_KINDS.items():
        per = {"cls": 1, "tokens": T}.get(layout, T - 1)
        for norm in (1, 0):
            g, b = (d_g.ptr, d_b.ptr) if norm else (None, None)
            name = f"{layout}_{'norm' if norm else 'raw'}"
            legs[name] = lambda g=g, b=b, k=k, per=per: L.vithip_tap_f32(None, d_x.ptr, D, d_y.ptr, per * D, g, b, n, T, D, k)
            rows[name] = per
    reps = 20
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
        med, nbytes = statistics.median(ms[leg]), 2 * n * rows[leg] * D * 4
        emit(out, dict({"part": "kernel", "launch": leg, "images": n, "tokens": T, "dim": D, "reps_per_sample": reps, "bytes": nbytes,
                        "effective_TBps": round(nbytes / (med * 1e-3) / 1e12, 3),
                        "over_layernorm_median": round(med / statistics.median(ms["layernorm"]), 4)}, **stats(ms[leg])))
    for e in ev:
        L.vithip_event_destroy(e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parts", default="engine,kernel")
    ap.add_argument("--leg", default="tokens", choices=TRACE_LEGS)
    ap.add_argument("--out")
    ap.add_argument("--label", default="this build", help="the `library` field of the records (name the build VIT_HIP_LIBRARY points at)")
    ap.add_argument("--summarize")
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize, a.leg)
    pkg = importlib.import_module("vision-transformer-opencl_amd")
    B = importlib.import_module("vision-transformer-opencl_amd.binding")
    out = open(a.out, "a") if a.out else None
    parts = a.parts.split(",")
    if "kernel" in parts:
        kernel_part(B, a, out)
    if "engine" in parts:
        engine_part(pkg, B, a, out)
    if "trace" in parts:
        trace_part(pkg, B, a, out)


if __name__ == "__main__":
    main()
