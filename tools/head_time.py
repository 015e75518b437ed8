#!/usr/bin/env python3
"""Pooled and multi-layer classifier heads: the pool-then-normalise launch and what a head costs a forward (GPU box only).

    python3 tools/head_time.py [--steps K] [--warmup W] [--calls N] [--parts kernel,engine] [--out FILE.jsonl]

kernel  vithip_pool_layernorm_f32 beside vithip_layernorm_pool_f32 on the same x at (images, tokens, dim) = (256, 197, 768) and
        (256, 257, 1024), first_tok = 1.  x rotates over ROTATE copies so that a launch finds none of its rows in the 256 MiB
        Infinity Cache; device events round `reps` back-to-back launches, the two legs alternated (A B, B A, ...).  Reported: us per
        launch and the bytes of x over that time against the 8 TB/s of HBM3E.
engine  ViT-B/16 at batch 256, fp32 and bf16 engines: vit_engine_forward_device with the checkpoint's own head against the same
        call with a DINOv2 1-layer head, a DINOv2 4-layer head and a timm fc_norm head (vit_engine_set_head), ms per call; host
        clock around a window of --calls calls and a stream sync, the four legs alternated (the head is set outside the window).

One JSON line per leg: median, min, max, mean ms and the window-to-window spread (max - min) / median.
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

KERNEL_SHAPES = [(256, 197, 768), (256, 257, 1024)]
ROTATE = 3
HBM_PEAK = 8.0e12
HEADS = {"own head": None, "dinov2 1 layer": ((-1,), "avg"), "dinov2 4 layers": ((-4, -3, -2, -1), "avg"), "timm fc_norm": ((), "avg_fcnorm")}


def stats(ms):
    med = statistics.median(ms)
    return {"median_ms": round(med, 5), "min_ms": round(min(ms), 5), "max_ms": round(max(ms), 5), "mean_ms": round(statistics.fmean(ms), 5),
            "spread_over_median": round((max(ms) - min(ms)) / med, 4), "steps": len(ms)}


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def kernel_part(B, a, out):
    L = B.lib()
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        B.hip_check(L.vithip_event_create(C.byref(e)), "event_create")
    for images, tokens, dim in KERNEL_SHAPES:
        rng = np.random.default_rng(tokens)
        x = (rng.standard_normal(dim)[None, :] + rng.standard_normal((images * tokens, dim))).astype(np.float32)
        d_x = [B.DeviceArray.from_numpy(x) for _ in range(ROTATE)]
        d_g = B.DeviceArray.from_numpy(rng.uniform(0.5, 1.5, dim).astype(np.float32))
        d_b = B.DeviceArray.from_numpy(rng.uniform(-0.5, 0.5, dim).astype(np.float32))
        d_o = B.DeviceArray((images, dim))
        d_ws = B.DeviceArray((L.vithip_pool_layernorm_f32_workspace_floats(images, tokens, 1, dim),))
        legs = {"vithip_layernorm_pool_f32": lambda p: L.vithip_layernorm_pool_f32(None, p, dim, d_o.ptr, dim, d_g.ptr, d_b.ptr, images, tokens, 1,
                                                                                   dim, 0, d_ws.ptr),
                "vithip_pool_layernorm_f32": lambda p: L.vithip_pool_layernorm_f32(None, p, dim, d_o.ptr, dim, d_g.ptr, d_b.ptr, images, tokens, 1,
                                                                                   dim, d_ws.ptr)}
        reps = 60
        ms = {leg: [] for leg in legs}
        order = list(legs)
        for step in range(a.warmup + a.steps):
            for leg in (order if step % 2 == 0 else order[::-1]):
                B.hip_check(L.vithip_event_record(ev[0], None), "record")
                for r in range(reps):
                    B.hip_check(legs[leg](d_x[r % ROTATE].ptr), leg)
                B.hip_check(L.vithip_event_record(ev[1], None), "record")
                B.hip_check(L.vithip_event_sync(ev[1]), "event_sync")
                t = C.c_float()
                B.hip_check(L.vithip_event_elapsed_ms(C.byref(t), ev[0], ev[1]), "elapsed")
                if step >= a.warmup:
                    ms[leg].append(t.value / reps)
        base = statistics.median(ms["vithip_layernorm_pool_f32"])
        for leg in order:
            med = statistics.median(ms[leg])
            emit(out, dict({"part": "kernel", "launch": leg, "images": images, "tokens": tokens, "dim": dim, "first_tok": 1, "reps_per_sample": reps,
                            "x_copies_rotated": ROTATE, "x_bytes": x.nbytes, "median_us": round(1e3 * med, 3),
                            "x_bytes_per_s": round(x.nbytes / (1e-3 * med), 1), "share_of_hbm_peak": round(x.nbytes / (1e-3 * med) / HBM_PEAK, 4),
                            "over_layernorm_pool_median": round(med / base, 4)}, **stats(ms[leg])))
        for d in d_x + [d_g, d_b, d_o, d_ws]:
            d.free()
    for e in ev:
        L.vithip_event_destroy(e)


def engine_part(pkg, B, a, out):
    cfg, n = pkg.VIT_B16, 256
    W = pkg.synth.make_weights(cfg, 1234)
    imgs = pkg.synth.make_images(cfg, n, 7)
    rng = np.random.default_rng(3)
    for dtype in ("f32", "bf16"):
        eng = {}
        for name, spec in HEADS.items():  # an engine per head: the legs alternate without a set_head inside the timed windows
            e = B.Engine(cfg, max_batch=n, dtype=dtype)
            e.load_weights(W)
            if spec:
                F = e.head_in_features(*spec)
                e.set_head((rng.uniform(-1, 1, (cfg.num_classes, F)) / np.sqrt(F)).astype(np.float32),
                           rng.uniform(-0.5, 0.5, cfg.num_classes).astype(np.float32), *spec)
            eng[name] = e
        d_x = B.DeviceArray.from_numpy(imgs)
        d_p = B.DeviceArray((n, cfg.num_classes))
        ms = {name: [] for name in eng}
        order = list(eng)
        for step in range(a.warmup + a.steps):
            for name in (order if step % 2 == 0 else order[::-1]):
                e = eng[name]
                e.sync()
                t0 = time.perf_counter()
                for _ in range(a.calls):
                    e.forward_device(d_x.ptr, n, d_p.ptr)
                e.sync()
                if step >= a.warmup:
                    ms[name].append(1e3 * (time.perf_counter() - t0) / a.calls)
        base = statistics.median(ms["own head"])
        for name in order:
            spec = HEADS[name]
            emit(out, dict({"part": "engine", "head": name, "dtype": dtype, "batch": n, "calls_per_window": a.calls,
                            "in_features": eng[name].head_in_features(*spec) if spec else cfg.embed_dim,
                            "ms_over_own_head": round(statistics.median(ms[name]) - base, 4),
                            "over_own_head_median": round(statistics.median(ms[name]) / base, 5)}, **stats(ms[name])))
        for e in eng.values():
            e.close()
        d_x.free()
        d_p.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=3, help="calls per timed window of the engine part (ms are per call)")
    ap.add_argument("--parts", default="kernel,engine")
    ap.add_argument("--out")
    a = ap.parse_args()
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
