#!/usr/bin/env python3
"""Attention at head dims other than 64 against the head_dim 64 kernels at equal MACs (GPU box only).

    python3 tools/head_dim_time.py [--steps K] [--warmup W] [--batch N] [--parts kernel,cls,engine] [--out FILE.jsonl]

kernel  one attention launch at batch N (default 256), 257 tokens: 16 heads x 80 (ViT-H/14) beside 20 heads x 64, and 16 x 104
        (ViT-bigG-14) beside 26 x 64 -- the same D, so the same multiply-adds in both products -- fp32 and bf16 (q_scaled, the engine's
        default).  Random U(-1.5, 1.5) operands; the legs of a pair alternate sample by sample in one process, a sample is `reps`
        back-to-back launches between device events.  One JSON line per leg (median, min, max ms per launch) and the ratio of medians.
cls     the class token's attention row (vithip_cls_attention_*_hd, per head) on the same pairs of shapes, fp32 and bf16, timed the
        same way with 20 launches per sample.
engine  synth.VIT_H14 forward_device at batch 64 with the profile on, fp32 and bf16: ms per call and the stage table, with the share
        of the attention stage.
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


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def kernel_part(B, a, out, cls=False):
    L = B.lib()
    n, T, reps = a.batch, 257, 20 if cls else 5
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        B.hip_check(L.vithip_event_create(C.byref(e)), "event_create")
    rng = np.random.default_rng(1)
    for dtype in ("f32", "bf16"):
        for (heads, hd), (heads64, _) in (((16, 80), (20, 64)), ((16, 104), (26, 64))):
            D = heads * hd
            assert D == heads64 * 64
            vals = rng.uniform(-1.5, 1.5, (n * T, 3 * D)).astype(np.float32)
            d_q = B.DeviceArray.from_numpy(vals if dtype == "f32" else B.to_bf16_bits(vals))
            d_o = B.DeviceArray((n * T, D), np.float32 if dtype == "f32" else np.uint16)
            if cls:
                d_o.free()
                d_o = B.DeviceArray((n, max(heads, heads64) * T))
                fn = L.vithip_cls_attention_f32_hd if dtype == "f32" else L.vithip_cls_attention_bf16_hd
                tail = () if dtype == "f32" else (0,)
                legs = {f"{heads}x{hd}": lambda: fn(None, d_q.ptr, 3 * D, d_o.ptr, heads * T, n, T, heads, hd, 0, *tail),
                        f"{heads64}x64": lambda: fn(None, d_q.ptr, 3 * D, d_o.ptr, heads64 * T, n, T, heads64, 64, 0, *tail)}
            elif dtype == "f32":
                legs = {f"{heads}x{hd}": lambda: L.vithip_attention_f32_hd(None, d_q.ptr, d_o.ptr, n, T, heads, hd, T),
                        f"{heads64}x64": lambda: L.vithip_attention_f32_hd(None, d_q.ptr, d_o.ptr, n, T, heads64, 64, T)}
            else:
                legs = {f"{heads}x{hd}": lambda: L.vithip_attention_bf16io_hd(None, d_q.ptr, d_o.ptr, n, T, heads, hd, T, 1),
                        f"{heads64}x64": lambda: L.vithip_attention_bf16io_hd(None, d_q.ptr, d_o.ptr, n, T, heads64, 64, T, 1)}
            order, ms = list(legs), {leg: [] for leg in legs}
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
            macs = 2 * n * heads * T * T * hd  # both products
            part = "cls" if cls else "kernel"
            for leg in order:
                med = statistics.median(ms[leg])
                rate = {"K_GBps": round(n * T * D * (4 if dtype == "f32" else 2) / (med * 1e-3) / 1e9, 1)} if cls else \
                       {"TFLOPs": round(2 * macs / (med * 1e-3) / 1e12, 1)}
                emit(out, dict({"part": part, "dtype": dtype, "shape": leg, "images": n, "tokens": T, "reps_per_sample": reps,
                                "median_ms": round(med, 4), "min_ms": round(min(ms[leg]), 4), "max_ms": round(max(ms[leg]), 4),
                                "steps": len(ms[leg])}, **rate))
            emit(out, {"part": part, "dtype": dtype, "pair": order,
                       "ratio_of_medians": round(statistics.median(ms[order[0]]) / statistics.median(ms[order[1]]), 3)})
            d_q.free()
            d_o.free()
    for e in ev:
        L.vithip_event_destroy(e)


def engine_part(pkg, B, a, out):
    cfg, n = pkg.VIT_H14, 64
    W = pkg.synth.make_weights(cfg, 1234)
    x = pkg.synth.make_images(cfg, n, 7)
    for dtype in ("f32", "bf16"):
        eng = B.Engine(cfg, max_batch=n, dtype=dtype, profile=True)
        eng.load_weights(W)
        d_x, d_p = B.DeviceArray.from_numpy(x), B.DeviceArray((n, cfg.num_classes))
        ms = []
        for step in range(a.warmup + a.steps):
            if step == a.warmup:
                eng.reset_stage_times()
            eng.sync()
            t0 = time.perf_counter()
            eng.forward_device(d_x.ptr, n, d_p.ptr)
            eng.sync()
            if step >= a.warmup:
                ms.append(1e3 * (time.perf_counter() - t0))
        st = eng.stage_times()
        calls = st["images"] / n
        stages = {s: round(v["ms"] / calls, 3) for s, v in st["stages"].items()}
        total = sum(stages.values())
        emit(out, {"part": "engine", "model": "VIT_H14", "dtype": dtype, "batch": n, "median_ms": round(statistics.median(ms), 3),
                   "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "steps": len(ms), "stage_ms_per_call": stages,
                   "attn_share_of_stages": round(stages["attn"] / total, 4)})
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--parts", default="kernel,engine")
    ap.add_argument("--out")
    a = ap.parse_args()
    pkg = importlib.import_module("vision-transformer-opencl_amd")
    B = importlib.import_module("vision-transformer-opencl_amd.binding")
    out = open(a.out, "a") if a.out else None
    parts = a.parts.split(",")
    if "kernel" in parts:
        kernel_part(B, a, out)
    if "cls" in parts:
        kernel_part(B, a, out, cls=True)
    if "engine" in parts:
        engine_part(pkg, B, a, out)


if __name__ == "__main__":
    main()
