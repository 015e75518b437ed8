#!/usr/bin/env python3
"""Class-token attention maps against the CLS features call, ViT-B/16 at batch 256, device resident (GPU box only).

    python3 tools/cls_attention_time.py [--steps K] [--warmup W] [--configs f32,bf16] [--batch N] [--parts kernel,engine] [--out FILE.jsonl]

kernel  vithip_cls_attention_f32 / _bf16 alone on a random qkv of the engine's shape [n * 197][3 * 768], HEADS and HEAD_MEAN; device
        events round `reps` back-to-back launches.  Effective bytes/s over the K bytes the kernel has to read once, n * T * D
        elements (the class rows' Q and the stores are 1 % of that and not counted).  A qkv of 465 MB (fp32) does not stay in the
        256 MB last-level cache from one launch to the next; the bf16 one (232 MB) may in part: the figure says "effective".
engine  one engine per dtype: vit_engine_cls_attention_device (HEADS, HEAD_MEAN) against vit_engine_features_device(CLS) and
        vit_engine_forward_device on the same images; host clock around the call and a stream sync; steps alternate the order of
        the legs.  An attention call drops what the last layer does behind in_proj, the final LayerNorm and the head.

One JSON line per measurement (median, min, mean ms).
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


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "mean_ms": round(statistics.fmean(ms), 4),
            "steps": len(ms)}


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def kernel_part(pkg, B, a, out):
    L = B.lib()
    cfg, n = pkg.VIT_B16, a.batch
    T, heads, D = cfg.tokens, cfg.num_heads, cfg.embed_dim
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        B.hip_check(L.vithip_event_create(C.byref(e)), "event_create")
    qkv = np.random.default_rng(1).standard_normal((n * T, 3 * D)).astype(np.float32)
    for name in a.configs.split(","):
        esz = 4 if name == "f32" else 2
        d_q = B.DeviceArray.from_numpy(qkv if name == "f32" else B.to_bf16_bits(qkv))
        d_o = B.DeviceArray((n, heads, T))
        if name == "f32":
            legs = {"heads": lambda: L.vithip_cls_attention_f32(None, d_q.ptr, 3 * D, d_o.ptr, heads * T, n, T, heads, 0),
                    "head_mean": lambda: L.vithip_cls_attention_f32(None, d_q.ptr, 3 * D, d_o.ptr, T, n, T, heads, 1)}
        else:
            legs = {"heads": lambda: L.vithip_cls_attention_bf16(None, d_q.ptr, 3 * D, d_o.ptr, heads * T, n, T, heads, 0, 0),
                    "head_mean": lambda: L.vithip_cls_attention_bf16(None, d_q.ptr, 3 * D, d_o.ptr, T, n, T, heads, 1, 0)}
        k_bytes = n * T * D * esz
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
            med = statistics.median(ms[leg])
            emit(out, dict({"part": "kernel", "dtype": name, "output": leg, "images": n, "tokens": T, "heads": heads, "reps_per_sample": reps,
                            "k_bytes": k_bytes, "effective_GBps": round(k_bytes / (med * 1e-3) / 1e9, 1)}, **stats(ms[leg])))
        d_q.free()
        d_o.free()
    for e in ev:
        L.vithip_event_destroy(e)


def engine_part(pkg, B, a, out):
    cfg, n = pkg.VIT_B16, a.batch
    W = pkg.synth.make_weights(cfg, 1234)
    for name in a.configs.split(","):
        eng = B.Engine(cfg, max_batch=n, dtype=name)
        eng.load_weights(W)
        d_x = B.DeviceArray.from_numpy(pkg.synth.make_images(cfg, n, 7))
        d_probs, d_row = B.DeviceArray((n, cfg.num_classes)), B.DeviceArray((n, cfg.embed_dim))
        d_map = B.DeviceArray((n, cfg.num_heads, cfg.tokens))
        legs = {"probs": lambda: eng.forward_device(d_x.ptr, n, d_probs.ptr),
                "features_cls": lambda: eng.features_device(d_x.ptr, n, d_row.ptr, "cls"),
                "attention_heads": lambda: eng.cls_attention_device(d_x.ptr, n, d_map.ptr, "heads"),
                "attention_head_mean": lambda: eng.cls_attention_device(d_x.ptr, n, d_map.ptr, "head_mean")}
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
        base = statistics.median(ms["features_cls"])
        for leg in order:
            emit(out, dict({"part": "engine", "dtype": name, "batch": n, "output": leg,
                            "over_features_cls_median": round(statistics.median(ms[leg]) / base, 4)}, **stats(ms[leg])))
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--configs", default="f32,bf16")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--parts", default="kernel,engine")
    ap.add_argument("--out")
    a = ap.parse_args()
    pkg = importlib.import_module("vision-transformer-opencl_amd")
    B = importlib.import_module("vision-transformer-opencl_amd.binding")
    out = open(a.out, "a") if a.out else None
    parts = a.parts.split(",")
    if "kernel" in parts:
        kernel_part(pkg, B, a, out)
    if "engine" in parts:
        engine_part(pkg, B, a, out)


if __name__ == "__main__":
    main()
