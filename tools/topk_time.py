#!/usr/bin/env python3
"""Top-k records against the probabilities: the launch, the device-resident call and the host-pointer call (GPU box only).

    python3 tools/topk_time.py [--steps K] [--warmup W] [--calls N] [--parts kernel,device,host] [--out FILE.jsonl]

kernel  vithip_softmax_topk_f32 at 256 rows x 1000 classes for k = 1, 5, 64 (PROB; the row's probabilities live in LDS) beside
        vithip_softmax_top1_f32 on the same logits, and both at 256 x 21,843 (k = 5: the row is recomputed in every selection round);
        device events round `reps` back-to-back launches, the legs of a shape alternated (A B C D, D C B A, ...).
device  the fp32 ViT-B/16 engine at batch 256: vit_engine_topk_device (k = 5) against vit_engine_forward_device on the same images,
        host clock around a window of --calls calls and a stream sync, the two legs alternated.
host    the same engine: vit_engine_topk_host (k = 5) against vit_engine_forward_host on 256 separately allocated images.

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

KERNEL_SHAPES = [(256, 1000, (1, 5, 64)), (256, 21843, (5,))]


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
    for rows, classes, ks in KERNEL_SHAPES:
        logits = (np.random.default_rng(classes).standard_normal((rows, classes)) * 3).astype(np.float32)
        d_l = B.DeviceArray.from_numpy(logits)
        d_p, d_lab, d_pr = B.DeviceArray((rows, classes)), B.DeviceArray((rows,), np.int32), B.DeviceArray((rows,))
        d_rec = B.DeviceArray((rows, 2 * 64), np.int32)
        legs = {"softmax_top1": lambda: L.vithip_softmax_top1_f32(None, d_l.ptr, classes, d_p.ptr, classes, d_lab.ptr, d_pr.ptr, rows, classes)}
        for k in ks:
            legs[f"topk_k{k}"] = lambda k=k: L.vithip_softmax_topk_f32(None, d_l.ptr, classes, d_rec.ptr, 2 * k, rows, classes, k, 0)
        reps = 2000
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
        base = statistics.median(ms["softmax_top1"])
        for leg in order:
            emit(out, dict({"part": "kernel", "launch": leg, "rows": rows, "classes": classes, "reps_per_sample": reps,
                            "over_softmax_top1_median": round(statistics.median(ms[leg]) / base, 4)}, **stats(ms[leg])))
        for d in (d_l, d_p, d_lab, d_pr, d_rec):
            d.free()
    for e in ev:
        L.vithip_event_destroy(e)


def alternate(legs, sync, a):
    order = list(legs)
    ms = {leg: [] for leg in legs}
    for step in range(a.warmup + a.steps):
        for leg in (order if step % 2 == 0 else order[::-1]):
            sync()
            t0 = time.perf_counter()
            for _ in range(a.calls):
                legs[leg]()
            sync()
            if step >= a.warmup:
                ms[leg].append(1e3 * (time.perf_counter() - t0) / a.calls)
    return ms


def engine_parts(pkg, B, a, out, parts):
    cfg, n, k = pkg.VIT_B16, 256, 5
    eng = B.Engine(cfg, max_batch=n)
    eng.load_weights(pkg.synth.make_weights(cfg, 1234))
    imgs = pkg.synth.make_images(cfg, n, 7)
    if "device" in parts:
        d_x = B.DeviceArray.from_numpy(imgs)
        d_probs, d_rec = B.DeviceArray((n, cfg.num_classes)), B.DeviceArray((n, 2 * k), np.int32)
        ms = alternate({"forward_device": lambda: eng.forward_device(d_x.ptr, n, d_probs.ptr),
                        "topk_device": lambda: eng.topk_device(d_x.ptr, n, d_rec.ptr, k)}, eng.sync, a)
        base = statistics.median(ms["forward_device"])
        for leg in ms:
            emit(out, dict({"part": "device", "call": leg, "dtype": "f32", "batch": n, "k": k, "calls_per_window": a.calls,
                            "over_forward_median": round(statistics.median(ms[leg]) / base, 5)}, **stats(ms[leg])))
    if "host" in parts:
        sep = [np.array(im) for im in imgs]  # separately allocated, as the host path's callers hold them
        in_ptrs = (B.f32p * n)(*[im.ctypes.data_as(B.f32p) for im in sep])
        probs, rec = np.empty((n, cfg.num_classes), np.float32), np.empty((n, 2 * k), np.int32)
        p_rows = (B.f32p * n)(*[probs[i].ctypes.data_as(B.f32p) for i in range(n)])
        r_rows = (B.i32p * n)(*[rec[i].ctypes.data_as(B.i32p) for i in range(n)])
        spec = B.topk_spec(k)
        L = B.lib()

        def check(rc):
            if rc:
                raise SystemExit(f"call failed ({rc}): {L.vit_engine_last_error(eng._h).decode()}")

        ms = alternate({"forward_host": lambda: check(L.vit_engine_forward_host(eng._h, in_ptrs, n, p_rows)),
                        "topk_host": lambda: check(L.vit_engine_topk_host(eng._h, in_ptrs, n, C.byref(spec), r_rows))}, eng.sync, a)
        base = statistics.median(ms["forward_host"])
        for leg in ms:
            emit(out, dict({"part": "host", "call": leg, "dtype": "f32", "batch": n, "k": k,
                            "bytes_down_per_image": 8 * k if leg == "topk_host" else 4 * cfg.num_classes,
                            "over_forward_median": round(statistics.median(ms[leg]) / base, 5)}, **stats(ms[leg])))
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=4, help="calls per timed window of the device and host parts (ms are per call)")
    ap.add_argument("--parts", default="kernel,device,host")
    ap.add_argument("--out")
    a = ap.parse_args()
    pkg = importlib.import_module("vision-transformer-opencl_amd")
    B = importlib.import_module("vision-transformer-opencl_amd.binding")
    out = open(a.out, "a") if a.out else None
    parts = a.parts.split(",")
    if "kernel" in parts:
        kernel_part(B, a, out)
    if "device" in parts or "host" in parts:
        engine_parts(pkg, B, a, out, parts)


if __name__ == "__main__":
    main()
