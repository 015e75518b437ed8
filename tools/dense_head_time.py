#!/usr/bin/env python3
"""The dense linear head: the upsample + argmax launch against its bytes and against PyTorch, and the dense call (GPU box only).

    python3 tools/dense_head_time.py [--steps K] [--warmup W] [--calls N] [--parts kernel,torch,call] [--batch B] [--out FILE.jsonl]

kernel  vithip_dense_upsample_argmax_f32 at batch 256, 150 classes, g = 16 -> 224 x 224 and g = 37 -> 518 x 518: device events round
        `reps` back-to-back launches.  Beside the time: the bytes the launch has to move (the logits read once, a byte per pixel
        written) and the time they take at the 8.0 TB/s of the HBM's specification -- the floor the kernel is reported against.
torch   the two-pass form on the same GPU and the same logits (given to it channel-major, as it wants them):
        torch.nn.functional.interpolate(mode="bilinear", align_corners=False) writes [B][150][H][W] floats, .argmax(1) reads them
        back.  torch.cuda events round each pass pair; its labels are compared with the kernel's (they may differ where two classes
        are within rounding of each other: the count is reported, not asserted).
call    the fp32 ViT-B/16 engine at batch 256 with a 150-class head over one layer (`linear`: the last) and over four (`ms`: the last
        four): vit_engine_dense_device (labels at 224 x 224) against vit_engine_intermediate_device (MAP, norm) of the same layers,
        host clock around a window of --calls calls and a stream sync, the two legs alternated; then the stage times of profiled
        dense calls (taps in "ln", GEMMs in "head", the upsampling in "softmax").

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

CLASSES = 150
KERNEL_SHAPES = [(16, 224), (37, 518)]  # g, output side
HBM_SPEC_BYTES_PER_S = 8.0e12


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


def make_logits(n, g):
    return np.random.default_rng(g).standard_normal((n, g * g, CLASSES)).astype(np.float32)


def kernel_part(B, a, out, with_torch):
    L = B.lib()
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        B.hip_check(L.vithip_event_create(C.byref(e)), "event_create")
    torch = importlib.import_module("torch") if with_torch else None
    for g, side in KERNEL_SHAPES:
        n, P = a.batch, g * g
        logits = make_logits(n, g)
        d_l, d_o = B.DeviceArray.from_numpy(logits), B.DeviceArray((n, side, side), np.uint8)

        def launch():
            B.hip_check(B.dense_upsample_argmax_raw(d_l.ptr, CLASSES, P * CLASSES, d_o.ptr, side * side, n, g, CLASSES, side, side), "dense")

        reps, ms = 20, []
        for step in range(a.warmup + a.steps):
            B.hip_check(L.vithip_event_record(ev[0], None), "record")
            for _ in range(reps):
                launch()
            B.hip_check(L.vithip_event_record(ev[1], None), "record")
            B.hip_check(L.vithip_event_sync(ev[1]), "event_sync")
            t = C.c_float()
            B.hip_check(L.vithip_event_elapsed_ms(C.byref(t), ev[0], ev[1]), "elapsed")
            if step >= a.warmup:
                ms.append(t.value / reps)
        nbytes = logits.nbytes + n * side * side
        floor_ms = 1e3 * nbytes / HBM_SPEC_BYTES_PER_S
        rec = dict({"part": "kernel", "launch": "dense_upsample_argmax", "batch": n, "g": g, "out": side, "classes": CLASSES,
                    "reps_per_sample": reps, "bytes_moved": nbytes, "floor_ms_at_8TBps": round(floor_ms, 5)}, **stats(ms))
        rec["over_floor"] = round(rec["median_ms"] / floor_ms, 2)
        emit(out, rec)
        labels = d_o.numpy()
        if torch is not None:
            maps = torch.from_numpy(np.ascontiguousarray(logits.transpose(0, 2, 1)).reshape(n, CLASSES, g, g)).cuda()
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            tms, got = [], None
            for step in range(2 + max(a.steps // 2, 3)):
                torch.cuda.synchronize()
                start.record()
                got = torch.nn.functional.interpolate(maps, size=(side, side), mode="bilinear", align_corners=False).argmax(1)
                stop.record()
                torch.cuda.synchronize()
                if step >= 2:
                    tms.append(start.elapsed_time(stop))
            differ = int((got.to(torch.uint8).cpu().numpy() != labels).sum())
            rec = dict({"part": "torch", "launch": "interpolate+argmax", "batch": n, "g": g, "out": side, "classes": CLASSES,
                        "full_resolution_logit_bytes": 4 * n * CLASSES * side * side, "labels_differing_from_kernel": differ,
                        "pixels": int(labels.size), "over_kernel_median": round(statistics.median(tms) / statistics.median(ms), 2)}, **stats(tms))
            emit(out, rec)
            del maps, got
            torch.cuda.empty_cache()
        d_l.free()
        d_o.free()
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


def call_part(pkg, B, a, out):
    cfg, n = pkg.VIT_B16, a.batch
    g = cfg.img_size // cfg.patch_size
    eng = B.Engine(cfg, max_batch=n)
    eng.load_weights(pkg.synth.make_weights(cfg, 1234))
    d_x = B.DeviceArray.from_numpy(pkg.synth.make_images(cfg, n, 7))
    for hname, layers in (("linear", (cfg.depth - 1,)), ("ms", tuple(range(cfg.depth - 4, cfg.depth)))):
        F = len(layers) * cfg.embed_dim
        rng = np.random.default_rng(F)
        eng.set_dense_head((rng.standard_normal((CLASSES, F)) / np.sqrt(F)).astype(np.float32), rng.standard_normal(CLASSES).astype(np.float32),
                           layers, True)
        d_lab = B.DeviceArray((n, cfg.img_size, cfg.img_size), np.uint8)
        d_map = B.DeviceArray((n, F, g, g))
        ms = alternate({"intermediate_map_device": lambda: eng.intermediate_device(d_x.ptr, n, d_map.ptr, layers, "map", True),
                        "dense_labels_device": lambda: eng.dense_device(d_x.ptr, n, d_lab.ptr, "labels")}, eng.sync, a)
        base = statistics.median(ms["intermediate_map_device"])
        for leg in ms:
            emit(out, dict({"part": "call", "call": leg, "head": hname, "layers": list(layers), "dtype": "f32", "batch": n, "classes": CLASSES,
                            "calls_per_window": a.calls, "bytes_out_per_image": cfg.img_size ** 2 if leg.startswith("dense") else 4 * F * g * g,
                            "over_intermediate_median": round(statistics.median(ms[leg]) / base, 5)}, **stats(ms[leg])))
        eng.set_profile(True)
        eng.reset_stage_times()
        for _ in range(3):
            eng.dense_device(d_x.ptr, n, d_lab.ptr, "labels")
        t = eng.stage_times()
        eng.set_profile(False)
        total = sum(v["ms"] for v in t["stages"].values())
        emit(out, {"part": "call", "call": "dense_labels_device profiled", "head": hname, "batch": n, "calls": 3,
                   "stage_ms_per_call": {s: round(v["ms"] / 3, 4) for s, v in t["stages"].items()},
                   "launches_per_call": {s: v["launches"] // 3 for s, v in t["stages"].items()},
                   "upsample_share": round(t["stages"]["softmax"]["ms"] / total, 5), "head_gemm_share": round(t["stages"]["head"]["ms"] / total, 5)})
        d_lab.free()
        d_map.free()
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=2, help="calls per timed window of the call part (ms are per call)")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--parts", default="kernel,torch,call")
    ap.add_argument("--out")
    a = ap.parse_args()
    parts = a.parts.split(",")
    if "torch" in parts:  # PyTorch's runtime first, as bench.py has it: initialised behind the library's it finds no device
        import torch
        if not torch.cuda.is_available():
            sys.exit("dense_head_time.py: the torch part needs a GPU that PyTorch sees (or run with --parts kernel,call)")
        torch.cuda.set_device(0)
        torch.zeros(1, device="cuda")
    pkg = importlib.import_module("vision-transformer-opencl_amd")
    B = importlib.import_module("vision-transformer-opencl_amd.binding")
    out = open(a.out, "a") if a.out else None
    if "kernel" in parts:
        kernel_part(B, a, out, "torch" in parts)
    if "call" in parts:
        call_part(pkg, B, a, out)


if __name__ == "__main__":
    main()
