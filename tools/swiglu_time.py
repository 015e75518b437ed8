#!/usr/bin/env python3
"""The SwiGLU gate kernel and ViT-g/14 engines, timed (GPU box only).

    python3 tools/swiglu_time.py [--steps K] [--warmup W] [--parts kernel,layer,full] [--dtypes f32,bf16] [--out FILE.jsonl]

kernel  vithip_swiglu_f32 / vithip_swiglu_bf16 at rows = 256 * 257, H = 4096, in place with ld = 2H (the engine's layout) and with
        dense operands, against a device-to-device copy of 6 * rows * H bytes (fp32) / 3 * rows * H bytes (bf16): the copy reads
        and writes that many bytes, which is the gate's total traffic (8 read + 4 written per hidden element in fp32).  Device
        events round `reps` back-to-back launches; bytes/s = traffic / time.
layer   one encoder layer at ViT-g/14 width and 257 tokens (depth 1), batch 64 fp32 / 256 bf16: ms per call, the stage table of a
        profiled call, and the gate alone at the engine's rows and layout -- its share of the fc1 stage.
full    synth.VIT_G14 (depth 40) on synthetic weights, the same batches: images/s, ms per call, TFLOP/s against the algorithmic MACs
        of vit_config_macs_per_image, the stage table and the gate's share of fc1.

One JSON line per measurement.
"""
import argparse
import ctypes as C
import dataclasses
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS, HIDDEN = 256 * 257, 4096
BATCH = {"f32": 64, "bf16": 256}


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "mean_ms": round(statistics.fmean(ms), 4),
            "steps": len(ms)}


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


class Timer:
    """Device events round `reps` back-to-back launches on the default stream: ms per launch."""

    def __init__(self, B):
        self.B, self.L = B, B.lib()
        self.ev = [C.c_void_p(), C.c_void_p()]
        for e in self.ev:
            B.hip_check(self.L.vithip_event_create(C.byref(e)), "event_create")

    def __call__(self, launch, reps):
        B, L = self.B, self.L
        B.hip_check(L.vithip_event_record(self.ev[0], None), "record")
        for _ in range(reps):
            B.hip_check(launch(), "launch")
        B.hip_check(L.vithip_event_record(self.ev[1], None), "record")
        B.hip_check(L.vithip_event_sync(self.ev[1]), "event_sync")
        t = C.c_float()
        B.hip_check(L.vithip_event_elapsed_ms(C.byref(t), self.ev[0], self.ev[1]), "elapsed")
        return t.value / reps


def device_fill(B, nbytes):
    """nbytes of device memory holding the byte 0x3C everywhere: 0.0115 as fp32 and as bf16 (no host copy of gigabytes)."""
    p = C.c_void_p()
    B.lib().vithip_memset.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    B.hip_check(B.lib().vithip_malloc(C.byref(p), nbytes), "vithip_malloc")
    B.hip_check(B.lib().vithip_memset(p, 0x3C, nbytes, None), "memset")
    B.hip_check(B.lib().vithip_device_sync(), "sync")
    return p.value


def gate_legs(B, rows, H, dtype):
    """{leg: launch} for the gate in place at ld = 2H, the gate on dense operands, and the copy of the same traffic; and the traffic."""
    L = B.lib()
    esz, bf16 = (2, True) if dtype == "bf16" else (4, False)
    u = device_fill(B, rows * 2 * H * esz)
    h = device_fill(B, rows * H * esz)
    half = 3 * rows * H * esz // 2   # the copy reads and writes this many bytes each: 1.5 elements per hidden element, twice
    c = device_fill(B, half)         # u holds 2 * rows * H elements: the copy's source is its first three quarters
    refill = lambda: L.vithip_memset(u, 0x3C, rows * 2 * H * esz, None)
    legs = {"gate_in_place_ld2H": lambda: B.swiglu_raw(u, 2 * H, u, 2 * H, rows, H, bf16),
            "gate_dense": lambda: B.swiglu_raw(u, 2 * H, h, H, rows, H, bf16),
            "copy_same_traffic": lambda: L.vithip_memcpy_d2d(c, u, half, None)}
    return legs, 3 * rows * H * esz, refill, (u, h, c)


def kernel_part(B, a, out):
    timer = Timer(B)
    reps = 10
    for dtype in a.dtypes:
        legs, traffic, refill, bufs = gate_legs(B, ROWS, HIDDEN, dtype)
        order = list(legs)
        ms = {leg: [] for leg in legs}
        for step in range(a.warmup + a.steps):
            for leg in (order if step % 2 == 0 else order[::-1]):
                B.hip_check(refill(), "memset")   # in place, the gate half decays towards 0 launch by launch: start each sample alike
                t = timer(legs[leg], reps)
                if step >= a.warmup:
                    ms[leg].append(t)
        base = statistics.median(ms["copy_same_traffic"])
        for leg in order:
            med = statistics.median(ms[leg])
            emit(out, dict({"part": "kernel", "dtype": dtype, "launch": leg, "rows": ROWS, "H": HIDDEN, "reps_per_sample": reps,
                            "traffic_bytes": traffic, "TBps": round(traffic / (med * 1e-3) / 1e12, 3), "over_copy_median": round(med / base, 4)},
                           **stats(ms[leg])))
        for p in bufs:
            B.lib().vithip_free(p)


def engine_part(pkg, B, a, out, part):
    cfg = pkg.synth.VIT_G14 if part == "full" else dataclasses.replace(pkg.synth.VIT_G14, depth=1)
    t0 = time.perf_counter()
    W = pkg.synth.make_weights(cfg, 1234)
    emit(out, {"part": part, "note": "synthetic weights made", "seconds": round(time.perf_counter() - t0, 1), "tensors": len(W)})
    macs = int(B.lib().vit_config_macs_per_image(C.byref(B.CConfig.of(cfg))))
    timer = Timer(B)
    for dtype in a.dtypes:
        n = BATCH[dtype]
        eng = B.Engine(cfg, max_batch=n, dtype=dtype)
        t0 = time.perf_counter()
        eng.load_weights(W)
        emit(out, {"part": part, "dtype": dtype, "note": "weights installed", "seconds": round(time.perf_counter() - t0, 1)})
        d_x = B.DeviceArray.from_numpy(pkg.synth.make_images(cfg, n, 7))
        d_p = B.DeviceArray((n, cfg.num_classes))
        ms = []
        for step in range(a.warmup + a.steps):
            eng.sync()
            t0 = time.perf_counter()
            eng.forward_device(d_x.ptr, n, d_p.ptr)
            eng.sync()
            if step >= a.warmup:
                ms.append(1e3 * (time.perf_counter() - t0))
        med = statistics.median(ms)
        emit(out, dict({"part": part, "dtype": dtype, "batch": n, "depth": cfg.depth, "images_per_s": round(n / (med * 1e-3), 1),
                        "macs_per_image": macs, "TFLOPs": round(2 * macs * n / (med * 1e-3) / 1e12, 1)}, **stats(ms)))
        eng.set_profile(True)
        eng.reset_stage_times()
        for _ in range(2):
            eng.forward_device(d_x.ptr, n, d_p.ptr)
            eng.sync()
        st = eng.stage_times()
        eng.set_profile(False)
        eng.close()
        per_call = {s: round(v["ms"] / 2, 4) for s, v in st["stages"].items()}
        # the gate alone, at the engine's rows and layout
        legs, _, refill, bufs = gate_legs(B, n * cfg.tokens, cfg.hidden_dim, dtype)
        gate = []
        for _ in range(a.warmup + a.steps):
            B.hip_check(refill(), "memset")
            gate.append(timer(legs["gate_in_place_ld2H"], 5))
        for p in bufs:
            B.lib().vithip_free(p)
        g = statistics.median(gate[a.warmup:])
        emit(out, {"part": part, "dtype": dtype, "batch": n, "stage_ms_per_call": per_call,
                   "launches_per_call": {s: v["launches"] // 2 for s, v in st["stages"].items()}, "gate_ms_per_layer": round(g, 4),
                   "gate_share_of_fc1": round(g * cfg.depth / per_call["fc1"], 4),
                   "gate_share_of_call": round(g * cfg.depth / sum(per_call.values()), 4)})
        d_x.free()
        d_p.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parts", default="kernel,layer,full")
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--out")
    a = ap.parse_args()
    a.dtypes = a.dtypes.split(",")
    pkg = importlib.import_module("vision-transformer-opencl_amd")
    B = importlib.import_module("vision-transformer-opencl_amd.binding")
    out = open(a.out, "a") if a.out else None
    parts = a.parts.split(",")
    if "kernel" in parts:
        kernel_part(B, a, out)
    for part in ("layer", "full"):
        if part in parts:
            engine_part(pkg, B, a, out, part)


if __name__ == "__main__":
    main()
