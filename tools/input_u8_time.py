#!/usr/bin/env python3
"""8-bit input against fp32 input, ViT-B/16: ms per forward of the same images, the two legs alternated in one process (GPU box only).

    python3 tools/input_u8_time.py [--steps K] [--warmup W] [--configs f32,bf16] [--paths device,host]
    python3 tools/input_u8_time.py --summarize KERNEL_STATS_CSV [--images N]   (no GPU)

Configurations: the fp32 engine at batch 256, the bf16 engine at batch 2048 (BASELINE.json configs[1], configs[2]).  Paths:
  device  vit_engine_forward_device (fp32 [n][3][224][224] in HBM) against vit_engine_forward_device_u8 ([n][224][224][3] bytes in
          HBM, normalised by the engine), host clock around the call and a stream sync;
  host    vit_engine_forward_host against vit_engine_forward_host_u8: separately addressed pageable images, gathered, uploaded and
          computed through the double-buffered pipeline, blocking.
The fp32 images are the u8 images normalised on the host by the same formula, so every leg's probabilities must be the same bits
(checked once per configuration and path).  Steps alternate A B B A ...; one JSON line per measurement (median, min, mean ms).

--summarize reads the kernel statistics of a `rocprofv3 --kernel-trace --stats` run of this tool (restricted to one configuration so
that every launch of the conversion kernel has the same size) and prints the conversion kernel's rate: n * S^2 * C * 5 bytes (one
read, four written per element) over its average duration.
"""
import argparse
import csv
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
KERNEL = "images_u8_hwc_to_f32_chw_kernel"


def normalise(imgs, mean, std):
    x = np.ascontiguousarray(np.moveaxis(imgs, -1, 1)).astype(np.float32)
    return (x / np.float32(255.0) - np.asarray(mean, np.float32)[None, :, None, None]) / np.asarray(std, np.float32)[None, :, None, None]


def summarize(path, images):
    S, C = 224, 3
    with open(path) as f:
        rows = [r for r in csv.DictReader(f) if KERNEL in r.get("Name", "")]
    if not rows:
        sys.exit(f"{path}: no {KERNEL} launches")
    r = rows[0]
    avg_ns = float(r["AverageNs"])
    nbytes = images * S * S * C * 5
    print(json.dumps({"kernel": r["Name"], "calls": int(r["Calls"]), "images": images, "average_us": round(avg_ns / 1e3, 2),
                      "min_us": round(float(r["MinNs"]) / 1e3, 2), "bytes": nbytes,
                      "effective_TBps": round(nbytes / avg_ns / 1e3, 3)}))


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return 1e3 * (time.perf_counter() - t0)


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "mean_ms": round(statistics.fmean(ms), 3),
            "steps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--configs", default="f32,bf16")
    ap.add_argument("--paths", default="device,host")
    ap.add_argument("--summarize")
    ap.add_argument("--images", type=int, default=256)
    a = ap.parse_args()
    if a.summarize:
        return summarize(a.summarize, a.images)

    pkg = importlib.import_module("vision-transformer-opencl_amd")
    B = importlib.import_module("vision-transformer-opencl_amd.binding")
    cfg = pkg.VIT_B16
    mean, std = B.IMAGENET_MEAN, B.IMAGENET_STD
    W = pkg.synth.make_weights(cfg, 1234)
    for name in a.configs.split(","):
        n = CONFIGS[name]
        imgs = np.random.default_rng(7).integers(0, 256, size=(n, cfg.img_size, cfg.img_size, cfg.in_chans), dtype=np.uint8)
        x = normalise(imgs, mean, std)
        eng = B.Engine(cfg, max_batch=n, dtype=name)
        eng.load_weights(W)
        for path in a.paths.split(","):
            probs = {}
            if path == "device":
                d_x, d_u8 = B.DeviceArray.from_numpy(x), B.DeviceArray.from_numpy(imgs)
                d_out = {leg: B.DeviceArray((n, cfg.num_classes)) for leg in ("fp32", "u8")}
                legs = {"fp32": lambda: eng.forward_device(d_x.ptr, n, d_out["fp32"].ptr),
                        "u8": lambda: eng.forward_device_u8(d_u8.ptr, n, d_out["u8"].ptr, mean, std)}
                read = {leg: d_out[leg].numpy for leg in legs}
            else:
                out = {}
                legs = {"fp32": lambda: out.__setitem__("fp32", eng.forward(x)),
                        "u8": lambda: out.__setitem__("u8", eng.forward_u8(imgs, mean, std))}
                read = {leg: (lambda leg=leg: out[leg]) for leg in legs}
            ms = {leg: [] for leg in legs}
            order = ["fp32", "u8"]
            for step in range(a.warmup + a.steps):
                for leg in (order if step % 2 == 0 else order[::-1]):
                    t = timed(legs[leg], eng.sync)
                    if step >= a.warmup:
                        ms[leg].append(t)
                    if step == 0:
                        probs[leg] = read[leg]().copy()
            same = bool(np.array_equal(probs["fp32"].view(np.uint32), probs["u8"].view(np.uint32)))
            for leg in order:
                in_bytes = n * cfg.img_size * cfg.img_size * cfg.in_chans * (4 if leg == "fp32" else 1)
                print(json.dumps(dict({"dtype": name, "batch": n, "path": path, "input": leg, "input_bytes": in_bytes}, **stats(ms[leg]))),
                      flush=True)
            r = statistics.median(ms["u8"]) / statistics.median(ms["fp32"])
            print(json.dumps({"dtype": name, "batch": n, "path": path, "u8_over_fp32_median": round(r, 4), "bitwise_equal": same}),
                  flush=True)
            if not same:
                sys.exit(f"{name} {path}: u8 and fp32 probabilities differ")
        eng.close()


if __name__ == "__main__":
    main()
