#!/usr/bin/env python3
"""Time the fp32 patch embeddings (implicit GEMMs over NCHW fp32 images) at batch 256.  GPU box only.

  python tools/embed_f32_time.py [batch]
      vithip_patch_embed_f32 at (224, 16, 3, 768), per tile shape with the probe build (tile override):
      VIT_HIP_LIBRARY=.../libvit_mi355x_probe.so python tools/embed_f32_time.py
  python tools/embed_f32_time.py [batch] --legs old:16,general:14,general:16 [--img 224 --chans 3 --dim 768 --rounds 5]
      warm, alternated legs in one process: KERNEL:PATCH, KERNEL = old (vithip_patch_embed_f32) | general
      (vithip_patch_embed_f32_general).  224 / 14 and 224 / 16 are the same pixels and the same MAC count
      (256 patches x 588 = 196 x 768).  One JSON line per leg and round, then the medians and the ratios to the first leg."""
import argparse, importlib, json, os, statistics, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B = importlib.import_module("vision-transformer-opencl_amd.binding")
from tools.gemm_probe import timed
ap = argparse.ArgumentParser()
ap.add_argument("batch", nargs="?", type=int, default=256)
ap.add_argument("--legs", default="")
ap.add_argument("--img", type=int, default=224)
ap.add_argument("--chans", type=int, default=3)
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()
n = args.batch
L = B.lib()
rng = np.random.default_rng(0)
img = B.DeviceArray.from_numpy(rng.uniform(-2, 2, (n, args.chans, args.img, args.img)).astype(np.float32))

if args.legs:
    legs = []
    for leg in args.legs.split(","):
        kernel, patch = leg.split(":")
        patch = int(patch)
        K, T = args.chans * patch * patch, (args.img // patch) ** 2 + 1
        fn = {"old": L.vithip_patch_embed_f32, "general": L.vithip_patch_embed_f32_general}[kernel]
        w = B.DeviceArray.from_numpy(rng.uniform(-.05, .05, (args.dim, K)).astype(np.float32))
        b, cls, pos, x = B.DeviceArray((args.dim,)), B.DeviceArray((args.dim,)), B.DeviceArray((T, args.dim)), B.DeviceArray((n * T, args.dim))
        call = lambda fn=fn, w=w, b=b, cls=cls, pos=pos, x=x, patch=patch: B.hip_check(
            fn(None, img.ptr, w.ptr, b.ptr, cls.ptr, pos.ptr, x.ptr, n, args.img, patch, args.chans, args.dim))
        legs.append((leg, call, 2.0 * n * (T - 1) * K * args.dim))
    for _, call, _ in legs:  # every shape warm before the first timed window
        timed(call, reps=3, warm=3)
    times = {leg: [] for leg, _, _ in legs}
    for rnd in range(args.rounds):
        for leg, call, flop in legs:
            ms = timed(call, reps=100, warm=2)  # includes the class-row launch of each call
            times[leg].append(ms)
            print(json.dumps({"round": rnd, "leg": leg, "embed_ms": round(ms, 4), "tflops": round(flop / ms / 1e9, 1)}))
    med = {leg: statistics.median(v) for leg, v in times.items()}
    first = legs[0][0]
    print(json.dumps({"batch": n, "img": args.img, "dim": args.dim, "median_ms": {k: round(v, 4) for k, v in med.items()},
                      "min_ms": {k: round(min(v), 4) for k, v in times.items()}, "max_ms": {k: round(max(v), 4) for k, v in times.items()},
                      "ratio_to_" + first: {k: round(v / med[first], 3) for k, v in med.items()}}))
    sys.exit(0)

w = B.DeviceArray.from_numpy(rng.uniform(-.05, .05, (768, 768)).astype(np.float32))
b = B.DeviceArray((768,)); cls = B.DeviceArray((768,)); pos = B.DeviceArray((197, 768)); x = B.DeviceArray((n * 197, 768))
flop = 2.0 * n * 196 * 768 * 768
for rnd in range(2):
    for tile in (0, 10, 3):   # 0 = pipelined 128x64 (the default), 10 = pipelined 128x128, 3 = classic 128x64 (the round-2 kernel)
        if hasattr(L, "vithip_gemm_set_tile"):
            L.vithip_gemm_set_tile(tile)
        elif tile:
            continue
        ms = min(timed(lambda: B.hip_check(L.vithip_patch_embed_f32(None, img.ptr, w.ptr, b.ptr, cls.ptr, pos.ptr, x.ptr, n, 224, 16, 3, 768)), reps=5, warm=2) for _ in range(3))
        print(json.dumps({"tile": tile, "embed_ms": round(ms, 4), "tflops": round(flop / ms / 1e9, 1)}))
if hasattr(L, "vithip_gemm_set_tile"):
    L.vithip_gemm_set_tile(0)
