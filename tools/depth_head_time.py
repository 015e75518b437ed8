"""Time vithip_dense_depth_f32 alone against the same tail in PyTorch, from the same g x g logits on the same GPU.

    python tools/depth_head_time.py [--batch 256] [--bins 256] [--windows 7] [--iters 5] [--parts kernel,call]

Per size (g = 16 -> 224^2, g = 37 -> 518^2; upsample 4): the median over `windows` event windows of `iters` launches each, with the
spread (min .. max), one JSON line per size.  The PyTorch tail is interpolate -> relu + 0.1 -> normalise -> einsum -> clamp ->
interpolate, which materialises the [n][bins][4g][4g] tensor the kernel never stores.
Part "call": ViT-B/16 fp32, dense_device(kind="depth") with a head over the last layer and over the last four, against
intermediate_device(kind="map") of the same layers, the two legs alternated (order reversed every other step), wall time per call.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

entry._import_pkg()
from vit_amd import binding as B  # noqa: E402


def windows(fn, n_windows, iters):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n_windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def call_part(a):
    pkg = entry._import_pkg()
    cfg, n = pkg.VIT_B16, a.batch
    g = cfg.img_size // cfg.patch_size
    eng = B.Engine(cfg, max_batch=n)
    eng.load_weights(pkg.synth.make_weights(cfg, 1234))
    d_x = B.DeviceArray.from_numpy(pkg.synth.make_images(cfg, n, 7))
    for layers in ((cfg.depth - 1,), tuple(range(cfg.depth - 4, cfg.depth))):
        C = len(layers) * 2 * cfg.embed_dim
        rng = np.random.default_rng(C)
        eng.set_depth_head((3 * rng.standard_normal((a.bins, C)) / np.sqrt(C)).astype(np.float32), rng.standard_normal(a.bins).astype(np.float32), layers)
        d_depth, d_map = B.DeviceArray((n, cfg.img_size, cfg.img_size)), B.DeviceArray((n, C // 2, g, g))
        legs = {"intermediate_map_device": lambda: eng.intermediate_device(d_x.ptr, n, d_map.ptr, layers, "map", False),
                "dense_depth_device": lambda: eng.dense_device(d_x.ptr, n, d_depth.ptr, "depth")}
        ms = {k: [] for k in legs}
        for step in range(2 + a.windows):
            for leg in (list(legs) if step % 2 == 0 else list(legs)[::-1]):
                eng.sync()
                t0 = time.perf_counter()
                legs[leg]()
                legs[leg]()
                eng.sync()
                if step >= 2:
                    ms[leg].append(1e3 * (time.perf_counter() - t0) / 2)
        rec = {"part": "call", "model": "ViT-B/16 fp32", "batch": n, "bins": a.bins, "layers": list(layers)}
        for leg, v in ms.items():
            rec[leg] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
        rec["depth_over_intermediate"] = round(rec["dense_depth_device"]["median_ms"] / rec["intermediate_map_device"]["median_ms"], 4)
        print(json.dumps(rec), flush=True)
        d_depth.free()
        d_map.free()
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="kernel,call")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--bins", type=int, default=256)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    n, bins, u, lo, hi = a.batch, a.bins, 4, 0.001, 10.0
    torch.zeros(1, device="cuda")  # PyTorch's runtime first, as bench.py has it
    if "call" in a.parts.split(","):
        call_part(a)
    for g, size in ((16, 224), (37, 518)) if "kernel" in a.parts.split(",") else ():
        torch.manual_seed(g)
        logits = 3 * torch.randn(n, g * g, bins, device="cuda")
        z = torch.randn(n, bins, device="cuda")
        centres = torch.linspace(lo, hi, bins, device="cuda")
        out = torch.empty(n, size, size, device="cuda")
        scratch = torch.empty(n, u * g, u * g, device="cuda")

        def kernel():
            B.hip_check(B.dense_depth_raw(logits.data_ptr(), bins, g * g * bins, z.data_ptr(), bins, centres.data_ptr(), out.data_ptr(), size * size,
                                          scratch.data_ptr(), n, g, bins, u, lo, hi, size, size), "vithip_dense_depth_f32")

        def tail():
            x = (logits + z[:, None]).reshape(n, g, g, bins).permute(0, 3, 1, 2)
            r = torch.relu(F.interpolate(x, size=(u * g, u * g), mode="bilinear", align_corners=False)) + 0.1
            d = torch.einsum("nbhw,b->nhw", r / r.sum(dim=1, keepdim=True), centres).clamp(lo, hi)
            return F.interpolate(d[:, None], size=(size, size), mode="bilinear", align_corners=False)[:, 0]

        rec = {"g": g, "out": size, "batch": n, "bins": bins, "kernel": windows(kernel, a.windows, a.iters)}
        ref = tail()
        rec["max_abs_diff_vs_torch"] = float((out - ref).abs().max())
        del ref
        rec["torch_tail"] = windows(tail, a.windows, max(1, a.iters // 5))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
