#!/usr/bin/env python3
"""k-NN over a feature gallery: the fused launch against PyTorch's matmul + topk, the floor, and the engine call (GPU box only).

    python3 tools/knn_time.py [--steps K] [--warmup W] [--reps R] [--parts kernel,slices,engine] [--small] [--out FILE.jsonl]

kernel  256 unit queries against banks of 1,281,167 x 768 and x 1024 (fp32 and bf16, k = 10, 200) and 21,843 x 512 (k = 10):
        vithip_knn_topk_* beside torch.topk(q @ bank.T, k) with the bank in the same dtype, device events round `reps` launches, the
        two legs alternated; the floor max(bank bytes / HBM rate, matrix flops / matrix rate); and the records checked against the
        torch result's float64 recomputation under the rule of tests/test_gpu_knn_kernel.py (bar (D + 2) 2^-24 |q|.|b|).
slices  the same launch at 1,281,167 x 768 (k = 10) for slices = 8 .. 256 beside the launcher's own choice (slices = 0).
engine  ViT-B/16 fp32 at batch 256: vit_engine_neighbours_device (k = 10, CLS, a 1,281,167 x 768 fp32 gallery) over
        vit_engine_features_device on the same images.
--small swaps 1,281,167 for 40,000 rows (a rehearsal; its numbers measure overheads).

The bank is made on the device from a seed.  One JSON line per leg.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12                                # MI355X HBM3E
MATRIX_FLOPS = {"f32": 157.3e12, "bf16": 2.5e15 / 3}    # fp32 MFMA; bf16 dense, three products per query piece
N = 256


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def stats(ms):
    med = statistics.median(ms)
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "steps": len(ms)}


def unit_rows(torch, rows, D, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((rows, D), generator=g, device="cuda", dtype=torch.float32)
    return x / x.norm(dim=1, keepdim=True)


def timed(torch, legs, a):
    """median-able ms per launch of every leg, the legs alternated inside every step"""
    ms = {leg: [] for leg in legs}
    order = list(legs)
    for step in range(a.warmup + a.steps):
        for leg in (order if step % 2 == 0 else order[::-1]):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.reps):
                legs[leg]()
            t1.record()
            t1.synchronize()
            if step >= a.warmup:
                ms[leg].append(t0.elapsed_time(t1) / a.reps)
    return ms


def launcher(torch, B, q, bank, k, slices):
    """(call, records tensor): vithip_knn_topk_* on torch tensors, on the stream torch itself uses (the NULL stream)"""
    L = B.lib()
    G, D = bank.shape
    rec = torch.empty((N, 2 * k), dtype=torch.int32, device="cuda")
    ws = torch.empty(max(L.vithip_knn_workspace_bytes(N, G, k, slices) // 4, 1), dtype=torch.int32, device="cuda")
    fn = L.vithip_knn_topk_bf16bank if bank.dtype == torch.bfloat16 else L.vithip_knn_topk_f32
    return (lambda: B.hip_check(fn(None, q.data_ptr(), D, N, bank.data_ptr(), D, G, D, k, rec.data_ptr(), 2 * k, ws.data_ptr(), slices), "knn")), rec


def check_records(torch, rec, q, bank, k):
    """the rule of test 1 on the device, the bank taken a block of rows at a time; returns (worst |error| / bar, rows above the bar)"""
    D = q.shape[1]
    q64 = q.double()
    idx, sc = rec[:, :k].long(), rec[:, k:].contiguous().view(torch.float32).double()
    assert (idx >= 0).all() and (idx < bank.shape[0]).all() and (sc[:, 1:] <= sc[:, :-1]).all()
    assert all(len(set(r)) == k for r in idx[:8].tolist())
    eps = (D + 2) * 2.0 ** -24
    b_got = bank[idx.reshape(-1)].double().reshape(N, k, D)
    exact = torch.einsum("nd,nkd->nk", q64, b_got)
    bar = eps * torch.einsum("nd,nkd->nk", q64.abs(), b_got.abs())
    worst = float(((sc - exact).abs() / bar).max())
    missed = 0
    for lo in range(0, bank.shape[0], 1 << 16):
        blk = bank[lo:lo + (1 << 16)].double()
        over = q64 @ blk.T > sc[:, -1:] + eps * (q64.abs() @ blk.abs().T) + bar[:, -1:]
        inside = (idx >= lo) & (idx < lo + blk.shape[0])
        rows = torch.arange(N, device="cuda")[:, None].expand_as(idx)[inside]
        over[rows, idx[inside] - lo] = False
        missed += int(over.sum())
    return worst, missed


def kernel_part(torch, B, a, out, big):
    shapes = [(big, 768, ("f32", "bf16"), (10, 200)), (big, 1024, ("f32", "bf16"), (10, 200)), (21843, 512, ("f32", "bf16"), (10,))]
    for G, D, dtypes, ks in shapes:
        q = unit_rows(torch, N, D, 1)
        for dtype in dtypes:
            bank = unit_rows(torch, G, D, 2)
            if dtype == "bf16":
                bank = bank.to(torch.bfloat16)
            qt = q.to(bank.dtype)
            for k in ks:
                call, rec = launcher(torch, B, q, bank, k, 0)
                ms = timed(torch, {"knn_topk": call, "torch_matmul_topk": lambda: torch.topk(qt @ bank.T, k)}, a)
                call()
                torch.cuda.synchronize()
                worst, missed = check_records(torch, rec, q, bank, k)
                floor = max(bank.numel() * bank.element_size() / HBM_BYTES_PER_S, 2.0 * N * G * D / MATRIX_FLOPS[dtype]) * 1e3
                ref = statistics.median(ms["torch_matmul_topk"])
                for leg in ms:
                    emit(out, dict({"part": "kernel", "leg": leg, "G": G, "D": D, "bank": dtype, "k": k, "bank_GiB": round(bank.numel() * bank.element_size() / 2 ** 30, 2),
                                    "slices": B.lib().vithip_knn_slices(N, G, 0), "floor_ms": round(floor, 4),
                                    "over_floor": round(statistics.median(ms[leg]) / floor, 2), "over_torch": round(statistics.median(ms[leg]) / ref, 3),
                                    "worst_error_over_bar": round(worst, 3), "omitted_above_bar": missed}, **stats(ms[leg])))
                assert worst <= 1.0 and missed == 0, (G, D, dtype, k, worst, missed)
            del bank


def slices_part(torch, B, a, out, big):
    D, k = 768, 10
    q = unit_rows(torch, N, D, 1)
    for dtype in ("f32", "bf16"):
        bank = unit_rows(torch, big, D, 2)
        if dtype == "bf16":
            bank = bank.to(torch.bfloat16)
        legs = {f"slices_{s}": launcher(torch, B, q, bank, k, s)[0] for s in (0, 8, 16, 32, 64, 128, 256)}
        ms = timed(torch, legs, a)
        for leg in ms:
            emit(out, dict({"part": "slices", "leg": leg, "G": big, "D": D, "bank": dtype, "k": k, "rule": B.lib().vithip_knn_slices(N, big, 0)}, **stats(ms[leg])))
        del bank


def engine_part(torch, pkg, B, a, out, big):
    cfg, k = pkg.VIT_B16, 10
    eng = B.Engine(cfg, max_batch=N)
    eng.load_weights(pkg.synth.make_weights(cfg, 1234))
    bank = unit_rows(torch, big, cfg.embed_dim, 2)
    eng._check(B.lib().vit_engine_set_gallery(eng._h, bank.data_ptr(), big, cfg.embed_dim, 0, 1), "vit_engine_set_gallery")
    del bank
    d_x = B.DeviceArray.from_numpy(pkg.synth.make_images(cfg, N, 7))
    d_f, d_r = B.DeviceArray((N, cfg.embed_dim)), B.DeviceArray((N, 2 * k), np.int32)
    a1 = argparse.Namespace(steps=a.steps, warmup=a.warmup, reps=2)
    ms = timed(torch, {"features_device": lambda: (eng.features_device(d_x.ptr, N, d_f.ptr, "cls", True), eng.sync()),
                       "neighbours_device": lambda: (eng.neighbours_device(d_x.ptr, N, d_r.ptr, k, "cls", 1), eng.sync())}, a1)
    base = statistics.median(ms["features_device"])
    for leg in ms:
        emit(out, dict({"part": "engine", "call": leg, "dtype": "f32", "batch": N, "k": k, "G": big,
                        "over_features_median": round(statistics.median(ms[leg]) / base, 4)}, **stats(ms[leg])))
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5, help="launches per timed window")
    ap.add_argument("--parts", default="kernel,slices,engine")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("knn_time.py needs the GPU: no timing without one")
    pkg = importlib.import_module("vision-transformer-opencl_amd")
    B = importlib.import_module("vision-transformer-opencl_amd.binding")
    out = open(a.out, "a") if a.out else None
    big = 40000 if a.small else 1281167
    parts = a.parts.split(",")
    if "kernel" in parts:
        kernel_part(torch, B, a, out, big)
    if "slices" in parts:
        slices_part(torch, B, a, out, big)
    if "engine" in parts:
        engine_part(torch, pkg, B, a, out, big)


if __name__ == "__main__":
    main()
