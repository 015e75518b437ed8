#!/usr/bin/env python3
"""The QuickGELU epilogue against the erf-GELU one on the same fc1 launch, and CLIP towers end to end (GPU box only).

    python3 tools/clip_time.py [--steps K] [--warmup W] [--parts fc1,towers] [--dtypes f32,bf16] [--towers b16,l14] [--out FILE.jsonl]

fc1     the fc1 GEMM of ViT-B/16 (N = 3072, K = 768) at batch 256 fp32 (M = 50,432; both arithmetics, the split with the pre-split
        weight image as the engine runs it) and batch 2048 bf16 (M = 403,456), with VITHIP_EPI_BIAS_QGELU / VITHIP_BF16_EPI_BF16_QGELU
        and with the GELU role in its place: the same operands, the same dispatch, alternated sample by sample.  Device events round
        `reps` back-to-back launches.
towers  synth.CLIP_B16 and synth.CLIP_L14 on synthetic weights with eps 1e-5 and a pre-norm: ms per call, images/s, the stage table
        of a profiled call, and the pre-norm launch alone (vithip_layernorm_f32_eps in place on batch * tokens rows) -- its share of
        the LayerNorm stage and of the call.

One JSON line per measurement.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCH = {"b16": {"f32": 256, "bf16": 2048}, "l14": {"f32": 128, "bf16": 1024}}


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "steps": len(ms)}


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


def device_fill(B, nbytes, byte=0x3C):
    """nbytes of device memory holding `byte` everywhere (0x3C: 0.0115 as fp32 and as bf16)."""
    p = C.c_void_p()
    B.lib().vithip_memset.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    B.hip_check(B.lib().vithip_malloc(C.byref(p), nbytes), "vithip_malloc")
    B.hip_check(B.lib().vithip_memset(p, byte, nbytes, None), "memset")
    B.hip_check(B.lib().vithip_device_sync(), "sync")
    return p.value


def fc1_part(pkg, B, a, out):
    import numpy as np
    L = B.lib()
    timer = Timer(B)
    N, K, T = 3072, 768, 197
    W = B.DeviceArray.from_numpy(pkg.synth.uniform(1, 1, N * K, -0.08, 0.08).reshape(N, K))
    bias = B.DeviceArray.from_numpy(pkg.synth.uniform(1, 2, N, -0.1, 0.1))
    for dtype in a.dtypes:
        M = BATCH["b16"][dtype] * T
        rng_rows = pkg.synth.uniform(1, 3, 4096 * K, -1.0, 1.0).reshape(4096, K)     # 4,096 distinct rows, repeated down the operand
        A_host = np.ascontiguousarray(np.tile(rng_rows, ((M + 4095) // 4096, 1))[:M])
        variants = []
        if dtype == "f32":
            dA, dC = B.DeviceArray.from_numpy(A_host), B.DeviceArray((M, N))
            dImg = B.split3_weights_device(W, N, K, K)
            for arith, name in ((B.ARITH_SPLIT3, "split3+image"), (B.ARITH_F32, "fp32-mfma")):
                def make(epi, arith=arith):
                    args = B.CGemmArgs(dA.ptr, K, W.ptr, K, bias.ptr, None, N, dC.ptr, N, M, N, K, epi, 0, 0, None, 0, None, None, None, None, arith)
                    if arith == B.ARITH_SPLIT3:
                        args.w_split = dImg.ptr
                    return lambda: L.vithip_gemm_f32(None, C.byref(args))
                variants.append((name, {"quickgelu": make(B.EPI_BIAS_QGELU), "gelu": make(B.EPI_BIAS_GELU), "bias": make(B.EPI_BIAS)}))
        else:
            L.vithip_gemm_bf16.argtypes = [C.c_void_p, C.POINTER(B.CGemmBf16Args)]
            dA, dW = B.DeviceArray.from_numpy(B.to_bf16_bits(A_host)), B.DeviceArray.from_numpy(B.to_bf16_bits(W.numpy()))
            dC = B.DeviceArray((M, N), np.uint16)

            def make(epi):
                args = B.CGemmBf16Args(dA.ptr, K, dW.ptr, K, bias.ptr, None, N, dC.ptr, N, M, N, K, epi, 0, None, None, None, N, None)
                return lambda: L.vithip_gemm_bf16(None, C.byref(args))
            variants.append(("ping-pong", {"quickgelu": make(B.BF16_EPI_BF16_QGELU), "gelu": make(B.BF16_EPI_BF16_GELU), "bias": make(B.BF16_EPI_BF16)}))
        reps = 5
        for name, legs in variants:
            order = list(legs)
            ms = {leg: [] for leg in legs}
            for step in range(a.warmup + a.steps):
                for leg in (order if step % 2 == 0 else order[::-1]):
                    t = timer(legs[leg], reps)
                    if step >= a.warmup:
                        ms[leg].append(t)
            base = statistics.median(ms["gelu"])
            for leg in order:
                med = statistics.median(ms[leg])
                emit(out, dict({"part": "fc1", "dtype": dtype, "kernel": name, "epilogue": leg, "M": M, "N": N, "K": K, "reps_per_sample": reps,
                                "TFLOPs": round(2.0 * M * N * K / (med * 1e-3) / 1e12, 1), "over_gelu_median": round(med / base, 4)}, **stats(ms[leg])))
        del dA, dC


def towers_part(pkg, B, a, out):
    L = B.lib()
    timer = Timer(B)
    L.vithip_layernorm_f32_eps.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double]
    for tower in a.towers:
        cfg = {"b16": pkg.synth.CLIP_B16, "l14": pkg.synth.CLIP_L14}[tower]
        t0 = time.perf_counter()
        W = pkg.synth.make_weights(cfg, 1234)
        D = cfg.embed_dim
        gamma, beta = pkg.synth.uniform(1234, 9001, D, 0.5, 1.5), pkg.synth.uniform(1234, 9002, D, -0.3, 0.3)
        emit(out, {"part": "towers", "tower": tower, "note": "synthetic weights made", "seconds": round(time.perf_counter() - t0, 1)})
        macs = int(L.vit_config_macs_per_image(C.byref(B.CConfig.of(cfg))))
        for dtype in a.dtypes:
            n = BATCH[tower][dtype]
            eng = B.Engine(cfg, max_batch=n, dtype=dtype)
            eng.set_layernorm_eps(1e-5)
            eng.load_weights(W)
            eng.set_pre_norm(gamma, beta)
            d_x = B.DeviceArray.from_numpy(pkg.synth.make_images(cfg, n, 7))
            d_p = B.DeviceArray((n, cfg.num_classes))
            ms = []
            for step in range(a.warmup + a.steps):
                eng.sync()
                t0 = time.perf_counter()
                eng.features_device(d_x.ptr, n, d_p.ptr, "head", True)
                eng.sync()
                if step >= a.warmup:
                    ms.append(1e3 * (time.perf_counter() - t0))
            med = statistics.median(ms)
            emit(out, dict({"part": "towers", "tower": tower, "dtype": dtype, "batch": n, "call": "features(head, l2)", "images_per_s": round(n / (med * 1e-3), 1),
                            "macs_per_image": macs, "TFLOPs": round(2 * macs * n / (med * 1e-3) / 1e12, 1)}, **stats(ms)))
            eng.set_profile(True)
            eng.reset_stage_times()
            for _ in range(2):
                eng.features_device(d_x.ptr, n, d_p.ptr, "head", True)
                eng.sync()
            st = eng.stage_times()
            eng.set_profile(False)
            eng.close()
            per_call = {s: round(v["ms"] / 2, 4) for s, v in st["stages"].items()}
            rows = n * cfg.tokens
            x = device_fill(B, rows * D * 4)
            dg, db = B.DeviceArray.from_numpy(gamma), B.DeviceArray.from_numpy(beta)
            pre = []
            for _ in range(a.warmup + a.steps):
                B.hip_check(L.vithip_memset(x, 0x3C, rows * D * 4, None), "memset")   # in place: start each sample alike
                pre.append(timer(lambda: L.vithip_layernorm_f32_eps(None, x, D, x, D, dg.ptr, db.ptr, rows, D, 1e-5), 3))
            L.vithip_free(x)
            p = statistics.median(pre[a.warmup:])
            emit(out, {"part": "towers", "tower": tower, "dtype": dtype, "batch": n, "stage_ms_per_call": per_call,
                       "launches_per_call": {s: v["launches"] // 2 for s, v in st["stages"].items()}, "pre_norm_ms": round(p, 4),
                       "pre_norm_share_of_ln_stage": round(p / per_call["ln"], 4), "pre_norm_share_of_call": round(p / sum(per_call.values()), 4)})
            d_x.free()
            d_p.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parts", default="fc1,towers")
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--towers", default="b16,l14")
    ap.add_argument("--out")
    a = ap.parse_args()
    a.dtypes, a.towers = a.dtypes.split(","), a.towers.split(",")
    pkg = importlib.import_module("vision-transformer-opencl_amd")
    B = importlib.import_module("vision-transformer-opencl_amd.binding")
    out = open(a.out, "a") if a.out else None
    if "fc1" in a.parts.split(","):
        fc1_part(pkg, B, a, out)
    if "towers" in a.parts.split(","):
        towers_part(pkg, B, a, out)


if __name__ == "__main__":
    main()
