#!/usr/bin/env python3
"""The four encoder GEMMs of the batch-256 ViT-B/16 forward (M = 50,432) with vithip_gemm_args.arith = 0 (fp32 MFMA) and 1 (the
three-piece split on the bf16 pipe), interleaved in one process, HIP events, the engine's call shape (auto tile, workspace lent;
QKV and fc1 as the LayerNorm fold's consumers with the centred weight).  GPU box only.
    python3 tools/gemm_f32_split_time.py [rounds] [--image | --geometry]
One JSON line per GEMM and arithmetic: microseconds per launch (min and median over the rounds) and the speed-up.
--image: the split without the pre-split weight image (arm 1) against the split with it (arm 2, vithip_gemm_args.w_split, what
the engine passes); "speedup" is then over arm 1.
--geometry (probe library: VIT_HIP_LIBRARY=.../libvit_mi355x_probe.so): the image walk forced to 128 x 128 tiles (arm 137) against
64 x 256 tiles (arm 138) through the override codes of vithip_gemm_set_tile; "speedup" is then over the 128 x 128 tiles."""
import ctypes as C, importlib, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B = importlib.import_module("vision-transformer-opencl_amd.binding")
from tools.gemm_probe import timed
args = [a for a in sys.argv[1:] if a not in ("--image", "--geometry")]
rounds = int(args[0]) if args else 5
# 0 fp32 MFMA, 1 split, 2 split with the weight image; 137 / 138: the image walk in 128 x 128 / 64 x 256 tiles
arms = (137, 138) if "--geometry" in sys.argv else (1, 2) if "--image" in sys.argv else (0, 1)
M, D, H = 50432, 768, 3072
rng = np.random.default_rng(0)
f = lambda *shape, a=1.0: B.DeviceArray.from_numpy(rng.uniform(-a, a, shape).astype(np.float32))
L = B.lib()
ws = B.gemm_workspace()
x, h = f(M, D), f(M, H)
rows = B.DeviceArray.from_numpy(np.stack([rng.uniform(0.5, 1.5, M), rng.uniform(-1, 1, M)], 1).astype(np.float32))
for name, N, K, epi, A, fold in (("qkv", 3 * D, D, B.EPI_BIAS, x, True), ("out_proj", D, D, B.EPI_BIAS_RESIDUAL, x, False),
                                 ("fc1", H, D, B.EPI_BIAS_GELU, x, True), ("fc2", D, H, B.EPI_BIAS_RESIDUAL, h, False)):
    W, b, out = f(N, K, a=.03), f(N, a=.1), B.DeviceArray((M, N))
    res = out if epi == B.EPI_BIAS_RESIDUAL else None
    img = B.split3_weights_device(W, N, K) if max(arms) >= 2 else None
    ms = {arm: [] for arm in arms}
    for _ in range(rounds):
        for arm in arms:
            a = B.CGemmArgs(A.ptr, K, W.ptr, K, b.ptr, res.ptr if res else None, N, out.ptr, N, M, N, K, epi, 0, 0, ws, 0,
                            rows.ptr if fold else None, None, None, None, min(arm, 1), img.ptr if arm >= 2 else None)
            if arm > 2:
                B.hip_check(L.vithip_gemm_set_tile(arm), "vithip_gemm_set_tile")
            ms[arm].append(timed(lambda: B.hip_check(L.vithip_gemm_f32(None, C.byref(a)), "gemm"), reps=6, warm=2))
    flops = 2.0 * M * N * K
    for arm in arms:
        t = float(np.median(ms[arm]))
        print(json.dumps({"gemm": name, "arith": min(arm, 1), "w_split": arm >= 2, **({"tile": "128x128" if arm == 137 else "64x256"} if arm > 2 else {}), "us_min": round(min(ms[arm]) * 1e3, 1),
                          "us_median": round(t * 1e3, 1), "tflops": round(flops / (t * 1e-3) / 1e12, 1),
                          "speedup": round(float(np.median(ms[arms[0]])) / t, 3)}), flush=True)
    del W, b, out, img
