#!/usr/bin/env python3
"""Time vithip_attention_f32 (the resident fp32 kernel) and, beside it on the same qkv, vithip_attention_f32_split (the three-piece
split on the bf16 matrix pipe) at the metric shape (256 images x 12 heads x 197 tokens) with HIP events. GPU box only.
    attn_time.py [n] [tokens] [rounds]
The two legs alternate round by round (default 5 rounds of 10 launches each); the line holds every round and the medians.  A library
without the split entry (VIT_HIP_LIBRARY = an earlier build) gets the first leg only.
VIT_TOOL_DATA=zeros: an all-zero qkv (the same instructions at a lower power draw)."""
import importlib, json, os, statistics, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B = importlib.import_module("vision-transformer-opencl_amd.binding")
from tools.gemm_probe import timed
n, T, heads = int(sys.argv[1]) if len(sys.argv) > 1 else 256, int(sys.argv[2]) if len(sys.argv) > 2 else 197, 12
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
D = heads * 64
rng = np.random.default_rng(0)
vals = rng.uniform(-1.5, 1.5, (n * T, 3 * D)).astype(np.float32)
if os.environ.get("VIT_TOOL_DATA") == "zeros":
    vals[:] = 0
dq = B.DeviceArray.from_numpy(vals)
do = B.DeviceArray((n * T, D))
L = B.lib()
legs = {"attention_ms": lambda: B.hip_check(L.vithip_attention_f32(None, dq.ptr, do.ptr, n, T, heads))}
if hasattr(L, "vithip_attention_f32_split"):
    legs["split_ms"] = lambda: B.hip_check(L.vithip_attention_f32_split(None, dq.ptr, do.ptr, n, T, heads, 64, T))
ms = {leg: [] for leg in legs}
for rnd in range(rounds):
    for leg in (list(legs) if rnd % 2 == 0 else list(legs)[::-1]):
        ms[leg].append(timed(legs[leg], reps=10, warm=3))
flop = 2.0 * n * 2 * heads * T * T * 64
rec = {"images": n, "tokens": T}
for leg, v in ms.items():
    rec[leg] = [round(m, 4) for m in v]
    rec[leg.replace("_ms", "_median_ms")] = round(statistics.median(v), 4)
best = min(ms["attention_ms"])
rec.update({"tflops": round(flop / (best * 1e-3) / 1e12, 1), "frac_of_157.3": round(flop / (best * 1e-3) / 1e12 / 157.3, 3)})
if "split_ms" in ms:
    rec["split_over_resident"] = round(statistics.median(ms["split_ms"]) / statistics.median(ms["attention_ms"]), 3)
print(json.dumps(rec))
