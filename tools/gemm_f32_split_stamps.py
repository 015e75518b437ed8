#!/usr/bin/env python3
"""How long a K step of the split GEMMs' image walk waits for its fragments: the stamped instantiation of the persistent walk
(probe library, tile code 129 with arith = 1 and a weight image; per workgroup [start, loop start, SUM of epilogue cycles, end,
SUM of fragment waits, ..., tiles, K-steps]) on the four encoder GEMMs of the metric batch, without helper pieces.  A fragment wait
runs from the top of a step (a segment's first step: from in front of its cold W request) to the point in front of the step's
first matrix instruction where A's fragments have landed from LDS and all W loads but the youngest four in flight (A's two staging
loads and W-mid's two) have landed from the image.  (profiles/r21 holds the figures of the steps that read W's fragments from LDS:
those arms are gone.)  GPU box only, probe library:
    VIT_HIP_LIBRARY=.../libvit_mi355x_probe.so python3 tools/gemm_f32_split_stamps.py"""
import ctypes as C, importlib, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B = importlib.import_module("vision-transformer-opencl_amd.binding")
from tools.gemm_probe import timed
L = B.lib()
M, D, H = 50432, 768, 3072
rng = np.random.default_rng(0)
f = lambda *shape, a=1.0: B.DeviceArray.from_numpy(rng.uniform(-a, a, shape).astype(np.float32))
x, h = f(M, D), f(M, H)
rows = B.DeviceArray.from_numpy(np.stack([rng.uniform(0.5, 1.5, M), rng.uniform(-1, 1, M)], 1).astype(np.float32))
L.vithip_gemm_set_debug_buffer.argtypes = [C.c_void_p]
for name, N, K, epi, A, fold in (("qkv", 3 * D, D, B.EPI_BIAS, x, True), ("out_proj", D, D, B.EPI_BIAS_RESIDUAL, x, False),
                                 ("fc1", H, D, B.EPI_BIAS_GELU, x, True), ("fc2", D, H, B.EPI_BIAS_RESIDUAL, h, False)):
    W, b, out = f(N, K, a=.03), f(N, a=.1), B.DeviceArray((M, N))
    res = out if epi == B.EPI_BIAS_RESIDUAL else None
    img = B.split3_weights_device(W, N, K)
    nwg = ((M + 127) // 128) * ((N + 127) // 128)
    a = B.CGemmArgs(A.ptr, K, W.ptr, K, b.ptr, res.ptr if res else None, N, out.ptr, N, M, N, K, epi, 0, 0, None, 0,
                    rows.ptr if fold else None, None, None, None, 1, img.ptr)
    dbg = B.DeviceArray((nwg, 8), np.uint64)
    L.vithip_gemm_set_debug_buffer(dbg.ptr)
    B.hip_check(L.vithip_gemm_set_tile(129))
    ms = timed(lambda: B.hip_check(L.vithip_gemm_f32(None, C.byref(a)), "gemm"), reps=3, warm=1)
    d = dbg.numpy().astype(np.int64)
    d = d[d[:, 7] > 0]
    tot, epi_c, frag, steps = d[:, 3] - d[:, 0], d[:, 2], d[:, 4], d[:, 7]
    print(json.dumps({"gemm": name, "event_ms": round(ms, 4), "wgs": int(len(d)),
                      "loop_cycles_per_k_step_median": round(float(np.median((d[:, 3] - d[:, 1] - epi_c) / steps)), 1),
                      "fragment_wait_cycles_per_k_step_median": round(float(np.median(frag / steps)), 1),
                      "fragment_wait_share_of_wg_time": round(float(np.median(frag / tot)), 4)}), flush=True)
    L.vithip_gemm_set_debug_buffer(None)
    L.vithip_gemm_set_tile(0)
    dbg.free()
    del W, b, out, img
