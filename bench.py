#!/usr/bin/env python3
"""bench.py -- images/sec of the ViT-B/16 224x224 fp32 forward at batch 256 per GPU (BASELINE.json configs[1]).

    python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]   (N > 1: launched by torch.distributed.run)

A step = one forward of one batch of synthetic images already resident in HBM, through the C-ABI
(vit_engine_forward_device) on this rank's GPU; with N > 1 every rank owns its own batch (weak
scaling, no data-path collective) and the per-image top-1 records are all-gathered over RCCL at
the end of each step (the only exchange the north star asks for).  One JSON line on rank 0.

A plain run sets up, warms up, times the K steps and prints the line (metric, value, unit, ms_per_step, dtype, config);
the objects below are null in it.  --full adds every check and measurement listed below, each outside the timed region.
--dump-outputs DIR writes what the last timed step returned to its caller, as float32 / float64 .npy files (rank 0):
  probs.npy [B][classes], top1_label.npy [B], top1_prob.npy [B], and with N > 1 gathered_top1_label.npy /
  gathered_top1_prob.npy [N][B] (the RCCL gather).  Above 48 MB of probabilities, a fixed seeded sample of rows is written
  instead, its row indices in probs_rows.npy.  Weights and images come from fixed seeds: same arguments, same inputs.

Extra objects in the line (--full):
  roofline      the dominant kernel (fp32 MFMA GEMM): algorithmic FLOPs per launch / average launch
                duration from HIP events recorded on the launch stream during the timed steps.
  golden        every rank's batch starts with the two images of tests/golden/vit_b16_e2e.npz (probabilities written by the
                reference's own ViT_seq(), oracle/gen_golden.py): rows 0-1 of the timed steps' output are checked against them
                on every rank, at any N (1e-4 fp32 / 2e-2 bf16, identical top-1); with N > 1 rank 0 also checks every rank's
                slot of the RCCL gather (against a broadcast of that rank's records and against the golden labels).
                Any failure sets "ok": false and the exit code.
  roofline.clock_limit_probe   N = 1: the dominant GEMM's launch shape timed on random and on all-zero operands (same instructions,
                same traffic): how much of the gap to the roofline is the clock the power limit leaves, measured on this device.
  c_surface     N = 1: the same batch through vit_engine_forward_host -- what ViT_opencl(ImageData*, Network*, float**) does
                underneath (separately allocated host images in, host probability rows out: H2D and D2H inside the time,
                Main.c:55-60 times exactly that call).  Never `value`.
  other_configs N = 1, default configuration only: BASELINE.json configs[2] (ViT-B/16 bf16, batch 2048) and configs[4] (ViT-L/16-384
                bf16, batch 1024) as short timed runs of their own AFTER everything above (1 warm-up + 3 timed forwards each, batch
                resident in HBM, the two golden images of the model open the batch: tests/golden/vit_b16_e2e.npz /
                vit_l16_384_e2e.npz): value, ms_per_step, dominant kernel's roofline fraction, golden block.  Never `value`.
  cpu_baseline  the reference's own ViT_seq() (oracle/_ref, compiled from its ViT_seq.c) when that library is
                present, else the CPU oracle (bit-identical restatement), timed on one host core on one
                image of the same batch; the GPU row for that image is checked against it (1e-4 on
                probabilities, same top-1); all_cores = one single-threaded forward per core.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

METRIC = "images/sec ViT-B/16 224² fp32 @batch256; % MFMA roofline; top-1 match"
FP32_MFMA_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: 256 CU x 4 SIMD x 64 flop/clk x 2.4 GHz
BF16_MFMA_PEAK_TFLOPS = 2516.6  # dense bf16 MFMA (16x the fp32 matrix rate), no sparsity
STAGE_KERNEL = {  # engine stage -> kernel instantiation that runs it at the metric configuration (fp32, batch 256, one lane)
    "qkv": "gemm_f32_nt_persistent_kernel<EPI_BIAS>", "head": "gemm_f32_nt_latency_kernel",
    "fc1": "gemm_f32_nt_persistent_kernel<EPI_BIAS_GELU>",
    "outproj": "gemm_f32_nt_persistent_kernel<EPI_BIAS_RESIDUAL>", "fc2": "gemm_f32_nt_persistent_kernel<EPI_BIAS_RESIDUAL>",
    "attn": "attention_f32_resident_kernel", "ln": "layernorm_f32_kernel", "embed": "gemm_f32_nt_kernel<A_PATCHES>",
    "softmax": "softmax_top1_f32_kernel",
}
# ... and with the LayerNorm fold (fp32 default): the consumer / producer instantiations of the same walk, and
# what is left of the LayerNorm stage (layer 0's statistics pass + the head's LayerNorm; the finalise launches are inside the
# residual GEMMs' brackets)
STAGE_KERNEL_FOLD = dict(STAGE_KERNEL, qkv="gemm_f32_nt_persistent_kernel<EPI_BIAS_LN>", fc1="gemm_f32_nt_persistent_kernel<EPI_BIAS_GELU_LN>",
                         outproj="gemm_f32_nt_persistent_kernel<EPI_RESIDUAL_STATS>", fc2="gemm_f32_nt_persistent_kernel<EPI_RESIDUAL_STATS>",
                         ln="rowstats_f32_kernel")


WEIGHT_SEED = 1234      # synthetic weights of every configuration (the golden fixtures were written with it)
GOLDEN_FILE = {"b16": "vit_b16_e2e.npz", "l16_384": "vit_l16_384_e2e.npz"}   # tests/golden/: oracle/gen_golden.py, gen_golden_vit_l.py


def load_golden(np, model, weight_seed):
    """(probabilities [2][classes], image seed) of the two golden images of `model`, or (None, None)."""
    try:
        g = np.load(os.path.join(ROOT, "tests", "golden", GOLDEN_FILE[model]))
    except (OSError, KeyError):
        return None, None
    if int(g["weight_seed"]) != weight_seed:
        return None, None
    return g["probs"].astype(np.float32), int(g["image_seed"])


PROFILE_ROUND = "r05"   # profiles/<round>/: the committed rocprofv3 passes the replayed counter fields come from


def profile_tag(dtype, model):
    """Suffix of the committed profile files for a bench configuration: f32 | bf16 | bf16_l16_384 (configs[1], [2], [4])."""
    return dtype if model == "b16" else f"{dtype}_{model}"


PROFILED_BATCH = {"f32": 256, "bf16": 2048, "bf16_l16_384": 1024}   # the batch each set of passes was collected at


def pmc_traffic(kernel, tag, batch):
    """(HBM bytes per launch of `kernel`, provenance) from the committed PMC passes (profiles/<round>/README.md: separate
    rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE runs of this same command, summarised by tools/pmc_summary.py).
    NOT collected live -- counters need the profiler -- so the value is a replay and says so (roofline.replayed_from).
    (None, None) when the passes do not cover this configuration."""
    rel = os.path.join("profiles", PROFILE_ROUND, f"hbm_traffic_pmc_{tag}.json")
    try:
        with open(os.path.join(ROOT, rel)) as f:
            rec = json.load(f)
    except OSError:
        return None, None
    if rec.get("batch") != batch or kernel not in rec.get("kernels", {}):
        return None, None
    return rec["kernels"][kernel], {"path": rel, "device": rec.get("device"), "commit": rec.get("commit"),
                                    "collected": rec.get("collected")}


def quiet_stdout(fn):
    """Run fn() with file descriptor 1 pointed at /dev/null (C code that printf()s), flushing C stdio before restoring."""
    import ctypes
    sys.stdout.flush()
    saved, devnull = os.dup(1), os.open(os.devnull, os.O_WRONLY)
    os.dup2(devnull, 1)
    try:
        return fn()
    finally:
        ctypes.CDLL(None).fflush(None)
        os.dup2(saved, 1)
        os.close(saved)
        os.close(devnull)


def pmc_mfma(kernel, tag, batch):
    """(MFMA-busy %, clock GHz) of `kernel` from the committed rocprofv3 PMC pass (profiles/<round>/mfma_util_<tag>.csv,
    tools/collect_profiles.sh); (None, None) when that pass does not cover this configuration."""
    import csv
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from pmc_summary import bench_key
        with open(os.path.join(ROOT, "profiles", PROFILE_ROUND, f"mfma_util_{tag}.csv"), newline="") as f:
            rows = [r for r in csv.DictReader(f) if bench_key(r["kernel"]) == kernel]
    except (OSError, ImportError):
        return None, None
    if not rows or batch != PROFILED_BATCH.get(tag):
        return None, None
    r = max(rows, key=lambda r: float(r["avg_us"]) * int(r["launches"]))
    return float(r["mfma_busy_percent"]), float(r["clock_ghz_from_gui_active"])


def replayed_counters(kernel, tag, batch):
    """Counter-derived fields of a roofline object for `kernel` (HBM bytes per launch, MFMA-busy %, clock) from the committed
    rocprofv3 passes of profiles/<round>/, with their provenance: they cannot be read without the profiler, so they are REPLAYED
    from another run of the same command (possibly another device of the pool) and marked `live: false`; everything else in
    the object they join is measured live in the process that prints it."""
    traffic, traffic_src = pmc_traffic(kernel, tag, batch)
    busy, clock = pmc_mfma(kernel, tag, batch)
    replayed = None
    if traffic_src or busy is not None:
        replayed = dict(traffic_src or {"path": os.path.join("profiles", PROFILE_ROUND, f"mfma_util_{tag}.csv")},
                        fields=[k for k, v in (("traffic", traffic), ("mfma_busy_percent_rocprof", busy),
                                               ("clock_ghz_rocprof", clock)) if v is not None],
                        live=False)
    return {"traffic": traffic, "mfma_busy_percent_rocprof": busy, "clock_ghz_rocprof": clock, "replayed_from": replayed}


DUMP_PROBS_BYTES = 48 << 20   # --dump-outputs: probability rows beyond this are sampled (the whole dump stays under 64 MB)


def dump_outputs(np, out_dir, probs, top1, gathered):
    """What the last timed step handed its caller, as .npy files in out_dir: float32 probabilities and top-1 probabilities,
    float64 labels (exact), and the gathered records of every rank when there are several."""
    os.makedirs(out_dir, exist_ok=True)
    p = probs.cpu().numpy()
    if p.nbytes > DUMP_PROBS_BYTES:
        n = DUMP_PROBS_BYTES // (p.shape[1] * p.itemsize)
        rows = np.sort(np.random.default_rng(0).choice(p.shape[0], n, replace=False))
        p = p[rows]
        np.save(os.path.join(out_dir, "probs_rows.npy"), rows.astype(np.float64))
    out = {"probs": p}
    rec = top1.cpu()
    out["top1_label"] = rec[0].numpy().astype(np.float64)
    out["top1_prob"] = rec[1].numpy().view(np.float32)
    if gathered is not None:
        g = gathered.cpu().numpy()
        out["gathered_top1_label"] = g[:, 0].astype(np.float64)
        out["gathered_top1_prob"] = np.ascontiguousarray(g[:, 1]).view(np.float32)
    for name, a in out.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def clock_limit_probe(binding, torch, dev, cfg, batch, dtype):
    """The same GEMM launch (the dominant kernel's shape, product library, default stream) on random and on all-zero operands:
    identical instructions and memory traffic, different bit activity.  The chip runs these kernels at the clock its power limit
    leaves, so the second figure is what the schedule delivers when the clock is not what gives."""
    import ctypes as C
    L = binding.lib()
    M = batch * cfg.tokens
    D, H = cfg.embed_dim, cfg.hidden_dim

    def timed(fn, reps=4, warm=2):
        e0, e1 = C.c_void_p(), C.c_void_p()
        L.vithip_event_create(C.byref(e0)); L.vithip_event_create(C.byref(e1))
        for _ in range(warm):
            fn()
        L.vithip_event_record(e0, None)
        for _ in range(reps):
            fn()
        L.vithip_event_record(e1, None)
        L.vithip_event_sync(e1)
        ms = C.c_float()
        L.vithip_event_elapsed_ms(C.byref(ms), e0, e1)
        return ms.value / reps

    torch.cuda.synchronize(dev)
    g = torch.Generator(device=dev).manual_seed(7)
    out = {}
    if dtype == "f32":      # fc2: [M, H] x [D, H]^T + bias + residual, helper pieces on (what the engine launches)
        N, K, kernel = D, H, "gemm_f32_nt_persistent_kernel<EPI_BIAS_RESIDUAL>"
        ws = binding.gemm_workspace()
        bias = torch.zeros(N, device=dev)
        Cbuf = torch.empty((M, N), device=dev)
        for name in ("random", "zero"):
            A = (torch.rand((M, K), device=dev, generator=g) * 2 - 1) if name == "random" else torch.zeros((M, K), device=dev)
            W = (torch.rand((N, K), device=dev, generator=g) * 0.1 - 0.05) if name == "random" else torch.zeros((N, K), device=dev)
            R = (torch.rand((M, N), device=dev, generator=g) * 2 - 1) if name == "random" else torch.zeros((M, N), device=dev)
            torch.cuda.synchronize(dev)
            ga = binding.CGemmArgs(A.data_ptr(), K, W.data_ptr(), K, bias.data_ptr(), R.data_ptr(), N, Cbuf.data_ptr(), N, M, N, K,
                                   binding.EPI_BIAS_RESIDUAL, 0, 0, ws, 0)
            ms = min(timed(lambda: binding.hip_check(L.vithip_gemm_f32(None, C.byref(ga)))) for _ in range(2))
            out[name] = 2.0 * M * N * K / (ms * 1e-3) / 1e12
            del A, W, R
        L.vithip_gemm_f32_workspace_destroy.argtypes = [C.c_void_p]
        L.vithip_gemm_f32_workspace_destroy(ws)
    else:                   # QKV: [M, D] x [3D, D]^T + bias -> bf16 (the plain form: no LayerNorm-fold operands)
        N, K, kernel = 3 * D, D, "gemm_bf16_pp_kernel<BF16>"
        L.vithip_gemm_bf16.argtypes = [C.c_void_p, C.POINTER(binding.CGemmBf16Args)]
        bias = torch.zeros(N, device=dev)
        Cbuf = torch.empty((M, N), device=dev, dtype=torch.bfloat16)
        for name in ("random", "zero"):
            A = torch.randn((M, K), device=dev, generator=g).to(torch.bfloat16) if name == "random" else torch.zeros((M, K), device=dev, dtype=torch.bfloat16)
            W = (torch.randn((N, K), device=dev, generator=g) * 0.03).to(torch.bfloat16) if name == "random" else torch.zeros((N, K), device=dev, dtype=torch.bfloat16)
            torch.cuda.synchronize(dev)
            ga = binding.CGemmBf16Args(A.data_ptr(), K, W.data_ptr(), K, bias.data_ptr(), None, N, Cbuf.data_ptr(), N, M, N, K, 0, 0,
                                       None, None, None, 0, None)
            ms = min(timed(lambda: binding.hip_check(L.vithip_gemm_bf16(None, C.byref(ga)))) for _ in range(2))
            out[name] = 2.0 * M * N * K / (ms * 1e-3) / 1e12
            del A, W
    return {"kernel": kernel, "shape_mnk": [M, N, K], "random_operands_tflops": round(out["random"], 1),
            "zero_operands_tflops": round(out["zero"], 1), "zero_over_random": round(out["zero"] / out["random"], 4),
            "note": "one launch shape of the product library timed on both operand sets (HIP events, default stream): same instructions "
                    "and traffic, the difference is clock the power limit takes back on busy operands"}


def stage_macs(cfg, batch):
    T, D, H = cfg.tokens, cfg.embed_dim, cfg.hidden_dim
    M = batch * T
    hd = D // cfg.num_heads
    return {  # algorithmic MACs of ONE launch of each stage (SURVEY.md 8d breakdown x batch)
        "embed": batch * cfg.patches * cfg.patch_dim * D,
        "qkv": M * D * 3 * D, "attn": batch * 2 * cfg.num_heads * T * T * hd, "outproj": M * D * D,
        "fc1": M * D * H, "fc2": M * D * H, "head": batch * D * cfg.num_classes, "ln": 0, "softmax": 0,
    }


def dominant_kernel(times, cfg, B, dtype, kernel_steps, saved=None, fold=False):
    """Per-kernel launch time and algorithmic FLOPs from the engine's stage brackets (one lane, every launch alone on the
    GPU) -> (name, record, average launch ms, achieved TFLOP/s) of the kernel with the most time, + all-GEMM ms and FLOPs."""
    saved = saved or {}
    macs = stage_macs(cfg, B)
    per_kernel = {}
    for stage, rec in times["stages"].items():
        k = (STAGE_KERNEL_FOLD if fold and dtype != "bf16" else STAGE_KERNEL)[stage]
        if dtype == "bf16" and stage == "embed":
            k = "gemm_bf16_pp_kernel<F32_EMBED>"
        if dtype == "bf16" and stage == "attn":
            k = "attention_bf16_kernel" if cfg.tokens <= 224 else "attention_bf16_stream_kernel"
        if dtype == "bf16" and stage in ("qkv", "outproj", "fc1", "fc2"):
            k = "gemm_bf16_pp_kernel<%s>" % {"qkv": "BF16", "fc1": "BF16_GELU", "outproj": "F32_RESIDUAL", "fc2": "F32_RESIDUAL"}[stage]
        d = per_kernel.setdefault(k, {"ms": 0.0, "launches": 0, "flop": 0.0})
        d["ms"] += rec["ms"]
        d["launches"] += rec["launches"]
        # per step: depth launches of the full size, minus what a pruned last layer skips (its extra small launches
        # are in rec["launches"] and rec["ms"]; the flops below are the executed ones either way)
        per_step = {"embed": 1, "head": 1}.get(stage, cfg.depth if stage in macs and macs[stage] else 0)
        d["flop"] += 2.0 * (macs[stage] * per_step - B * saved.get(stage, 0)) * kernel_steps
    dom_name, dom = max(per_kernel.items(), key=lambda kv: kv[1]["ms"])
    avg_ms = dom["ms"] / max(dom["launches"], 1)
    achieved = dom["flop"] / max(dom["launches"], 1) / (avg_ms * 1e-3) / 1e12 if avg_ms > 0 else 0.0
    gemm_ms = sum(v["ms"] for k, v in per_kernel.items() if k.startswith("gemm"))
    gemm_flop = sum(v["flop"] for k, v in per_kernel.items() if k.startswith("gemm"))
    return dom_name, dom, avg_ms, achieved, gemm_ms, gemm_flop


def workload_name(model, dtype, batch, config):
    return (f"{'ViT-B/16 224x224' if model == 'b16' else 'ViT-L/16 384x384'} {'fp32' if dtype == 'f32' else 'bf16-MFMA'} forward, "
            f"batch {batch} per GPU, synthetic weights and images (BASELINE.json configs[{config}])")


def other_config(pkg, binding, torch, np, dev, device_index, config, weights=None, steps=3, warmup=1):
    """BASELINE.json configs[2] / configs[4] as a short timed run of their own in the process that has just measured the headline
    (outside its timed region, rank 0 of an N = 1 run only): same protocol -- batch resident in HBM, the two golden images open
    the batch, `warmup` untimed and `steps` timed forwards bracketed by synchronisation, then a one-lane pass with every launch
    bracketed for the dominant kernel's rate -- so that the driver-run line carries these configurations too.  Never `value`."""
    model, dtype, B, lanes = {2: ("b16", "bf16", 2048, 2), 4: ("l16_384", "bf16", 1024, 2)}[config]
    cfg = pkg.VIT_B16 if model == "b16" else pkg.VIT_L16_384
    t_setup = time.perf_counter()
    if weights is None:
        weights = pkg.synth.make_weights(cfg, WEIGHT_SEED)
    eng = binding.Engine(cfg, max_batch=B, device=device_index, profile=False, lanes=lanes, dtype=dtype)
    eng.load_weights(weights)
    del weights
    n_distinct = 8
    host_imgs = pkg.synth.make_images(cfg, n_distinct, seed=99)
    golden, image_seed = load_golden(np, model, WEIGHT_SEED)
    if golden is not None:
        host_imgs[:2] = pkg.synth.make_images(cfg, 2, seed=image_seed)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        base = torch.from_numpy(host_imgs).to(dev)
        images = base.repeat((B + n_distinct - 1) // n_distinct, 1, 1, 1)[:B].contiguous()
        off = torch.arange(B, device=dev, dtype=torch.float32)
        off[:n_distinct] = 0.0
        images += 1e-3 * off.view(B, 1, 1, 1)
        probs = torch.empty((B, cfg.num_classes), device=dev, dtype=torch.float32)
        top1 = torch.empty((2, B), device=dev, dtype=torch.int32)
    stream.synchronize()

    def step():
        eng.forward_device(images.data_ptr(), B, probs.data_ptr(), top1[0].data_ptr(), top1[1].data_ptr(), stream.cuda_stream)

    def fence():
        stream.synchronize()
        torch.cuda.synchronize(dev)

    for _ in range(warmup):
        step()
    fence()
    setup_s = time.perf_counter() - t_setup
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    fence()
    dt = time.perf_counter() - t0
    tol = 2e-2
    gold = None
    if golden is not None:
        got2 = probs[:2].cpu().numpy()
        gold = {"rows": 2, "max_abs_prob_err": float(np.abs(got2 - golden).max()),
                "top1_match": bool((got2.argmax(1) == golden.argmax(1)).all()), "tolerance": tol,
                "fixture": "tests/golden/" + GOLDEN_FILE[model]}
    eng.set_lanes(1)
    eng.set_profile(True)
    step()
    fence()
    eng.reset_stage_times()
    step()
    fence()
    times = eng.stage_times()
    eng.close()
    dom_name, dom, avg_ms, achieved, gemm_ms, gemm_flop = dominant_kernel(times, cfg, B, dtype, 1)
    value = B * steps / dt
    tflops = value * 2.0 * cfg.macs_per_image / 1e12
    return {"workload": workload_name(model, dtype, B, config), "dtype": dtype, "value": round(value, 2), "unit": "images/sec",
            "ms_per_step": round(1e3 * dt / steps, 3), "steps": steps, "warmup": warmup, "lanes_per_gpu": lanes,
            "setup_seconds": round(setup_s, 2),
            "roofline": {"bound": "mfma", "kernel": dom_name, "achieved": round(achieved, 2), "peak": BF16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                         "frac": round(achieved / BF16_MFMA_PEAK_TFLOPS, 4), **replayed_counters(dom_name, profile_tag(dtype, model), B),
                         "avg_launch_ms": round(avg_ms, 4),
                         "all_gemm_tflops": round(gemm_flop / (gemm_ms * 1e-3) / 1e12, 2) if gemm_ms > 0 else None,
                         "whole_model_tflops": round(tflops, 2), "whole_model_frac": round(tflops / BF16_MFMA_PEAK_TFLOPS, 4),
                         "stage_ms_per_step": {s_: round(r["ms"], 3) for s_, r in times["stages"].items()}},
            "golden": gold,
            "ok": gold is None or (gold["top1_match"] and gold["max_abs_prob_err"] <= tol)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256, help="images per GPU per step (metric config: 256)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-threads", type=int, default=1)
    ap.add_argument("--no-cpu-all-cores", action="store_true", help="skip the one-forward-per-core aggregate CPU figure")
    ap.add_argument("--cpu-all-cores", type=int, default=16,
                    help="cap on concurrent single-threaded CPU forwards for cpu_baseline.all_cores (a 1-GPU box's CPU share is 16)")
    ap.add_argument("--lanes", type=int, default=0,
                    help="concurrent sub-batches per step (engine option; 1 = every kernel alone on the GPU).  Default: 1 for fp32 "
                         "(its GEMMs balance their own tails and assume their workgroups resident), 2 for bf16 (the HBM-bound "
                         "LayerNorm / residual kernels of one lane overlap the other's GEMMs: +6 %%)")
    ap.add_argument("--kernel-steps", type=int, default=3,
                    help="extra steps with lanes=1 and per-launch event brackets for the roofline object (when lanes > 1)")
    ap.add_argument("--model", choices=("b16", "l16_384"), default="b16",
                    help="b16 = ViT-B/16 224 (the metric); l16_384 = ViT-L/16 384 (BASELINE.json configs[4], use --dtype bf16 --batch 1024)")
    ap.add_argument("--dtype", choices=("f32", "bf16"), default="f32",
                    help="f32 = the metric configuration (BASELINE.json configs[1]); bf16 = configs[2] (use --batch 2048)")
    ap.add_argument("--prune-last-layer", action="store_true",
                    help="NOT the metric configuration: vit_engine_options.prune_last_layer (the last encoder layer computes "
                         "only the class rows; bit-identical probabilities, 7 %% less arithmetic).  FLOP figures then count "
                         "the executed work")
    ap.add_argument("--stage-brackets", dest="no_stage_brackets", action="store_false",
                    help="with --lanes 1: record the per-launch event brackets INSIDE the timed steps (they cost ~0.5 ms per "
                         "forward at batch 1, 1-3 %% at batch 256); default: the timed steps carry no instrumentation and the "
                         "roofline pass (same batch, same kernels, every launch bracketed) runs right after them")
    ap.add_argument("--no-stage-brackets", dest="no_stage_brackets", action="store_true", help=argparse.SUPPRESS)
    ap.set_defaults(no_stage_brackets=True)
    ap.add_argument("--graph", action="store_true",
                    help="vit_engine_options.use_graph: replay the forward as one hipGraph (needs --lanes 1; small batches)")
    ap.add_argument("--ln-fold", type=int, default=0, choices=(-1, 0, 1),
                    help="fold the encoder LayerNorms into the GEMMs either side (0 auto = on, -1 off: a LayerNorm kernel each, the reference's operation order)")
    ap.add_argument("--gemm-tile", type=int, default=0, help="tuning: vithip_gemm_args.tile of every fp32 GEMM (0 auto; 6..12, include/vit_hip_kernels.h)")
    ap.add_argument("--config", type=int, default=0, choices=(0, 1, 2, 3, 4),
                    help="BASELINE.json configs[i] preset: 1 = fp32 batch 256 (the metric, the default), 2 = bf16 batch 2048, "
                         "3 = bf16 2048 per GPU (global 16384 at --gpus 8), 4 = ViT-L/16-384 bf16 batch 1024")
    ap.add_argument("--no-c-surface", action="store_true", help="skip the host-pointer (ViT_opencl-shaped) timing after the timed region")
    ap.add_argument("--no-clock-probe", action="store_true",
                    help="skip roofline.clock_limit_probe (the dominant GEMM shape once on random and once on all-zero operands)")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="skip other_configs (short timed runs of BASELINE.json configs[2] and [4] after the headline's timed region; "
                         "only the default N = 1 configs[1] run does them)")
    ap.add_argument("--spawn", action="store_true",
                    help="start the rank processes from this process even for --gpus 1 (N > 1 always does when not "
                         "already launched): exercises the launcher and the RCCL gather at world size 1")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beyond the headline figure: golden / parity / gather checks, roofline pass, CPU baseline, "
                         "C surface, clock probe and the other configurations (the --no-* switches above select among them)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write what the last timed step computed (probabilities, top-1 records) as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if args.config:
        args.model, args.dtype, args.batch = {1: ("b16", "f32", 256), 2: ("b16", "bf16", 2048), 3: ("b16", "bf16", 2048),
                                              4: ("l16_384", "bf16", 1024)}[args.config]
    if args.lanes <= 0:
        args.lanes = 1 if args.dtype == "f32" else 2

    # ---- one process per GPU -------------------------------------------------------------------------
    # `python bench.py --gpus N` started plainly: THIS process only spawns the N ranks (fresh interpreters, before
    # anything here has imported torch or loaded the HIP library) and relays rank 0's JSON line.  Started by
    # torch.distributed.run (WORLD_SIZE set) it is a rank already.  N = 1 without --spawn stays in-process, so
    # `rocprofv3 -- python3 bench.py` profiles the process it launched.
    pkg = importlib.import_module("vision-transformer-opencl_amd")
    launch = pkg.launch
    if not launch.launched() and args.gpus > 1:
        # fail fast, before any rank exists; the count is taken in a child interpreter (this parent imports neither torch nor HIP)
        have = launch.visible_gpus()
        if 0 <= have < args.gpus:
            sys.exit(f"bench.py: --gpus {args.gpus} needs {args.gpus} GPUs on this node, it shows {have} (one rank per GPU; "
                     f"nothing was started)")
    if not launch.launched() and (args.gpus > 1 or args.spawn):
        rc, _ = launch.launch_ranks(os.path.abspath(__file__), [a for a in sys.argv[1:] if a != "--spawn"], args.gpus)
        sys.exit(rc)

    import numpy as np
    import torch
    import torch.distributed as dist

    binding = importlib.import_module("vision-transformer-opencl_amd.binding")
    synth = pkg.synth
    cfg = pkg.VIT_B16 if args.model == "b16" else pkg.VIT_L16_384

    rank, local_rank, world = launch.rank_env()
    distributed = launch.launched()   # a launched rank takes the RCCL path even at world size 1
    if world != args.gpus:
        if rank == 0:
            print(f"bench.py: --gpus {args.gpus} but WORLD_SIZE={world}", file=sys.stderr)
        sys.exit(2)
    if not torch.cuda.is_available():
        sys.exit("bench.py needs a GPU: the HIP path has no CPU fallback")
    if torch.cuda.device_count() < world or local_rank >= torch.cuda.device_count():
        # every rank leaves (nobody waits in a rendezvous for a rank that cannot exist); rank 0 says why
        if rank == 0:
            print(f"bench.py: --gpus {world} needs {world} GPUs on this node, it shows {torch.cuda.device_count()} (one rank per GPU)",
                  file=sys.stderr)
        sys.exit(2)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if distributed:
        launch.init_process_group("nccl", dev)

    B = args.batch
    weights = synth.make_weights(cfg, WEIGHT_SEED)
    # per-launch HIP-event brackets are on during the timed steps when every kernel runs alone (lanes = 1);
    # with concurrent lanes they would time overlapping kernels, so the roofline pass runs after (below)
    eng = binding.Engine(cfg, max_batch=B, device=local_rank, profile=(args.lanes == 1 and not args.graph and not args.no_stage_brackets), lanes=args.lanes,
                         dtype=args.dtype, prune_last_layer=args.prune_last_layer, use_graph=args.graph, gemm_tile=args.gemm_tile, ln_fold=args.ln_fold)
    eng.load_weights(weights)

    # synthetic batch, generated on the host with the repo PRNG for the first images (so that the
    # CPU baseline sees the same bytes) and tiled on the device; resident in HBM before timing.
    n_distinct = min(B, 8)
    host_imgs = synth.make_images(cfg, n_distinct, seed=99 + 1000 * rank)
    golden = None
    if B >= 2:
        # images 0 and 1 of EVERY rank's batch are the two golden images (generated from the seed the fixture records; the
        # fixture holds what the reference's own ViT_seq() made of them with the seed-1234 weights used above -- for ViT-L/16-384,
        # which the reference's macros cannot express, what the parametrised oracle pinned to it at B/16 made of them)
        golden, golden_image_seed = load_golden(np, args.model, WEIGHT_SEED)
        if golden is not None:
            host_imgs[:2] = synth.make_images(cfg, 2, seed=golden_image_seed)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        base = torch.from_numpy(host_imgs).to(dev)
        reps = (B + n_distinct - 1) // n_distinct
        images = base.repeat(reps, 1, 1, 1)[:B].contiguous()
        # decorrelate the copies a little so the batch is not B/8 identical groups
        off = torch.arange(B, device=dev, dtype=torch.float32)
        off[:n_distinct] = 0.0
        images += 1e-3 * off.view(B, 1, 1, 1)
        probs = torch.empty((B, cfg.num_classes), device=dev, dtype=torch.float32)
        top1 = torch.empty((2, B), device=dev, dtype=torch.int32)  # row 0 labels, row 1 prob bits
        gathered = torch.empty((world, 2, B), device=dev, dtype=torch.int32) if distributed else None
    stream.synchronize()
    sptr = stream.cuda_stream

    def step():
        eng.forward_device(images.data_ptr(), B, probs.data_ptr(), top1[0].data_ptr(), top1[1].data_ptr(), sptr)
        if distributed:  # the one exchange of the path: everybody receives every image's (label, prob)
            with torch.cuda.stream(stream):
                pkg.dp.gather_packed(top1, gathered)

    def fence():
        stream.synchronize()
        torch.cuda.synchronize(dev)
        if distributed:
            dist.barrier()
        torch.cuda.synchronize(dev)

    for _ in range(args.warmup):
        step()
    fence()
    eng.reset_stage_times()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    fence()
    dt = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(np, args.dump_outputs, probs, top1, gathered)
    gather_ok = None
    per_rank_ms = None
    tol = 1e-4 if args.dtype == "f32" else 2e-2
    gold = None
    if args.full and golden is not None:  # rows 0-1 of the timed steps' output against the reference's probabilities, on this rank
        got2 = probs[:2].cpu().numpy()
        gold = {"rows": 2, "max_abs_prob_err": float(np.abs(got2 - golden).max()),
                "top1_match": bool((got2.argmax(1) == golden.argmax(1)).all()), "tolerance": tol,
                "fixture": "tests/golden/" + GOLDEN_FILE[args.model], "ranks": 1}
    if distributed:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        every = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(every, t)                      # each rank's own time: devices of one node differ by a few per cent in the
        per_rank_ms = [round(1e3 * float(x.item()) / args.steps, 3) for x in every]   # clock they hold, and the slowest one is `value`
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    if distributed and args.full:
        # the gather, checked outside the timed region: EVERY slot r must hold what rank r says its records are (a broadcast
        # per rank: another collective than the one under test), and -- the batches start with the golden images -- the
        # golden labels in its first two entries
        gather_ok = pkg.dp.verify_gather(top1, gathered, golden.argmax(1).tolist() if golden is not None else None)
        flags = torch.tensor([-gold["max_abs_prob_err"] if gold else 0.0,
                              1.0 if (gold is None or gold["top1_match"]) else 0.0], device=dev, dtype=torch.float64)
        dist.all_reduce(flags, op=dist.ReduceOp.MIN)   # the worst of all ranks
        if gold:
            gold.update(max_abs_prob_err=float(-flags[0].item()), top1_match=bool(flags[1].item() == 1.0), ranks=world)

    ms_per_step = 1e3 * dt / args.steps
    value = world * B * args.steps / dt
    T_, D_, H_, hd_ = cfg.tokens, cfg.embed_dim, cfg.hidden_dim, cfg.embed_dim // cfg.num_heads
    # MACs per image the pruned last layer does not execute, by stage (vit_config_macs_per_image_pruned)
    saved = ({"qkv": (T_ - 1) * D_ * D_, "attn": (T_ - 1) * 2 * cfg.num_heads * T_ * hd_, "outproj": (T_ - 1) * D_ * D_,
              "fc1": (T_ - 1) * D_ * H_, "fc2": (T_ - 1) * D_ * H_} if args.prune_last_layer else {})
    gflop_img = 2.0 * (cfg.macs_per_image - sum(saved.values())) / 1e9
    model_tflops = value * gflop_img / 1e3 / world  # per GPU

    # ---- roofline of the dominant kernel (per-launch, from the stage brackets) -------------------
    roofline = None
    if args.full:
        handover = eng.handover_stats() if args.dtype == "f32" else None   # fp32 GEMM helper pieces of warm-up + timed steps
        kernel_steps = args.steps
        if args.lanes == 1 and not args.graph and not args.no_stage_brackets:
            times = eng.stage_times()
        else:
            # kernel-level pass: same batch, same kernels, one lane, every launch bracketed by events on its stream
            eng.set_lanes(1)
            eng.set_profile(True)
            step()
            fence()
            eng.reset_stage_times()
            kernel_steps = max(1, args.kernel_steps)
            for _ in range(kernel_steps):
                step()
            fence()
            times = eng.stage_times()
        peak = FP32_MFMA_PEAK_TFLOPS if args.dtype == "f32" else BF16_MFMA_PEAK_TFLOPS
        dom_name, dom, avg_ms, achieved, gemm_ms, gemm_flop = dominant_kernel(times, cfg, B, args.dtype, kernel_steps, saved, fold=args.ln_fold >= 0 and cfg.embed_dim % 64 == 0)
        tag = profile_tag(args.dtype, args.model)
        counters = replayed_counters(dom_name, tag, B)
        roofline = {
            "bound": "mfma", "kernel": dom_name, "achieved": round(achieved, 2), "peak": peak,
            "unit": "TFLOP/s", "frac": round(achieved / peak, 4), **counters,
            "avg_launch_ms": round(avg_ms, 4), "launches": dom["launches"],
            "flop_per_launch": dom["flop"] / max(dom["launches"], 1),
            "all_gemm_tflops": round(gemm_flop / (gemm_ms * 1e-3) / 1e12, 2) if gemm_ms > 0 else None,
            "whole_model_tflops": round(model_tflops, 2),
            "whole_model_frac": round(model_tflops / peak, 4),
            "stage_ms_per_step": {s: round(r["ms"] / kernel_steps, 3) for s, r in times["stages"].items()},
            # fp32 GEMM helper pieces over warm-up + timed steps: tiles finished from a parked piece / tiles whose owner found none
            # and computed all of it (lost time, never a wrong result: nothing in the hand-over waits)
            "gemm_handover": handover,
            "measured": ("HIP events around every launch during the timed steps" if (args.lanes == 1 and not args.graph and not args.no_stage_brackets) else
                         f"HIP events around every launch in {kernel_steps} extra steps with lanes=1 right after the timed region "
                         + (f"(the timed steps run {args.lanes} concurrent lanes, whose kernels overlap)" if args.lanes > 1 else
                            "(same batch, same kernels; the timed steps themselves carry no instrumentation)")),
        }

    # ---- CPU baseline + parity on the sampled image (rank 0, N = 1 only) -------------------------
    cpu = None
    parity = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        from oracle import pyoracle as po
        ocfg = po.Config(cfg.img_size, cfg.patch_size, cfg.in_chans, cfg.num_classes, cfg.embed_dim,
                         cfg.depth, cfg.num_heads, cfg.hidden_dim)
        po.set_threads(args.cpu_threads)
        t1 = time.perf_counter()
        ref_p, _, _ = po.forward_image(ocfg, host_imgs[0], weights)
        cpu_dt = time.perf_counter() - t1
        got = probs[0].cpu().numpy()
        err = float(np.abs(got - ref_p).max())
        parity = {"max_abs_prob_err": err, "top1_match": bool(int(got.argmax()) == int(ref_p.argmax())),
                  "tolerance": 1e-4 if args.dtype == "f32" else 2e-2}
        cpu = {"value": round(1.0 / cpu_dt, 5), "unit": "images/sec", "cores": args.cpu_threads, "kind": "port",
               "sample": f"image 0 of the batch (1 of {B}), {cpu_dt:.2f} s, oracle/vit_cpu_ref.c gcc -O2 -ffp-contract=off"}
        if args.model == "b16" and os.path.exists(po.REF_PATH):
            # the reference's own ViT_seq() (oracle/_ref, compiled from /root/reference/ViT_seq.c by oracle/Makefile in
            # the build container; the .so travels, the sources do not) on the same image: it becomes the baseline
            # ("reference"), the port's time stays beside it, and the GPU row is checked against it as well
            def run_ref():
                t = time.perf_counter()
                out = po.Reference().vit_seq([host_imgs[0]], weights)
                return out, time.perf_counter() - t
            ref_probs, ref_dt = quiet_stdout(run_ref)   # ViT_seq printf()s its own timing: keep stdout to one JSON line
            cpu = {"value": round(1.0 / ref_dt, 5), "unit": "images/sec", "cores": 1, "kind": "reference",
                   "sample": f"image 0 of the batch (1 of {B}), {ref_dt:.2f} s in the reference's ViT_seq() (ViT_seq.c gcc -O2 "
                             "-ffp-contract=off, oracle/_ref/libvitseq_ref.so)",
                   "port": {"value": round(1.0 / cpu_dt, 5), "seconds": round(cpu_dt, 2), "bit_identical_to_reference":
                            bool(np.array_equal(ref_probs[0], ref_p))}}
            parity["max_abs_prob_err_vs_reference"] = float(np.abs(got - ref_probs[0]).max())
        if args.cpu_threads == 1 and not args.no_cpu_all_cores:
            # the reference is single-threaded, so the honest "all cores" figure is one independent
            # single-threaded forward per core, run concurrently (ctypes releases the GIL; the oracle has no shared state)
            import threading
            ncore = min(len(os.sched_getaffinity(0)), args.cpu_all_cores)
            ths = [threading.Thread(target=po.forward_image, args=(ocfg, host_imgs[i % n_distinct], weights))
                   for i in range(ncore)]
            t2 = time.perf_counter()
            for th in ths:
                th.start()
            for th in ths:
                th.join()
            all_dt = time.perf_counter() - t2
            cpu["all_cores"] = {"value": round(ncore / all_dt, 4), "unit": "images/sec", "cores": ncore,
                                "sample": f"{ncore} concurrent single-threaded forwards (one image each), {all_dt:.2f} s"}

    # ---- through the C surface (N = 1): host images in, host probability rows out ------------------
    c_surface = None
    if args.full and rank == 0 and world == 1 and not args.no_c_surface:
        import ctypes as C
        eng.set_profile(False)
        eng.set_lanes(args.lanes)
        host_batch = images.cpu().numpy()                  # the SAME batch, as B separately addressed host images
        host_probs = np.empty((B, cfg.num_classes), np.float32)
        in_ptrs = (binding.f32p * B)(*[host_batch[i].ctypes.data_as(binding.f32p) for i in range(B)])
        out_ptrs = (binding.f32p * B)(*[host_probs[i].ctypes.data_as(binding.f32p) for i in range(B)])
        reps = 3
        best = None
        for i in range(reps + 1):                          # the first call is a warm-up (pinned staging gets touched)
            t3 = time.perf_counter()
            rc = binding.lib().vit_engine_forward_host(eng._h, in_ptrs, B, out_ptrs)
            d3 = time.perf_counter() - t3
            if rc != 0:
                sys.exit("bench.py: vit_engine_forward_host failed")
            if i > 0:
                best = d3 if best is None else min(best, d3)
        same = bool(np.array_equal(host_probs, probs.cpu().numpy()))
        c_surface = {"value": round(B / best, 2), "unit": "images/sec", "ms_per_call": round(1e3 * best, 3),
                     "h2d_mb": round(host_batch.nbytes / 1e6, 1), "d2h_mb": round(host_probs.nbytes / 1e6, 3),
                     "sample": f"best of {reps} calls of vit_engine_forward_host on the timed batch ({B} images, pageable host "
                               "memory, pinned double-buffered staging inside the call)",
                     "bit_identical_to_device_path": same}

    # ---- how much of the gap to the roofline is clock (N = 1): the dominant GEMM's shape on busy and on quiet operands ------------
    if args.full and rank == 0 and world == 1 and not args.no_clock_probe and not args.prune_last_layer:
        roofline["clock_limit_probe"] = clock_limit_probe(binding, torch, dev, cfg, B if args.lanes == 1 else B // args.lanes, args.dtype)

    # ---- the other single-GPU configurations of BASELINE.json, each as a short timed run of its own (N = 1, headline only) ----------
    others = None
    headline = args.model == "b16" and args.dtype == "f32" and B == 256 and not args.prune_last_layer and not args.graph
    if args.full and rank == 0 and world == 1 and not distributed and headline and not args.no_other_configs:
        eng.close()                       # the headline engine's work is done: its 2 GB go back before the larger batches
        del images, probs
        torch.cuda.empty_cache()
        others = [other_config(pkg, binding, torch, np, dev, local_rank, 2, weights=weights),
                  other_config(pkg, binding, torch, np, dev, local_rank, 4)]

    ok = (gather_ok is not False) and (gold is None or (gold["top1_match"] and gold["max_abs_prob_err"] <= tol))
    if parity is not None:
        ok = ok and parity["top1_match"] and parity["max_abs_prob_err"] <= parity["tolerance"]
    if others:
        ok = ok and all(o["ok"] for o in others)
    if rank == 0:
        info = binding.device_info(local_rank)
        print(json.dumps({
            "metric": METRIC, "value": round(value, 2), "unit": "images/sec", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3), "per_rank_ms_per_step": per_rank_ms,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": args.dtype,
            "data": "synthetic",
            "config": {"workload": workload_name(args.model, args.dtype, B, args.config or (4 if args.model != "b16" else (1 if args.dtype == "f32" else 2))),
                       "batch_per_gpu": B, "global_batch": B * world, "parallelism": f"dp{world}", "lanes_per_gpu": args.lanes,
                       "top1_gather": ("rccl all_gather, 8 B per image" + ("" if gather_ok is not False else " (MISMATCH)")) if distributed else None,
                       "gflop_per_image": round(gflop_img, 4), "prune_last_layer": bool(args.prune_last_layer), "ln_fold": args.ln_fold >= 0, "device": info["name"], "arch": info["arch"],
                       "compute_units": info["compute_units"], "clock_mhz": info["clock_mhz"]},
            "roofline": roofline, "cpu_baseline": cpu, "parity": parity, "golden": gold, "c_surface": c_surface, "other_configs": others, "ok": ok,
        }))
    eng.close()
    if distributed:
        dist.destroy_process_group()
    if not ok:
        sys.exit(1)


if __name__ == "__main__":
    main()
