"""Several engines in one process, weight replication, the packed weight cache on the device, the 2 GiB lane cap and the
RCCL gather of bench.py -- everything that a 1-GPU box can say about the multi-device path (the N = 8 run itself is the
driver's)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def small():
    cfg = synth.VIT_SMALL
    return cfg, synth.make_weights(cfg, 7), synth.make_images(cfg, 11, 8)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_weight_replication_device_to_device(small, dtype):
    cfg, W, imgs = small
    a = B.Engine(cfg, max_batch=16, dtype=dtype)
    a.load_weights(W)
    b = B.Engine(cfg, max_batch=16, dtype=dtype)
    with pytest.raises(B.VitError):
        b.forward(imgs)                                  # no weights yet
    b.copy_weights_from(a)
    pa, pb = a.forward(imgs), b.forward(imgs)
    assert np.array_equal(pa, pb)
    c = B.Engine(cfg, max_batch=16, dtype="bf16" if dtype == "f32" else "f32")
    with pytest.raises(B.VitError, match="dtype"):
        c.copy_weights_from(a)
    for e in (a, b, c):
        e.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_cache_loaded_engine_is_bit_identical_to_file_loaded_engine(small, dtype, tmp_path):
    cfg, W, imgs = small
    ref = B.Engine(cfg, max_batch=16, dtype=dtype)
    ref.load_weights(W)                                  # Network[] path: packed on the host, bf16 converted on the device
    want = ref.forward(imgs)
    host_img = B.WeightImage.build(cfg, W, with_bf16=True)  # bf16 section converted on the HOST (what vit_main --cache writes)
    path = str(tmp_path / "w.cache")
    assert host_img.save(path) == 0
    loaded = B.WeightImage.load(cfg, path)
    eng = B.Engine(cfg, max_batch=16, dtype=dtype)
    eng.load_weight_image(loaded)                        # one H2D, no conversion launch
    assert np.array_equal(eng.forward(imgs), want)
    dev_img = ref.read_weight_image()                    # the device's own bytes
    assert np.array_equal(dev_img.f32_section(), host_img.f32_section())
    if dtype == "bf16":
        assert np.array_equal(dev_img.bf16_section(), host_img.bf16_section())   # host RNE == v_cvt_pk_bf16_f32
    nob = B.WeightImage.build(cfg, W, with_bf16=False)   # an image without the bf16 section: converted on upload
    eng2 = B.Engine(cfg, max_batch=16, dtype=dtype)
    eng2.load_weight_image(nob)
    assert np.array_equal(eng2.forward(imgs), want)
    other = B.WeightImage.build(synth.VIT_TINY, synth.make_weights(synth.VIT_TINY, 1))
    with pytest.raises(B.VitError, match="another model"):
        eng2.load_weight_image(other)
    for e in (ref, eng, eng2):
        e.close()


def test_reloading_weights_invalidates_the_captured_graph(small):
    cfg, W, imgs = small
    n = imgs.shape[0]
    d_img = B.DeviceArray.from_numpy(imgs)
    d_out = B.DeviceArray((n, cfg.num_classes))
    eng = B.Engine(cfg, max_batch=16, use_graph=True)
    eng.load_weights(W)
    for _ in range(2):                                   # capture, then replay
        eng.forward_device(d_img.ptr, n, d_out.ptr)
    eng.sync()
    first = d_out.numpy().copy()
    W2 = synth.make_weights(cfg, 8)
    eng.load_weights(W2)                                 # frees / rewrites the weight blob the graph pointed into
    eng.forward_device(d_img.ptr, n, d_out.ptr)
    eng.sync()
    plain = B.Engine(cfg, max_batch=16)
    plain.load_weights(W2)
    want = plain.forward(imgs)
    assert np.array_equal(d_out.numpy(), want) and not np.array_equal(first, want)
    eng.close()
    plain.close()


def test_facade_with_two_engines_splits_the_image_loop():
    """VIT_HIP_DEVICES: one engine + host thread per listed device, image[0..n) cut into contiguous slices.  A 1-GPU box
    lists device 0 twice -- two engines, two threads, weights replicated device-to-device -- and must reproduce the
    single-engine result bit for bit, for even and ragged splits and for n < number of engines."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "vit_b16_e2e.npz"))
    cfg = synth.VIT_B16
    W = synth.make_weights(cfg, int(g["weight_seed"]))
    imgs = synth.make_images(cfg, 5, int(g["image_seed"]))
    single = B.facade_forward(imgs, W)
    assert B.lib().ViT_hip_device_count() == 0            # released
    os.environ["VIT_HIP_DEVICES"] = "0,0"
    try:
        L = B.lib()
        L.initialize_opencl()
        assert L.ViT_hip_device_count() == 2
        L.Release_opencl()
        for n in (5, 4, 1):
            got = B.facade_forward(imgs[:n], W)
            assert np.array_equal(got, single[:n]), n
    finally:
        del os.environ["VIT_HIP_DEVICES"]
    n_gold = min(5, int(g["n_images"]))
    assert float(np.abs(single[:n_gold] - g["probs"][:n_gold]).max()) <= 1e-4


def test_facade_on_all_devices_of_the_node():
    """VIT_HIP_DEVICES=all on a node with several GPUs: one engine per physical device, the weights replicated device-to-device
    (xGMI), image[0..n) cut into one contiguous slice per device.  Must reproduce the single-device result bit for bit.
    Skipped on a 1-GPU box (the same code path is covered there by VIT_HIP_DEVICES=0,0 above)."""
    import ctypes as C
    n_dev = C.c_int()
    B.hip_check(B.lib().vithip_device_count(C.byref(n_dev)), "vithip_device_count")
    if n_dev.value < 2:
        pytest.skip(f"needs >= 2 HIP devices, this box has {n_dev.value}")
    g = np.load(os.path.join(ROOT, "tests", "golden", "vit_b16_e2e.npz"))
    cfg = synth.VIT_B16
    W = synth.make_weights(cfg, int(g["weight_seed"]))
    n = 2 * n_dev.value + 1                                # ragged: one device gets an extra image
    imgs = synth.make_images(cfg, n, int(g["image_seed"]))
    single = B.facade_forward(imgs, W)
    os.environ["VIT_HIP_DEVICES"] = "all"
    try:
        L = B.lib()
        L.initialize_opencl()
        assert L.ViT_hip_device_count() == n_dev.value
        L.Release_opencl()
        got = B.facade_forward(imgs, W)
    finally:
        del os.environ["VIT_HIP_DEVICES"]
    assert np.array_equal(got, single)
    assert float(np.abs(single[:2] - g["probs"][:2]).max()) <= 1e-4


def _forward_with_top1(eng, dev, imgs, classes):
    """One device-resident forward that leaves the packed top-1 records [2][n] (labels | probability bits) in HBM."""
    import ctypes as C
    L = B.lib()
    B.hip_check(L.vithip_set_device(dev), "vithip_set_device")
    n = imgs.shape[0]
    d_img, d_probs, d_top1 = B.DeviceArray.from_numpy(imgs), B.DeviceArray((n, classes)), B.DeviceArray((2, n), np.int32)
    eng.forward_device(d_img.ptr, n, d_probs.ptr, d_top1.ptr, d_top1.ptr + 4 * n, 0)
    eng.sync()
    return d_img, d_probs, d_top1


def test_c_abi_rccl_gather_of_top1_records(small):
    """include/vit_dp.h (libvit_mi355x_dp.so): N engines driven through vit_engine_forward_device from one process gather their
    per-image top-1 records with one grouped ncclAllGather on device memory.  On this box: a communicator group of size 1 -- the
    gathered block must equal the local records, which must equal the probabilities' arg-max -- and, where the node has
    several GPUs, every device's gathered buffer against every device's own records (the shard axis is the reference's image
    loop, ViT_opencl.c:802)."""
    import ctypes as C
    if not os.path.exists(B.DP_LIB_PATH):
        pytest.skip("libvit_mi355x_dp.so not built on this box (no RCCL)")
    cfg, W, imgs = small
    n_dev = C.c_int()
    B.hip_check(B.lib().vithip_device_count(C.byref(n_dev)), "vithip_device_count")
    for devices in ([0], list(range(n_dev.value)) if n_dev.value >= 2 else None):
        if devices is None:
            continue
        nd = len(devices)
        per = 4                                             # images per device
        engines, held, sends, recvs = [], [], [], []
        for r, d in enumerate(devices):
            eng = B.Engine(cfg, max_batch=per, device=d)
            eng.load_weights(W)
            engines.append(eng)
            held.append(_forward_with_top1(eng, d, imgs[(r * per) % 8:(r * per) % 8 + per], cfg.num_classes))
            sends.append(held[-1][2].ptr)
            recvs.append(B.DeviceArray((nd, 2, per), np.int32))
        group = B.DpGroup(devices)
        assert B.dp_lib().vit_dp_size(group._h) == nd and B.dp_lib().vit_dp_device(group._h, 0) == devices[0]
        group.gather_top1(sends, [x.ptr for x in recvs], per)      # default streams
        own = []
        for r, d in enumerate(devices):
            B.hip_check(B.lib().vithip_set_device(d), "vithip_set_device")
            probs, top1 = held[r][1].numpy(), held[r][2].numpy()
            assert np.array_equal(top1[0], probs.argmax(1)) and np.array_equal(top1[1].view(np.float32), probs.max(1))
            own.append(top1)
        for r, d in enumerate(devices):
            B.hip_check(B.lib().vithip_set_device(d), "vithip_set_device")
            got = recvs[r].numpy()
            for q in range(nd):
                assert np.array_equal(got[q], own[q]), (devices, r, q)
        group.close()
        for eng in engines:
            eng.close()
        B.hip_check(B.lib().vithip_set_device(0), "vithip_set_device")
    with pytest.raises(B.VitError):
        B.DpGroup([0, 0])                                   # a group holds a device once


def test_fp32_chunk_is_capped_below_2gib_per_launch():
    """ViT-L/16-384 fp32: one image's MLP hidden rows are 9.45 MB, so 227 images fill the 2 GiB a buffer descriptor
    addresses (max_batch 256 used to fail mid-layer with hipErrorInvalidValue).  The engine now cuts the chunk."""
    cfg = synth.ModelConfig(img_size=384, embed_dim=1024, depth=1, num_heads=16, hidden_dim=4096)
    W = synth.make_weights(cfg, 31)
    n = 230
    imgs = np.tile(synth.make_images(cfg, 2, 32), (n // 2, 1, 1, 1))
    imgs += (np.arange(n, dtype=np.float32) * 1e-3).reshape(n, 1, 1, 1)
    big = B.Engine(cfg, max_batch=256, lanes=1)
    big.load_weights(W)
    got = big.forward(imgs)
    big.close()
    small_eng = B.Engine(cfg, max_batch=32, lanes=1)
    small_eng.load_weights(W)
    want = small_eng.forward(imgs)
    small_eng.close()
    assert np.array_equal(got, want)


def test_bench_rank_takes_the_rccl_path_at_world_size_one(tmp_path):
    """bench.py --spawn: the parent launches its rank (before touching the GPU), the rank initialises nccl (= RCCL),
    all-gathers the packed top-1 records through dp.gather_packed on the forward's stream, and prints the JSON line;
    --dump-outputs writes the gathered records beside the rank's own."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "VIT_LAUNCH_CHILD")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--spawn", "--steps", "2", "--warmup", "1",
                        "--batch", "16", "--no-cpu-baseline", "--full", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 1 and rec["config"]["top1_gather"] == "rccl all_gather, 8 B per image"
    assert rec["value"] > 0
    assert len(rec["per_rank_ms_per_step"]) == 1 and abs(rec["per_rank_ms_per_step"][0] - rec["ms_per_step"]) < 1e-2   # max over ranks
    # the line validates itself: golden rows inside the timed batch, every gather slot checked, the host-pointer surface
    assert rec["ok"] is True
    assert rec["golden"]["top1_match"] and rec["golden"]["max_abs_prob_err"] <= 1e-4 and rec["golden"]["ranks"] == 1
    assert rec["c_surface"]["bit_identical_to_device_path"] and rec["c_surface"]["value"] > 0
    assert rec["roofline"]["gemm_handover"] is not None
    probe = rec["roofline"]["clock_limit_probe"]      # the dominant GEMM's shape on random and on all-zero operands
    assert probe["shape_mnk"] == [16 * 197, 768, 3072] and probe["random_operands_tflops"] > 0 and probe["zero_operands_tflops"] > 0
    assert np.array_equal(np.load(tmp_path / "gathered_top1_label.npy"), np.load(tmp_path / "top1_label.npy")[None])
    assert np.array_equal(np.load(tmp_path / "gathered_top1_prob.npy"), np.load(tmp_path / "top1_prob.npy")[None])


def test_bench_config3_preset_is_bf16_2048_per_gpu():
    """--config 3 = BASELINE.json configs[3]'s per-GPU shape (bf16, 2,048 images per GPU); the bf16 line carries the golden
    parity block too (2e-2, identical top-1), measured on the timed batch itself."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "VIT_LAUNCH_CHILD")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "3", "--steps", "2", "--warmup", "1",
                        "--no-cpu-baseline", "--no-c-surface", "--full"], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert rec["dtype"] == "bf16" and rec["config"]["batch_per_gpu"] == 2048 and "configs[3]" in rec["config"]["workload"]
    assert rec["ok"] is True and rec["golden"]["top1_match"] and rec["golden"]["max_abs_prob_err"] <= 2e-2
    # the probe's SHAPE is the contract; how much faster the launch is on quiet operands is a property of the device in front of
    # us (power limit, cooling), reported in the line and never asserted here
    probe = rec["roofline"]["clock_limit_probe"]
    assert probe["shape_mnk"] == [1024 * 197, 2304, 768] and probe["random_operands_tflops"] > 0 and probe["zero_operands_tflops"] > 0, probe


def test_bench_default_line_carries_the_other_single_gpu_configs():
    """`python bench.py --full` (N = 1, configs[1]) also times BASELINE.json configs[2] and configs[4] after the
    headline's timed region and reports them under other_configs, each with its golden block: ViT-B/16 bf16 against the
    reference's own probabilities, ViT-L/16-384 bf16 against tests/golden/vit_l16_384_e2e.npz (2e-2, identical top-1)."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "VIT_LAUNCH_CHILD")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--no-cpu-baseline",
                        "--no-c-surface", "--no-clock-probe", "--full"], capture_output=True, text=True, timeout=1200, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert rec["dtype"] == "f32" and rec["config"]["batch_per_gpu"] == 256 and rec["ok"] is True
    assert rec["golden"]["fixture"] == "tests/golden/vit_b16_e2e.npz" and rec["golden"]["max_abs_prob_err"] <= 1e-4
    others = rec["other_configs"]
    assert [("configs[2]" in o["workload"], "configs[4]" in o["workload"]) for o in others] == [(True, False), (False, True)]
    for o, fixture in zip(others, ("tests/golden/vit_b16_e2e.npz", "tests/golden/vit_l16_384_e2e.npz")):
        assert o["dtype"] == "bf16" and o["value"] > 0 and o["ok"] is True
        assert o["golden"]["fixture"] == fixture and o["golden"]["top1_match"] and o["golden"]["max_abs_prob_err"] <= 2e-2
        assert 0 < o["roofline"]["frac"] < 1 and o["roofline"]["kernel"].startswith("gemm_bf16_pp_kernel")


def test_bench_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    """A plain run (no --full) prints the headline fields and nothing that takes work of its own; --dump-outputs writes what
    the last timed step returned.  The batch opens with the two golden images, so rows 0-1 of the dump must match
    tests/golden/vit_b16_e2e.npz (1e-4, identical top-1), and the top-1 records must point at each row's maximum."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "VIT_LAUNCH_CHILD")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", "16", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0 and rec["dtype"] == "f32"
    assert rec["unit"] == "images/sec" and rec["higher_is_better"] is True and rec["ok"] is True
    assert abs(rec["value"] - 16 * 1e3 / rec["ms_per_step"]) <= 1e-2 * rec["value"]
    assert all(rec[k] is None for k in ("roofline", "cpu_baseline", "parity", "golden", "c_surface", "other_configs"))
    probs = np.load(tmp_path / "probs.npy")
    label, p1 = np.load(tmp_path / "top1_label.npy"), np.load(tmp_path / "top1_prob.npy")
    assert probs.dtype == np.float32 and probs.shape == (16, 1000)
    assert label.dtype == np.float64 and p1.dtype == np.float32 and label.shape == p1.shape == (16,)
    assert np.array_equal(probs[np.arange(16), label.astype(int)], p1) and np.array_equal(p1, probs.max(1))
    g = np.load(os.path.join(ROOT, "tests", "golden", "vit_b16_e2e.npz"))
    assert np.abs(probs[:2] - g["probs"]).max() <= 1e-4 and (probs[:2].argmax(1) == g["probs"].argmax(1)).all()


@pytest.mark.parametrize("n_images", [6, 5])
def test_two_ranks_shard_the_batch_over_hip_engines(small, n_images):
    """The data-parallel path with the HIP engine as each rank's forward: two rank processes (started by the launcher
    bench.py uses) forward their contiguous shard on their own engine, all-gather the top-1 records, and rank 0 holds the
    whole batch's labels / probabilities -- equal to one engine forwarding everything."""
    import io
    import importlib
    pkg = importlib.import_module("vision-transformer-opencl_amd")
    worker = os.path.join(ROOT, "tests", "workers", "dp_gpu_worker.py")
    rc, out = pkg.launch.launch_ranks(worker, [str(n_images)], 2, timeout=600, relay_stdout=io.StringIO())
    assert rc == 0
    rec = json.loads([l for l in out.splitlines() if l.startswith("{")][0])
    cfg, W, _ = small
    eng = B.Engine(cfg, max_batch=8)
    eng.load_weights(W)
    full = eng.forward(synth.make_images(cfg, n_images, 8))
    eng.close()
    assert rec["world"] == 2 and rec["n_local"] == pkg.dp.shard_range(n_images, 0, 2)[1]
    assert rec["labels"] == full.argmax(1).tolist()
    assert np.array_equal(np.asarray(rec["probs"], np.float32), full.max(1))
