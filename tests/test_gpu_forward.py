"""End-to-end parity of the HIP forward (through the C-ABI) with the oracle and the golden vectors.

Bars (north_star): probabilities within 1e-4 absolute of ViT_seq.c, top-1 argmax identical;
logits within 1e-3 relative.  tests/golden/vit_b16_e2e.npz was written by the
reference's own ViT_seq.c compiled in the build container (oracle/gen_golden.py).
"""
import os

import numpy as np
import pytest

from conftest import oracle_config
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "vit_b16_e2e.npz")
PROB_TOL = 1e-4
LOGIT_REL = 1e-3


def check(probs, logits, ref_probs, ref_logits):
    assert float(np.abs(probs - ref_probs).max()) <= PROB_TOL
    assert (probs.argmax(1) == ref_probs.argmax(1)).all()
    if logits is not None:
        scale = float(np.abs(ref_logits).max())
        assert float(np.abs(logits - ref_logits).max()) <= LOGIT_REL * scale


@pytest.mark.parametrize("cfg,batches", [(synth.VIT_TINY, (1, 2, 5, 11)), (synth.VIT_SMALL, (1, 3, 8))])
def test_small_models_match_live_oracle(oracle, cfg, batches):
    W = synth.make_weights(cfg, 21)
    ocfg = oracle_config(cfg)
    eng = B.Engine(cfg, max_batch=4)  # max_batch 4 < 5, 8: exercises the chunk loop and ragged tails
    eng.load_weights(W)
    for n in batches:
        imgs = synth.make_images(cfg, n, 100 + n)
        probs = eng.forward(imgs)
        ref = [oracle.forward_image(ocfg, imgs[i], W) for i in range(n)]
        ref_p = np.stack([r[0] for r in ref])
        check(probs, None, ref_p, None)
        last = n % 4 or 4  # logits tap holds the last chunk
        ref_l = np.stack([r[1] for r in ref])[-last:]
        scale = float(np.abs(ref_l).max())
        assert float(np.abs(eng.logits(last) - ref_l).max()) <= LOGIT_REL * scale
    eng.close()


@pytest.fixture(scope="module")
def b16():
    W = synth.make_weights(synth.VIT_B16, 1234)
    eng = B.Engine(synth.VIT_B16, max_batch=256)
    eng.load_weights(W)
    yield eng, W
    eng.close()


def test_b16_matches_reference_golden(b16):
    eng, _ = b16
    g = np.load(GOLD)
    n = int(g["n_images"])
    assert int(g["weight_seed"]) == 1234
    imgs = synth.make_images(synth.VIT_B16, n, int(g["image_seed"]))
    probs = eng.forward(imgs)
    check(probs, eng.logits(n), g["probs"], g["logits"])


def test_b16_facade_with_reference_names(b16):
    """initialize_opencl -> ViT_opencl(ImageData*, Network*, float**) -> Release_opencl."""
    _, W = b16
    g = np.load(GOLD)
    imgs = synth.make_images(synth.VIT_B16, 1, int(g["image_seed"]))
    probs = B.facade_forward(imgs, W, use_reference_names=True)
    check(probs, None, g["probs"][:1], None)


def test_b16_batch256_position_invariance_and_golden(b16):
    """Full metric batch: 256 images = 16 distinct x 16 copies in a shuffled order.  Copies of
    one image must give bit-identical rows wherever they sit in the batch, rows must sum to 1,
    and the two golden images inside the batch must still match the reference."""
    eng, _ = b16
    g = np.load(GOLD)
    base = synth.make_images(synth.VIT_B16, 16, int(g["image_seed"]))  # images 0,1 are the golden ones
    order = np.random.default_rng(0).permutation(256)
    idx = np.arange(256) % 16
    idx = idx[order]
    probs = eng.forward(base[idx])
    for k in range(16):
        rows = probs[idx == k]
        assert (rows == rows[0]).all(), f"image {k}: rows differ with batch position"
    assert np.allclose(probs.sum(1), 1.0, atol=1e-5)
    for k in (0, 1):
        row = probs[idx == k][0]
        assert float(np.abs(row - g["probs"][k]).max()) <= PROB_TOL
        assert int(row.argmax()) == int(g["probs"][k].argmax())


def test_device_resident_path_matches_host_path(b16):
    """vit_engine_forward_device on HBM pointers (what bench.py times) == the host-pointer path."""
    eng, _ = b16
    imgs = synth.make_images(synth.VIT_B16, 5, 321)
    host = eng.forward(imgs)
    d_in = B.DeviceArray.from_numpy(imgs)
    d_out = B.DeviceArray((5, 1000))
    d_lab = B.DeviceArray((5,), np.int32)
    d_pr = B.DeviceArray((5,))
    eng.forward_device(d_in.ptr, 5, d_out.ptr, d_lab.ptr, d_pr.ptr)
    eng.sync()
    dev = d_out.numpy()
    assert np.array_equal(dev, host)
    assert (d_lab.numpy() == host.argmax(1)).all()
    assert np.array_equal(d_pr.numpy(), host.max(1))


def test_missing_weight_is_reported_by_index():
    cfg = synth.VIT_TINY
    W = synth.make_weights(cfg, 3)
    eng = B.Engine(cfg, max_batch=2)
    with pytest.raises(B.VitError, match="forward before"):
        eng.forward(synth.make_images(cfg, 1, 1))
    broken = list(W)
    broken[6] = None  # in_proj_weight of layer 0 -- one of the blobs the reference repo lacks
    with pytest.raises(B.VitError, match="weight 6 is missing"):
        eng.load_weights(broken)
    broken[6] = W[6].ravel()[:-1]
    with pytest.raises(B.VitError, match="weight 6 has"):
        eng.load_weights(broken)
    eng.close()


def test_unsupported_config_is_rejected():
    with pytest.raises(B.VitError, match="head_dim"):
        B.Engine(synth.ModelConfig(img_size=32, embed_dim=128, num_heads=4, depth=1, hidden_dim=256))
    with pytest.raises(B.VitError, match="multiples of 32"):
        B.Engine(synth.ModelConfig(img_size=32, embed_dim=64, num_heads=1, depth=1, hidden_dim=100))


LONG_SEQ = synth.ModelConfig(img_size=384, num_classes=50, embed_dim=128, depth=2, num_heads=2, hidden_dim=256)
VIT_L_2LAYERS = synth.ModelConfig(img_size=384, embed_dim=1024, depth=2, num_heads=16, hidden_dim=4096)


@pytest.mark.parametrize("cfg", [LONG_SEQ, VIT_L_2LAYERS], ids=["577tokens-narrow", "vit-l-16-384-width-2-layers"])
def test_vit_l_geometry_matches_oracle(oracle, cfg):
    """ViT-L/16-384 geometry (577 tokens, K/V-chunked attention; D=1024, H=4096, 16 heads).  The
    reference fixes ViT-B with macros (ViT_seq.c:10-21), so the oracle here is the parametrised
    restatement that is bit-identical to the reference at ViT-B/16."""
    W = synth.make_weights(cfg, 31)
    eng = B.Engine(cfg, max_batch=2)
    eng.load_weights(W)
    imgs = synth.make_images(cfg, 2, 32)
    probs = eng.forward(imgs)
    ocfg = oracle_config(cfg)
    ref = [oracle.forward_image(ocfg, imgs[i], W) for i in range(2)]
    check(probs, eng.logits(2), np.stack([r[0] for r in ref]), np.stack([r[1] for r in ref]))
    eng.close()


@pytest.mark.parametrize("lanes", [1, 2], ids=["lanes1", "lanes2"])
@pytest.mark.parametrize("prune", [False, True], ids=["full", "pruned"])
@pytest.mark.parametrize("ln_fold", [-1, 0], ids=["nofold", "fold"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_stage_profile_counts_launches(dtype, ln_fold, prune, lanes):
    """The launch list of every layer sequence (dtype x LayerNorm fold x pruned last layer), per stage: each stage is issued once
    per lane; the pruned last layer adds a Q launch, and with the fold a gather of the class rows' statistics (LN)."""
    cfg = synth.VIT_TINY
    eng = B.Engine(cfg, max_batch=4, profile=True, dtype=dtype, ln_fold=ln_fold, prune_last_layer=prune, lanes=lanes)
    eng.load_weights(synth.make_weights(cfg, 3))
    eng.forward(synth.make_images(cfg, 4, 1))
    t = eng.stage_times()
    assert t["images"] == 4
    if (dtype, ln_fold, prune, lanes) == ("f32", 0, False, 1):  # the default engine
        assert t["stages"]["fc1"]["launches"] == cfg.depth
        assert t["stages"]["ln"]["launches"] == 2 * cfg.depth + 1
    fold = ln_fold >= 0  # VIT_TINY meets the fold's shape rules in both dtypes
    d = cfg.depth
    per_lane = {"embed": 1, "ln": 2 * d + 1 + (prune and fold), "qkv": d + prune, "attn": d, "outproj": d, "fc1": d,
                "fc2": d, "head": 1, "softmax": 1}
    assert {s: v["launches"] for s, v in t["stages"].items()} == {s: lanes * k for s, k in per_lane.items()}
    assert all(v["ms"] >= 0 for v in t["stages"].values())
    eng.close()


@pytest.mark.parametrize("lanes", [2, 3])
def test_concurrent_lanes_give_identical_results(b16, lanes):
    """Sub-batches on separate streams (engine option `lanes`) must not change a single bit."""
    eng, W = b16
    imgs = synth.make_images(synth.VIT_B16, 7, 4321)
    ref = eng.forward(imgs)
    eng.set_lanes(lanes)
    try:
        got = eng.forward(imgs)
    finally:
        eng.set_lanes(1)
    assert np.array_equal(got, ref)


def _forward_device(eng, imgs, classes=1000):
    """One vit_engine_forward_device call on HBM-resident images: the whole batch is ONE chunk (the host-pointer path cuts a
    single chunk in two pieces to overlap its copies), i.e. the GEMM shapes bench.py times."""
    n = imgs.shape[0]
    d_in, d_out = B.DeviceArray.from_numpy(imgs), B.DeviceArray((n, classes))
    eng.forward_device(d_in.ptr, n, d_out.ptr)
    eng.sync()
    return d_out.numpy()


def _batch256():
    g = np.load(GOLD)
    base = synth.make_images(synth.VIT_B16, 16, int(g["image_seed"]))  # images 0,1 are the golden ones
    idx = (np.arange(256) % 16)[np.random.default_rng(1).permutation(256)]
    return g, base[idx], idx


@pytest.mark.parametrize("lanes", [2, 3])
def test_b16_batch256_lanes_with_handover_are_bit_identical(b16, lanes):
    """The metric batch with 2 and 3 concurrent lanes: every lane's fc1 / fc2 / out_proj hands helper pieces over
    (csrc/vit_gemm_persistent.hip) while the other lanes' kernels share the CUs, so a lane's 512 workgroups are NOT all
    resident -- the case in which round 2's owner could wait for a helper that had not started.  Nothing waits now: an owner that
    finds no piece computes its tile whole.  Results must equal the one-lane run bit for bit and the golden rows."""
    eng, _ = b16
    g, imgs, idx = _batch256()
    eng.handover_stats()
    ref = _forward_device(eng, imgs)
    one = eng.handover_stats()
    assert one["taken"] + one["recomputed"] == 12 * (316 + 316 + 240)   # owners per layer: out_proj, fc2 (2364 tiles - 4 x 512), fc1 (9456 - 18 x 512)
    eng.set_lanes(lanes)
    try:
        got = _forward_device(eng, imgs)
        many = eng.handover_stats()
    finally:
        eng.set_lanes(1)
    assert np.array_equal(got, ref)
    assert many["taken"] + many["recomputed"] > 0
    print(f"hand-overs: 1 lane {one}, {lanes} lanes {many}")
    for k in (0, 1):
        row = got[idx == k][0]
        assert float(np.abs(row - g["probs"][k]).max()) <= PROB_TOL
        assert int(row.argmax()) == int(g["probs"][k].argmax())


def test_b16_batch256_with_late_helpers_is_bit_identical(b16):
    """`gemm_handover_test = 1`: every helper workgroup runs its pieces LAST, so the owners look for them too early, withdraw
    and compute their tiles whole (and the helpers, arriving late, clear the withdrawn marks).  Same bits as the normal run."""
    eng, W = b16
    g, imgs, idx = _batch256()
    ref = _forward_device(eng, imgs)
    late = B.Engine(synth.VIT_B16, max_batch=256, gemm_handover_test=1)
    try:
        late.copy_weights_from(eng)
        got = _forward_device(late, imgs)
        st = late.handover_stats()
    finally:
        late.close()
    assert np.array_equal(got, ref)
    assert st["recomputed"] > 0 and st["taken"] + st["recomputed"] == 12 * (316 + 316 + 240), st


@pytest.mark.parametrize("prune", [False, True])
def test_b16_batch256_row_statistics_from_the_gemm_epilogue_are_bit_identical(b16, prune):
    """At the metric batch the two residual GEMMs of every layer take the row statistics of the LayerNorm that follows them in
    their own epilogue (vithip_gemm_args.stats_out; csrc/vit_gemm_common.hpp): of the 25 statistics passes only layer 0's and the
    head's LayerNorm stay launches (pruned last layer: plus the class rows' pass and the copy of their pairs).  An engine held to
    the one-tile-per-workgroup kernel (gemm_tile = 10: a statistics pass behind every residual GEMM) must give the same bits."""
    eng, _ = b16
    g, imgs, idx = _batch256()
    depth = synth.VIT_B16.depth
    outs = {}
    for tile in (0, 10):
        e2 = B.Engine(synth.VIT_B16, max_batch=256, profile=True, gemm_tile=tile, prune_last_layer=prune)
        try:
            e2.copy_weights_from(eng)
            outs[tile] = _forward_device(e2, imgs)
            launches = e2.stage_times()["stages"]["ln"]["launches"]
        finally:
            e2.close()
        assert launches == ((4 if prune else 2) if tile == 0 else 2 * depth + 1 + (1 if prune else 0)), (tile, launches)
    assert np.array_equal(outs[0], outs[10])
    assert np.array_equal(outs[0], _forward_device(eng, imgs))
    for k in (0, 1):
        row = outs[0][idx == k][0]
        assert float(np.abs(row - g["probs"][k]).max()) <= PROB_TOL
        assert int(row.argmax()) == int(g["probs"][k].argmax())


def test_b16_layernorm_fold_fp32_stays_within_the_bar(b16):
    """fp32 engines fold the encoder LayerNorms into in_proj / fc1 by default (vit_engine_options.ln_fold; the GEMMs multiply the
    raw rows with gamma-folded weights and rescale in the epilogue).  That is another operation order than ViT_seq.c:103-147, so
    it is held to the same bar: the golden rows of the reference's own ViT_seq() within 1e-4 with the same top-1, at the metric
    batch -- and next to the unfolded engine (ln_fold = -1, the reference's order), which it must track far inside the bar."""
    eng, _ = b16
    g, imgs, idx = _batch256()
    folded = _forward_device(eng, imgs)
    plain = B.Engine(synth.VIT_B16, max_batch=256, ln_fold=-1)
    try:
        plain.copy_weights_from(eng)
        unfolded = _forward_device(plain, imgs)
    finally:
        plain.close()
    assert not np.array_equal(folded, unfolded)          # (the default engine does fold)
    diff = float(np.abs(folded - unfolded).max())
    print(f"fp32 LayerNorm fold: max |dprob| against the unfolded engine {diff:.3g}")
    assert diff <= 2e-5
    assert np.array_equal(folded.argmax(1), unfolded.argmax(1))
    for out in (folded, unfolded):
        for k in (0, 1):
            row = out[idx == k][0]
            assert float(np.abs(row - g["probs"][k]).max()) <= PROB_TOL
            assert int(row.argmax()) == int(g["probs"][k].argmax())


def test_empty_and_invalid_inputs(b16):
    """Empty input: the facade is a no-op for image[0].n == 0 (the reference's loop simply would not run,
    ViT_opencl.c:802); the engine API rejects n <= 0 and NULL rows with an error code instead of crashing."""
    import ctypes as C
    eng, W = b16
    L = B.lib()
    img = np.zeros((3, 224, 224), np.float32)
    one = (B.CImageData * 1)(B.CImageData(0, 3, 224, 224, img.ctypes.data_as(B.f32p)))
    nets, keep = B.networks_from(W)
    rows = (B.f32p * 1)()
    L.initialize_hip()
    L.ViT_hip(one, nets, rows)      # n == 0: returns without touching rows
    L.Release_hip()
    with pytest.raises(B.VitError, match="bad arguments"):
        eng.forward(np.zeros((0, 3, 224, 224), np.float32))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_prune_last_layer_is_bit_identical(dtype):
    """vit_engine_options.prune_last_layer: the last encoder layer computes only what the class token needs.  Every
    operator computes its rows independently of how many rows it is given, so probabilities and logits must be
    IDENTICAL to the full forward, bit for bit (ViT-B/16 golden images plus a batch that spans lanes)."""
    cfg = synth.VIT_B16
    W = synth.make_weights(cfg, 1234)
    imgs = synth.make_images(cfg, 9, 99)
    outs = []
    for prune in (False, True):
        eng = B.Engine(cfg, max_batch=16, lanes=2, dtype=dtype, prune_last_layer=prune)
        eng.load_weights(W)
        p = eng.forward(imgs)
        outs.append((p.copy(), eng.logits(9).copy()))
        eng.close()
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1])


def test_attention_rows_only_touches_the_requested_rows():
    """vithip_attention_f32_rows(q_rows = 1): row 0 of every image equals the full attention's row 0, the other rows
    of the output buffer keep their previous contents."""
    n, T, heads = 3, 197, 12
    qkv = synth.uniform(999, 70, n * T * 3 * heads * 64, -1.0, 1.0).reshape(n * T, 3 * heads * 64)
    full = B.attention(qkv, n, T, heads)
    got = B.attention_rows(qkv, n, T, heads, 1, fill=7.0)
    for b in range(n):
        assert np.array_equal(got[b * T], full[b * T])
        assert (got[b * T + 1:(b + 1) * T] == 7.0).all()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_graph_replay_matches_direct_launches(dtype):
    """vit_engine_options.use_graph: the first device-path forward captures the launch sequence into a hipGraph and
    runs it, later forwards with the same arguments replay it; all of them must equal the directly launched forward."""
    cfg = synth.VIT_SMALL
    W = synth.make_weights(cfg, 21)
    n = 5
    a, b = synth.make_images(cfg, n, 3), synth.make_images(cfg, n, 4)
    ref = {}
    for use_graph in (False, True):
        eng = B.Engine(cfg, max_batch=4, dtype=dtype, use_graph=use_graph)   # max_batch 4: two chunks inside one graph
        eng.load_weights(W)
        d_img = B.DeviceArray.from_numpy(a)
        d_probs = B.DeviceArray((n, cfg.num_classes))
        d_lab, d_p = B.DeviceArray((n,), np.int32), B.DeviceArray((n,))
        outs = []
        for images in (a, b, a):          # capture + run, replay on new data, replay again
            B.hip_check(B.lib().vithip_memcpy_h2d(d_img.ptr, np.ascontiguousarray(images).ctypes.data, images.nbytes, None), "h2d")
            B.hip_check(B.lib().vithip_device_sync(), "sync")
            eng.forward_device(d_img.ptr, n, d_probs.ptr, d_lab.ptr, d_p.ptr)
            eng.sync()
            outs.append((d_probs.numpy().copy(), d_lab.numpy().copy()))
        eng.close()
        ref[use_graph] = outs
    for (p0, l0), (p1, l1) in zip(ref[False], ref[True]):
        assert np.array_equal(p0, p1) and np.array_equal(l0, l1)
    assert not np.array_equal(ref[True][0][0], ref[True][1][0])   # the replay really saw the new images
    assert np.array_equal(ref[True][0][0], ref[True][2][0])


def test_vit_l16_384_full_depth_matches_oracle(oracle):
    """BASELINE.json configs[4] at its REAL depth: ViT-L/16 384x384, 24 layers, D = 1024, 16 heads, H = 4096, 577 tokens
    (chunked online-softmax attention end to end).  The reference fixes ViT-B with macros (ViT_seq.c:10-21), so the
    oracle here is the parametrised restatement that is bit-identical to the reference at ViT-B/16 (16 OpenMP threads).
    fp32: probabilities within 1e-4, logits within 1e-3 relative; bf16: same top-1, probabilities within 2e-2."""
    from conftest import oracle_config
    cfg = synth.VIT_L16_384
    assert (cfg.depth, cfg.embed_dim, cfg.tokens) == (24, 1024, 577)
    W = synth.make_weights(cfg, 41)
    imgs = synth.make_images(cfg, 2, 42)
    ref_p, ref_l = [], []
    for i in range(2):
        p, l, _ = oracle.forward_image(oracle_config(cfg), imgs[i], W)
        ref_p.append(p)
        ref_l.append(l)
    ref_p, ref_l = np.stack(ref_p), np.stack(ref_l)
    for dtype, tol in (("f32", 1e-4), ("bf16", 2e-2)):
        eng = B.Engine(cfg, max_batch=2, dtype=dtype)
        eng.load_weights(W)
        probs = eng.forward(imgs)
        logits = eng.logits(2)
        eng.close()
        err = float(np.abs(probs - ref_p).max())
        lerr = float(np.abs(logits - ref_l).max() / np.abs(ref_l).max())
        print(f"ViT-L/16-384 depth 24 {dtype}: max |dprob| = {err:.3e}, logits rel err = {lerr:.3e}, pmax = {float(ref_p.max()):.3f}")
        assert (probs.argmax(1) == ref_p.argmax(1)).all(), dtype
        assert err <= tol, dtype
        if dtype == "f32":
            assert lerr <= 1e-3
        else:
            # the configuration's own regime: 272 images = 4,352 (image, head) items for the streamed attention's 256
            # persistent workgroups, 613 row-tiles for the ping-pong GEMMs, two lanes.  Copies of the two oracle-checked images
            # scattered through the batch must come out exactly as in the 2-image run, wherever they sit.
            n = 272
            idx = (np.arange(n) % 2)[np.random.default_rng(3).permutation(n)]
            big = B.Engine(cfg, max_batch=n, dtype="bf16", lanes=2)
            big.load_weights(W)
            got = _forward_device(big, imgs[idx], cfg.num_classes)
            big.close()
            assert np.array_equal(got, probs[idx]), "ViT-L/16-384 bf16: a row depends on the batch it is computed in"
