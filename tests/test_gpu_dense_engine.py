"""Dense linear heads on the engine (vit_engine_set_dense_head, vit_engine_dense_*), fp32 and bf16 engines.

Models: VIT_SMALL (patch 16, g = 4) and SMALL14 (patch 14 at 56 px, g = 4), depth 3; heads of 21 classes over one layer (the last) and
over all three, with and without the final LayerNorm on the taps.  What is checked against what:

  GRID    bit for bit the transposed chain of vithip_gemm_f32 launches (arith = 0) that include/vit_engine.h states, run here through
          the binding on the rows Engine.intermediate(kind="patches") returns for each tapped layer;
          fp32 engines: against the live oracle's stages within LOGIT_REL, the logits bar of tests/test_gpu_head_engine.py
  LABELS  the numpy model (tests/dense_head_model.py) applied to the call's own GRID, label for label, at 64 x 64 and 37 x 53
  bits    the same whatever lanes, prune_last_layer, the batch position and the input path
"""
import ctypes as C

import numpy as np
import pytest

import dense_head_model as M
from conftest import oracle_config
from engine_helpers import CONSTS, same_bits
from patch14_model import SMALL14
from strided import SENTINEL
from test_gpu_head_engine import LOGIT_REL, rel_err
from test_gpu_preproc import DeviceImages
from test_input_u8_model import normalise_u8
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

MODELS = {"small": synth.VIT_SMALL, "small14": SMALL14}
HEADS = {"last": (2,), "all": (0, 1, 2)}
CLASSES = 21
SIZES = [(64, 64), (37, 53)]
SEED = 31
ERR_ARG, ERR_STATE = 1, 5
_cache = {}


def weights(name):
    if ("w", name) not in _cache:
        _cache[("w", name)] = synth.make_weights(MODELS[name], SEED)
    return _cache[("w", name)]


def head(name, layers):
    """(weight [CLASSES][K * D], bias [CLASSES]) of a head over `layers`: logits of order 1 on normalised rows."""
    F = len(layers) * MODELS[name].embed_dim
    rng = np.random.default_rng(F)
    return (rng.standard_normal((CLASSES, F)) / np.sqrt(F)).astype(np.float32) * np.float32(3), rng.standard_normal(CLASSES).astype(np.float32)


@pytest.fixture(scope="module")
def engines():
    cache = {}

    def get(name, dtype="f32", **opt):
        key = (name, dtype, tuple(sorted(opt.items())))
        if key not in cache:
            eng = B.Engine(MODELS[name], dtype=dtype, **opt)
            eng.load_weights(weights(name))
            cache[key] = eng
        eng = cache[key]
        eng.reset_dense_head()  # engine state: every test sets its own
        eng.set_lanes(opt.get("lanes", 1))
        return eng

    yield get
    for eng in cache.values():
        eng.close()


def chain(eng, imgs, layers, norm, w, b):
    """The logits [n][P][CLASSES] as the header states them: vithip_gemm_f32 launches over the PATCHES rows of each tapped layer."""
    n, D, K = len(imgs), eng.cfg.embed_dim, len(layers)
    out = None
    for j, l in enumerate(layers):
        A = eng.intermediate(imgs, [l], "patches", norm)[:, 0].reshape(-1, D)
        Wj = w[:, j * D:(j + 1) * D]
        if j == 0:
            out = B.gemm(A, Wj, b, epilogue=B.EPI_BIAS, ldw=K * D)
        else:
            out = B.gemm(A, Wj, np.zeros(CLASSES, np.float32), residual=out, epilogue=B.EPI_BIAS_RESIDUAL, in_place=True, ldw=K * D)
    return out.reshape(n, -1, CLASSES)


def device_dense(eng, d_images, n, kind, out_size=None, u8=False, stream=0):
    spec = B.dense_spec(kind, out_size)
    shape = eng.dense_shape(n, spec)
    d_out = B.DeviceArray(shape, np.uint8 if kind == "labels" else np.float32)
    if u8:
        eng.dense_device_u8(d_images.ptr, n, d_out.ptr, kind, out_size, *CONSTS, stream=stream)
    else:
        eng.dense_device(d_images.ptr, n, d_out.ptr, kind, out_size, stream=stream)
    eng.sync()
    return d_out.numpy()


# ---- the stated bits ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("norm", [0, 1])
@pytest.mark.parametrize("hname", list(HEADS))
@pytest.mark.parametrize("name", list(MODELS))
def test_grid_is_the_gemm_chain_and_labels_are_the_model_on_the_grid(engines, name, hname, norm, dtype):
    cfg, layers = MODELS[name], HEADS[hname]
    eng = engines(name, dtype, max_batch=4)  # 7 images: a full chunk and a ragged one
    w, b = head(name, layers)
    eng.set_dense_head(w, b, layers, norm)
    imgs = synth.make_images(cfg, 7, 500)
    g = cfg.img_size // cfg.patch_size
    grid = eng.dense(imgs, "grid")
    assert grid.shape == (7, CLASSES, g, g) and grid.dtype == np.float32
    assert eng.dense_row_bytes("grid") == CLASSES * g * g * 4
    want = chain(eng, imgs, layers, norm, w, b)
    assert same_bits(grid.reshape(7, CLASSES, g * g), np.ascontiguousarray(want.transpose(0, 2, 1))), \
        int((grid.reshape(7, CLASSES, -1).view(np.uint32) != np.ascontiguousarray(want.transpose(0, 2, 1)).view(np.uint32)).sum())
    assert float(np.abs(grid).max()) > 0.5 and np.isfinite(grid).all()
    for oh, ow in SIZES:
        lab = eng.dense(imgs, "labels", (oh, ow))
        assert lab.shape == (7, oh, ow) and lab.dtype == np.uint8 and eng.dense_row_bytes("labels", (oh, ow)) == oh * ow
        model = np.stack([M.labels(M.grid_to_logits(grid[i]), g, oh, ow) for i in range(7)])
        assert np.array_equal(lab, model), (oh, ow, int((lab != model).sum()))
        assert lab.max() < CLASSES
    full = eng.dense(imgs[:2])  # no size: img_size x img_size
    assert full.shape == (2, cfg.img_size, cfg.img_size)
    assert np.array_equal(full, np.stack([M.labels(M.grid_to_logits(grid[i]), g, cfg.img_size, cfg.img_size) for i in range(2)]))
    with pytest.raises(B.VitError):  # nothing wrote the classifier's logits
        eng.logits(1)


@pytest.mark.parametrize("norm", [0, 1])
@pytest.mark.parametrize("hname", list(HEADS))
@pytest.mark.parametrize("name", list(MODELS))
def test_fp32_grid_matches_the_live_oracle_within_the_logit_bar(oracle, engines, name, hname, norm):
    cfg, layers, W = MODELS[name], HEADS[hname], weights(name)
    eng = engines(name, "f32", max_batch=4)
    w, b = head(name, layers)
    eng.set_dense_head(w, b, layers, norm)
    imgs = synth.make_images(cfg, 5, 501)
    if ("stages", name) not in _cache:
        _cache[("stages", name)] = [oracle.forward_image(oracle_config(cfg), im, W, want_stages=True)[2] for im in imgs]
    stages = _cache[("stages", name)]
    ref = []
    for st in stages:
        rows = [(oracle.layer_norm(st[l + 1], W[-4], W[-3]) if norm else st[l + 1])[1:] for l in layers]
        ref.append((np.concatenate(rows, axis=1).astype(np.float64) @ w.astype(np.float64).T + b.astype(np.float64)).T)
    ref = np.stack(ref)
    got = eng.dense(imgs, "grid").reshape(5, CLASSES, -1)
    err = rel_err(got, ref)
    print(f"fp32 {name} {hname} norm={norm}: grid max |d| / max |ref| = {err:.3e}")
    assert err <= LOGIT_REL, err


# ---- the same bits, however the pixels arrive ----------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_lanes_pruning_and_batch_position_change_no_bit(engines, dtype):
    name, layers = "small", HEADS["all"]
    w, b = head(name, layers)
    base = synth.make_images(MODELS[name], 3, 502)
    idx = np.array([0, 1, 2, 2, 0, 1, 1, 0, 2, 0, 1])  # chunks of 4, 4, 3
    plain = engines(name, dtype, max_batch=4)
    plain.set_dense_head(w, b, layers, 1)
    alone = {k: [plain.dense(base[i:i + 1], k, s)[0] for i in range(3)] for k, s in (("grid", None), ("labels", (37, 53)))}
    assert not same_bits(alone["grid"][0], alone["grid"][1])
    for opt in (dict(), dict(lanes=2), dict(prune_last_layer=True), dict(prune_last_layer=True, lanes=2)):
        eng = engines(name, dtype, max_batch=4, **opt)
        eng.set_dense_head(w, b, layers, 1)
        for kind, size in (("grid", None), ("labels", (37, 53))):
            got = eng.dense(base[idx], kind, size)
            for pos, k in enumerate(idx):
                assert same_bits(got[pos], alone[kind][k]), (opt, kind, pos)
        eng.set_dense_head(w[:, -192:], b, HEADS["last"], 1)  # the last layer alone: a pruning engine runs it unpruned for the call
        plain.set_dense_head(w[:, -192:], b, HEADS["last"], 1)
        assert same_bits(eng.dense(base[idx], "grid"), plain.dense(base[idx], "grid")), opt
        plain.set_dense_head(w, b, layers, 1)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(MODELS))
def test_the_six_input_paths_agree_bit_for_bit(engines, name, dtype):
    eng = engines(name, dtype, max_batch=4)
    cfg, n = eng.cfg, 11
    w, b = head(name, HEADS["all"])
    eng.set_dense_head(w, b, HEADS["all"], 1)
    u8 = np.random.default_rng(503).integers(0, 256, size=(n, cfg.img_size, cfg.img_size, cfg.in_chans), dtype=np.uint8)
    x = normalise_u8(u8, *CONSTS)
    d_x, d_u8, dev = B.DeviceArray.from_numpy(x), B.DeviceArray.from_numpy(u8), DeviceImages(list(u8), lead=0)
    before = eng.forward(x)
    for kind, size in (("labels", None), ("grid", None), ("labels", (37, 53))):  # the widest row first, an odd row of bytes last
        host = eng.dense(x, kind, size)
        assert same_bits(device_dense(eng, d_x, n, kind, size), host), kind
        assert same_bits(eng.dense_u8(u8, kind, size, *CONSTS), host), kind
        assert same_bits(device_dense(eng, d_u8, n, kind, size, u8=True), host), kind
        assert same_bits(eng.dense_images(list(u8), cfg.img_size, kind, size, *CONSTS), host), kind
        d_out = B.DeviceArray(host.shape, host.dtype)
        eng.dense_device_images(dev.triples, d_out.ptr, cfg.img_size, kind, size, *CONSTS)
        eng.sync()
        assert same_bits(d_out.numpy(), host), kind
    assert same_bits(eng.forward_u8(u8, *CONSTS), before)  # the probabilities still come through the (regrown) staging unharmed


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_graph_cache_keys_on_the_whole_dense_spec(engines, dtype):
    plain = engines("small", dtype, max_batch=8)
    graph = engines("small", dtype, max_batch=8, use_graph=True)
    w, b = head("small", HEADS["all"])
    for e in (plain, graph):
        e.set_dense_head(w, b, HEADS["all"], 1)
    n = 6
    d_images = B.DeviceArray.from_numpy(synth.make_images(plain.cfg, n, 504))
    calls = [("labels", (64, 64)), ("labels", (64, 64)), ("labels", (32, 128)), ("grid", None), ("labels", (64, 64)), ("grid", None)]
    want = {c: device_dense(plain, d_images, n, *c) for c in set(calls)}
    for c in calls:
        assert same_bits(device_dense(graph, d_images, n, *c), want[c]), c
    assert not same_bits(want[("labels", (64, 64))].reshape(-1), want[("labels", (32, 128))].reshape(-1))


# ---- independence ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_the_classifier_is_untouched_installs_remove_the_head_and_a_bad_image_stays_alone(engines, dtype):
    name = "small"
    eng = engines(name, dtype, max_batch=4)
    cfg = eng.cfg
    imgs = synth.make_images(cfg, 6, 505)
    probs = eng.forward(imgs)
    logits = eng.logits(2)
    w, b = head(name, HEADS["all"])
    eng.set_dense_head(w, b, HEADS["all"], 1)
    assert same_bits(eng.forward(imgs), probs) and same_bits(eng.logits(2), logits)
    grid, lab = eng.dense(imgs, "grid"), eng.dense(imgs, "labels", 64)
    # a caller's classifier head and the dense head do not disturb each other
    rng = np.random.default_rng(7)
    hw, hb = rng.standard_normal((cfg.num_classes, cfg.embed_dim)).astype(np.float32), rng.standard_normal(cfg.num_classes).astype(np.float32)
    eng.set_head(hw, hb, (-1,), "none")
    own = eng.forward(imgs)
    assert not same_bits(own, probs) and same_bits(eng.dense(imgs, "grid"), grid)
    eng.set_dense_head(w[:, :192], b, (0,), 0)
    assert same_bits(eng.forward(imgs), own) and not same_bits(eng.dense(imgs, "grid"), grid)
    eng.reset_head()
    eng.set_dense_head(w, b, HEADS["all"], 1)
    assert same_bits(eng.forward(imgs), probs) and same_bits(eng.dense(imgs, "grid"), grid)
    # a non-finite image reaches its own row only
    bad = imgs.copy()
    bad[2, 1, 5:9, 3] = np.nan
    bad[4, 0, 0, 0] = np.inf
    g2, l2 = eng.dense(bad, "grid"), eng.dense(bad, "labels", 64)
    keep = [0, 1, 3, 5]
    assert same_bits(g2[keep], grid[keep]) and same_bits(l2[keep], lab[keep])
    assert not np.isfinite(g2[2]).all() and not np.isfinite(g2[4]).all()
    assert np.array_equal(l2[2], M.labels(M.grid_to_logits(g2[2]), 4, 64, 64))
    # removing the head, and every weight install, leaves no dense head behind; the classifier goes on
    eng.reset_dense_head()
    with pytest.raises(B.VitError) as err:
        eng.dense(imgs)
    assert err.value.code == ERR_STATE and eng.dense_row_bytes("grid") == 0
    assert same_bits(eng.forward(imgs), probs)
    eng.set_dense_head(w, b, HEADS["all"], 1)
    eng.load_weights(weights(name))
    with pytest.raises(B.VitError) as err:
        eng.dense(imgs)
    assert err.value.code == ERR_STATE
    assert same_bits(eng.forward(imgs), probs)
    eng.set_dense_head(w, b, HEADS["all"], 1)
    assert same_bits(eng.dense(imgs, "grid"), grid)
    fresh = B.Engine(cfg, dtype=dtype, max_batch=4)
    try:
        with pytest.raises(B.VitError) as err:  # before any weights
            fresh.set_dense_head(w, b, HEADS["all"], 1)
        assert err.value.code == ERR_STATE
        fresh.copy_weights_from(eng)
        with pytest.raises(B.VitError) as err:  # a copy does not carry the head
            fresh.dense(imgs)
        assert err.value.code == ERR_STATE
    finally:
        fresh.close()


@pytest.mark.parametrize("lanes", [1, 2])
def test_only_the_tapped_layers_run_and_the_stages_are_accounted_as_stated(engines, lanes):
    eng = engines("small", "f32", max_batch=4, lanes=lanes, profile=True, ln_fold=-1)
    n = 4
    imgs = synth.make_images(eng.cfg, n, 506)
    w, b = head("small", HEADS["all"])

    def launches(fn):
        eng.reset_stage_times()
        fn()
        t = eng.stage_times()
        assert t["images"] == n
        return {s: v["launches"] for s, v in t["stages"].items()}

    gemms = ("qkv", "attn", "outproj", "fc1", "fc2")
    for layers in ((0,), (0, 1), (1,), (0, 1, 2)):
        K, deepest = len(layers), layers[-1] + 1
        eng.set_dense_head(w[:, :192 * K], b, layers, 1)
        for kind in ("labels", "grid"):
            got = launches(lambda: eng.dense(imgs, kind))
            assert all(got[s] == deepest * lanes for s in gemms), (layers, got)
            assert got["ln"] == (2 * deepest + K) * lanes and got["head"] == K * lanes and got["softmax"] == lanes, (layers, kind, got)


# ---- refusals ----------------------------------------------------------------------------------------------------------------

def test_refusals_change_nothing_and_enqueue_nothing(engines):
    L = B.lib()
    eng = engines("small", "f32", max_batch=4)
    cfg, n = eng.cfg, 3
    imgs = synth.make_images(cfg, n, 507)
    w, b = head("small", HEADS["all"])
    eng.set_dense_head(w, b, HEADS["all"], 1)
    ref_p, ref_g, ref_l = eng.forward(imgs), eng.dense(imgs, "grid"), eng.dense(imgs, "labels", (37, 53))
    d_x = B.DeviceArray.from_numpy(imgs)
    sent = SENTINEL[np.dtype(np.float32)]
    d_out = B.DeviceArray.from_numpy(np.full(n * 64 * 64, sent, np.uint32))

    def still_fine():
        assert L.vit_engine_last_error(eng._h)
        B.hip_check(L.vithip_device_sync(), "sync")
        assert (d_out.numpy() == sent).all(), "a refused call wrote to its output"
        assert same_bits(eng.forward(imgs), ref_p) and same_bits(eng.dense(imgs, "grid"), ref_g)
        assert same_bits(eng.dense(imgs, "labels", (37, 53)), ref_l)

    bad_specs = {"kind": B.dense_spec(2), "kind<0": B.dense_spec(-1), "reserved": B.dense_spec("labels", 64, reserved=1),
                 "grid with a size": B.dense_spec("grid", 64), "tall": B.dense_spec("labels", (4097, 64)), "wide": B.dense_spec("labels", (64, 4097)),
                 "negative": B.dense_spec("labels", (-1, 64))}
    for why, s in bad_specs.items():
        assert L.vit_engine_dense_device(eng._h, d_x.ptr, n, C.byref(s), d_out.ptr, None) == ERR_ARG, why
        assert L.vit_engine_dense_row_bytes(eng._h, C.byref(s)) == 0, why
        assert L.vit_engine_last_error(eng._h).decode().startswith("dense_device:"), why
        still_fine()
    good = C.byref(B.dense_spec("labels", 64))
    for d_images, nn, sp, out in [(None, n, good, d_out.ptr), (d_x.ptr, n, good, None), (d_x.ptr, n, None, d_out.ptr),
                                  (d_x.ptr, 0, good, d_out.ptr), (d_x.ptr, -1, good, d_out.ptr)]:
        assert L.vit_engine_dense_device(eng._h, d_images, nn, sp, out, None) == ERR_ARG
        still_fine()
    mean, std = (C.c_float * 3)(*B.IMAGENET_MEAN), (C.c_float * 3)(*B.IMAGENET_STD)
    zero_std = (C.c_float * 3)(0.229, 0.0, 0.225)
    d_u8 = B.DeviceArray.from_numpy(np.zeros((n, cfg.img_size, cfg.img_size, 3), np.uint8))
    for d_images, m, s in [(d_u8.ptr, None, std), (d_u8.ptr, mean, zero_std), (d_u8.ptr + 1, mean, std)]:
        assert L.vit_engine_dense_device_u8(eng._h, d_images, n, m, s, good, d_out.ptr, None) == ERR_ARG
        still_fine()
    out = np.zeros((n, 64, 64), np.uint8)
    rows = (C.c_void_p * n)(*[out[i].ctypes.data for i in range(n)])
    holes = (C.c_void_p * n)(*[out[i].ctypes.data if i != 1 else None for i in range(n)])
    in_f32 = (B.f32p * n)(*[imgs[i].ctypes.data_as(B.f32p) for i in range(n)])
    for ptrs, nn, sp, r in [(None, n, good, rows), (in_f32, n, good, None), (in_f32, 0, good, rows), (in_f32, n, None, rows),
                            (in_f32, n, C.byref(bad_specs["kind"]), rows), (in_f32, n, good, holes)]:
        assert L.vit_engine_dense_host(eng._h, ptrs, nn, sp, r) == ERR_ARG
        still_fine()
    assert not out.any()
    keep, recs = B.host_image_records([np.zeros((cfg.img_size, cfg.img_size, 3), np.uint8)] * n, cfg.in_chans)
    small_pp = B.preproc_params(cfg.img_size - 4, *CONSTS, cfg.in_chans)
    for p in (None, C.byref(small_pp)):
        assert L.vit_engine_dense_host_images(eng._h, recs, n, p, good, rows) == ERR_ARG
        still_fine()
    assert L.vit_engine_dense_row_bytes(eng._h, None) == 0 and L.vit_engine_dense_row_bytes(None, good) == 0
    assert L.vit_engine_dense_row_bytes(eng._h, good) == 64 * 64

    # a refused set_dense_head leaves the head in force as it was
    def hspec(layers=(0, 1, 2), norm=1, classes=CLASSES, reserved=0, num=None):
        s = B.dense_head_spec(layers, norm, classes, reserved=reserved)
        if num is not None:
            s.num_layers = num
        return s

    wp, bp = w.ctypes.data_as(B.f32p), b.ctypes.data_as(B.f32p)
    bad_heads = {"none": hspec(num=0), "negative count": hspec(num=-1), "too many": hspec(range(33)), "deep": hspec((0, 3)),
                 "negative layer": hspec((-1,)), "equal": hspec((1, 1)), "falling": hspec((2, 1)), "norm": hspec(norm=2),
                 "no classes": hspec(classes=0), "256 classes": hspec(classes=256), "reserved": hspec(reserved=1)}
    for why, s in bad_heads.items():
        assert L.vit_engine_set_dense_head(eng._h, C.byref(s), wp, bp) == ERR_ARG, why
        msg = L.vit_engine_last_error(eng._h).decode()
        assert msg.startswith("set_dense_head:"), msg
        if why in ("deep", "equal", "falling"):
            assert "layers[1]" in msg, msg
        if why == "negative layer":
            assert "layers[0]" in msg, msg
        still_fine()
    for s, ww, bb in [(C.byref(hspec()), None, bp), (C.byref(hspec()), wp, None), (None, wp, None), (None, None, bp)]:
        assert L.vit_engine_set_dense_head(eng._h, s, ww, bb) == ERR_ARG
        still_fine()
    assert L.vit_engine_set_dense_head(None, C.byref(hspec()), wp, bp) == ERR_ARG
    with pytest.raises(B.VitError):
        eng.set_dense_head(w[:, :100], b, HEADS["all"], 1)
    still_fine()
