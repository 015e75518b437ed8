"""Classifier heads as engine state (vit_engine_set_head): pooled and multi-layer operands for the head GEMM, fp32 and bf16 engines.

Models: TINY14 (T = 5), a depth-4 copy of SMALL14 at 56 px (T = 17: the pooled block is exactly one segment of 16 rows) and the same
at 70 px (T = 26: a ragged second segment).  References: tests/head_model.py on the live oracle's stages.  Bars, those of
tests/test_gpu_patch14_engine.py: fp32 probabilities 1e-4 (PROB_TOL) with the same top-1, logits and fp32 rows 1e-3 of max |ref|
(LOGIT_REL), bf16 probabilities 2e-2 (BF16_PROB_TOL) with the same top-1, the bf16 operand 2e-2 of max |ref| (BF16_ROW_REL); the head
GEMM against float64 on the engine's own operand within the fp32 op bar REL = 2e-5.  Everything promised bit-identical is compared
bitwise.

The heads' weights are random; of the seeds 0, 1, 2, ... a (model, family) takes the first whose REFERENCE probabilities keep, for
every test image, a gap of more than 2 * BF16_PROB_TOL between the best and the second class: an output within the bar then cannot
have another top-1 than the reference, so "same top-1" tests the engine and not the luck of a near tie.  The choice reads the
oracle only.
"""
import dataclasses

import numpy as np
import pytest

import head_model
from conftest import oracle_config
from engine_helpers import CONSTS, device_forward, read_back, same_bits
from patch14_model import SMALL14, TINY14
from test_input_u8_model import normalise_u8
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

PROB_TOL, LOGIT_REL, BF16_PROB_TOL, BF16_ROW_REL = 1e-4, 1e-3, 2e-2, 2e-2
REL = 2e-5  # tests/test_gpu_ops.py
ROW_BAR = {"f32": LOGIT_REL, "bf16": BF16_ROW_REL}
DEEP14 = dataclasses.replace(SMALL14, depth=4)        # T = 17
DEEP14_70 = dataclasses.replace(DEEP14, img_size=70)  # T = 26
MODELS = {"tiny14": TINY14, "deep14": DEEP14, "deep14_70": DEEP14_70}
assert (DEEP14.tokens, DEEP14_70.tokens) == (17, 26)
SEED = 23
NS = (1, 3, 8)
LOGIT_SPREAD = 3.0  # standard deviation of an image's reference logits over the classes
ERR_ARG, ERR_STATE = 1, 5
_cache = {}


def rel_err(got, ref) -> float:
    return float(np.abs(got - ref).max()) / float(np.abs(ref).max())


def weights(name):
    if ("w", name) not in _cache:
        _cache[("w", name)] = synth.make_weights(MODELS[name], SEED)
    return _cache[("w", name)]


def oracle_run(oracle, name, n):
    """(images, stages per image) of the live oracle, computed once per (model, n)."""
    key = ("oracle", name, n)
    if key not in _cache:
        cfg = MODELS[name]
        imgs = synth.make_images(cfg, n, 200 + n)
        _cache[key] = (imgs, [oracle.forward_image(oracle_config(cfg), im, weights(name), want_stages=True)[2] for im in imgs])
    return _cache[key]


def reference(oracle, name, family):
    """The head of (model, family) and the reference per n: (cls_layers, pool, weight, bias, {n: (rows, logits, probs)})."""
    key = ("ref", name, family)
    if key not in _cache:
        cfg, W = MODELS[name], weights(name)
        cls_layers, pool = head_model.families(cfg.depth)[family]
        rows = {n: head_model.operands(oracle, oracle_run(oracle, name, n)[1], W[-4], W[-3], cls_layers, pool) for n in NS}
        for seed in range(64):
            w, b = head_model.make_head(cfg.num_classes, rows[1].shape[1], seed)
            # a pooled block of synthetic images is small (the mean of P nearly independent rows): scale the weight so that the
            # reference logits of an image spread by LOGIT_SPREAD over the classes, as a trained head's do
            spread = float(np.mean([(rows[n].astype(np.float64) @ w.astype(np.float64).T).std(1).mean() for n in NS]))
            w *= np.float32(LOGIT_SPREAD / spread)
            lg = {n: head_model.logits(oracle, rows[n], w, b) for n in NS}
            pr = {n: head_model.probs(oracle, lg[n]) for n in NS}
            top2 = np.concatenate([np.sort(pr[n], 1)[:, -2:] for n in NS])
            if float((top2[:, 1] - top2[:, 0]).min()) > 2 * BF16_PROB_TOL:
                break
        else:
            raise AssertionError(f"no head with a clear top-1 among 64 seeds for {name} {family}")
        _cache[key] = (cls_layers, pool, w, b, {n: (rows[n], lg[n], pr[n]) for n in NS})
    return _cache[key]


def families(name):
    return list(head_model.families(MODELS[name].depth))


CASES = [(name, fam) for name in MODELS for fam in families(name)]


@pytest.fixture(scope="module")
def engines():
    cache = {}

    def get(name, dtype, **opt):
        key = (name, dtype, tuple(sorted(opt.items())))
        if key not in cache:
            eng = B.Engine(MODELS[name], dtype=dtype, **opt)
            eng.load_weights(weights(name))
            cache[key] = eng
        eng = cache[key]
        eng.reset_head()  # a head is engine state: every test starts from the checkpoint's own
        eng.set_lanes(opt.get("lanes", 1))
        return eng

    yield get
    for eng in cache.values():
        eng.close()


def set_family(eng, oracle, name, family):
    cls_layers, pool, w, b, ref = reference(oracle, name, family)
    eng.set_head(w, b, cls_layers, pool)
    return cls_layers, pool, w, b, ref


# ---- accuracy --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name,family", CASES)
def test_probabilities_logits_and_operand_match_the_head_model(oracle, engines, name, family, dtype):
    cfg = MODELS[name]
    eng = engines(name, dtype, max_batch=4)  # 8 images: the chunk loop; 3: a ragged chunk
    cls_layers, pool, w, b, ref = set_family(eng, oracle, name, family)
    F = head_model.in_features(cfg.embed_dim, cls_layers, pool)
    assert eng.head_in_features(cls_layers, pool) == F == w.shape[1]
    for n in NS:
        imgs = oracle_run(oracle, name, n)[0]
        ref_rows, ref_l, ref_p = ref[n]
        probs = eng.forward(imgs)
        err = float(np.abs(probs - ref_p).max())
        print(f"{dtype} {name} {family} n={n}: max |dprob| = {err:.3e}")
        assert err <= (PROB_TOL if dtype == "f32" else BF16_PROB_TOL), (n, err)
        assert (probs.argmax(1) == ref_p.argmax(1)).all(), n
        last = n % 4 or 4  # the taps hold the last chunk
        logits, rows = eng.logits(last), eng.head_operand(last)
        assert rows.shape == (last, F)
        e_rows = rel_err(rows, ref_rows[-last:])
        print(f"{dtype} {name} {family} n={n}: operand max |d| / max |ref| = {e_rows:.3e}")
        assert e_rows <= ROW_BAR[dtype], (n, e_rows)
        if dtype == "f32":
            e_l = rel_err(logits, ref_l[-last:])
            print(f"f32 {name} {family} n={n}: logits max |d| / max |ref| = {e_l:.3e}")
            assert e_l <= LOGIT_REL, (n, e_l)
        # the head GEMM on the engine's own operand: fp32 on both dtypes
        gemm = rows.astype(np.float64) @ w.astype(np.float64).T + b.astype(np.float64)
        e_g = rel_err(logits.astype(np.float64), gemm)
        print(f"{dtype} {name} {family} n={n}: head GEMM max |d| / max |ref| = {e_g:.3e}")
        assert e_g <= REL, (n, e_g)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name,family", CASES)
def test_operand_is_the_bits_of_the_intermediate_and_features_calls(oracle, engines, name, family, dtype):
    cfg, W = MODELS[name], weights(name)
    eng = engines(name, dtype, max_batch=4)
    n, D = 3, cfg.embed_dim
    imgs = oracle_run(oracle, name, n)[0]
    blocks = []
    cls_layers, pool = head_model.families(cfg.depth)[family]
    if cls_layers:
        blocks.append(eng.intermediate(imgs, list(cls_layers), "cls", 1).reshape(n, len(cls_layers) * D))
    if pool == "avg":
        blocks.append(eng.features(imgs, "mean"))
    elif pool == "avg_fcnorm":  # the kernel on the engine's own last-layer rows (position independent: any batch gives these bits)
        x_last = eng.intermediate(imgs, [cfg.depth - 1], "tokens", 0).reshape(n * cfg.tokens, D)
        fused = B.pool_layernorm(x_last, W[-4], W[-3], n, cfg.tokens, 1)
        assert same_bits(fused, B.layernorm(B.pool_layernorm(x_last, None, None, n, cfg.tokens, 1), W[-4], W[-3]))
        blocks.append(fused)
    want = np.concatenate(blocks, 1)
    set_family(eng, oracle, name, family)
    eng.forward(imgs)
    assert same_bits(eng.head_operand(n), want)


# ---- same bits ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name,family", [("tiny14", "dinov2_1"), ("deep14", "dinov2_4"), ("deep14", "timm_fcnorm"), ("deep14", "probe")])
def test_every_input_path_and_topk_give_the_forwards_bits(oracle, engines, name, family, dtype):
    cfg = MODELS[name]
    eng = engines(name, dtype, max_batch=4)
    set_family(eng, oracle, name, family)
    n, S = 5, cfg.img_size
    u8 = np.random.default_rng(5).integers(0, 256, (n, S, S, cfg.in_chans), dtype=np.uint8)
    imgs = normalise_u8(u8, *CONSTS)
    want = eng.forward(imgs)
    assert np.isfinite(want).all()
    dev, label, prob = device_forward(eng, B.DeviceArray.from_numpy(imgs), n)
    assert same_bits(dev, want)
    assert (label == want.argmax(1)).all() and same_bits(prob, want.max(1))
    assert same_bits(eng.forward_u8(u8, *CONSTS), want)
    assert same_bits(device_forward(eng, B.DeviceArray.from_numpy(u8), n, CONSTS)[0], want)
    assert same_bits(eng.forward_images([im for im in u8], S, *CONSTS), want)  # decoded images already of the model's size
    d_u8 = [B.DeviceArray.from_numpy(im) for im in u8]
    d_p = B.DeviceArray((n, cfg.num_classes))
    eng.forward_device_images([(d.ptr, S, S) for d in d_u8], d_p.ptr, S, *CONSTS)
    assert same_bits(read_back(eng, d_p, (n, cfg.num_classes)), want)
    k = 5
    labels, scores = B.split_topk(eng.topk_host(imgs, k))
    assert (labels[:, 0] == want.argmax(1)).all()
    assert same_bits(scores, np.take_along_axis(want, labels, 1))
    assert (np.diff(scores, axis=1) <= 0).all()
    d_rec = B.DeviceArray((n, 2 * k), np.int32)
    eng.topk_device(B.DeviceArray.from_numpy(imgs).ptr, n, d_rec.ptr, k)
    eng.sync()
    assert same_bits(d_rec.numpy(), eng.topk_host(imgs, k))


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name,family", [("deep14", "dinov2_4"), ("deep14_70", "timm_fcnorm"), ("deep14_70", "dinov2_1")])
def test_lanes_and_batch_position_change_no_bit(oracle, engines, name, family, dtype):
    cfg = MODELS[name]
    eng = engines(name, dtype, max_batch=8)
    set_family(eng, oracle, name, family)
    base = synth.make_images(cfg, 4, 301)
    idx = np.array([0, 1, 2, 3, 3, 0, 2, 1, 1, 3, 0])  # 11 images: chunks of 8 and 3, every image at several places
    imgs = base[idx]
    want = eng.forward(imgs)
    rows = eng.head_operand(3)  # the last chunk: images 1, 3, 0
    for k in range(4):
        assert (want[idx == k] == want[idx == k][0]).all(), k
    alone = eng.forward(base)
    assert same_bits(alone, want[[0, 1, 2, 3]])  # and in another batch
    assert same_bits(eng.head_operand(4)[[1, 3, 0]], rows)
    try:
        eng.set_lanes(2)
        assert same_bits(eng.forward(imgs), want)
        assert same_bits(eng.head_operand(3), rows)
        assert same_bits(eng.forward(base), alone)
    finally:
        eng.set_lanes(1)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("family", ["probe", "dinov2_4", "timm_avg", "timm_fcnorm"])
def test_prune_last_layer_changes_no_bit(oracle, engines, family, dtype):
    """NONE: the last layer stays pruned (only class rows are read); a pooled block: it runs unpruned for the call, silently."""
    name = "deep14"
    plain, pruned = engines(name, dtype, max_batch=4), engines(name, dtype, max_batch=4, prune_last_layer=True)
    imgs = oracle_run(oracle, name, 8)[0]
    default = plain.forward(imgs)
    assert same_bits(pruned.forward(imgs), default)
    set_family(plain, oracle, name, family)
    set_family(pruned, oracle, name, family)
    want = plain.forward(imgs)
    assert not same_bits(want, default)
    assert same_bits(pruned.forward(imgs), want)
    assert same_bits(pruned.head_operand(4), plain.head_operand(4))
    assert same_bits(pruned.logits(4), plain.logits(4))
    pruned.reset_head()
    assert same_bits(pruned.forward(imgs), default)  # and pruned again


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("prune", [False, True])
@pytest.mark.parametrize("name,n,lanes", [("tiny14", 3, 1), ("deep14_70", 8, 2)])  # lanes split only when n >= 2 * lanes
def test_the_checkpoints_head_set_as_a_callers_head_gives_the_own_heads_bits(engines, name, n, lanes, prune, dtype):
    """The own head is the instance {cls_layers = (depth - 1,), pool none} over the checkpoint's head tensors: set by the caller it
    issues the own head's launches, so every output of the head has the own head's bits, and the operand is D wide in both states."""
    cfg, W = MODELS[name], weights(name)
    eng = engines(name, dtype, max_batch=8 if lanes > 1 else 4, **({"prune_last_layer": True} if prune else {}))
    eng.set_lanes(lanes)
    d_img = B.DeviceArray.from_numpy(synth.make_images(cfg, n, 200 + n))
    k = 3

    def outputs():  # probabilities, top-1 labels, top-1 probabilities, logits, operand rows, top-k records
        out = list(device_forward(eng, d_img, n)) + [eng.logits(n), eng.head_operand(n)]
        d_rec = B.DeviceArray((n, 2 * k), np.int32)
        eng.topk_device(d_img.ptr, n, d_rec.ptr, k)
        eng.sync()
        return out + [d_rec.numpy()]

    own = outputs()
    assert np.isfinite(own[0]).all() and (own[1] == own[0].argmax(1)).all() and own[4].shape == (n, cfg.embed_dim)
    eng.set_head(W[-2], W[-1], (cfg.depth - 1,), "none")
    assert eng.head_in_features((cfg.depth - 1,), "none") == cfg.embed_dim
    for state in ("set_head", "reset_head"):
        got = outputs()
        assert got[4].shape == (n, cfg.embed_dim), state
        for what, a, b in zip(("probs", "labels", "top-1 probs", "logits", "operand", "top-k records"), got, own):
            assert same_bits(a, b), (state, what)
        eng.reset_head()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_captured_graph_does_not_outlive_the_head_it_was_captured_with(oracle, engines, dtype):
    name = "deep14"
    plain, graph = engines(name, dtype, max_batch=4), engines(name, dtype, max_batch=4, use_graph=True)
    n = 3
    imgs = oracle_run(oracle, name, n)[0]
    d_img = B.DeviceArray.from_numpy(imgs)
    d_p, d_l, d_q = B.DeviceArray((n, MODELS[name].num_classes)), B.DeviceArray((n,), np.int32), B.DeviceArray((n,))

    def run():  # the same pointers every time: the second call of a kind replays the graph of the first
        graph.forward_device(d_img.ptr, n, d_p.ptr, d_l.ptr, d_q.ptr)
        return read_back(graph, d_p, (n, MODELS[name].num_classes))

    default = plain.forward(imgs)
    assert same_bits(run(), default) and same_bits(run(), default)
    for family in ("dinov2_4", "timm_fcnorm"):
        set_family(plain, oracle, name, family)
        set_family(graph, oracle, name, family)
        want = plain.forward(imgs)
        assert not same_bits(want, default)
        assert same_bits(run(), want) and same_bits(run(), want), family
    graph.reset_head()
    assert same_bits(run(), default) and same_bits(run(), default)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["tiny14", "deep14_70"])
def test_the_other_outputs_do_not_see_the_head(oracle, engines, name, dtype):
    cfg = MODELS[name]
    eng = engines(name, dtype, max_batch=4)
    imgs = oracle_run(oracle, name, 3)[0]
    layers = list(range(cfg.depth))

    def others():
        return [eng.features(imgs, "cls"), eng.features(imgs, "mean", True), eng.features(imgs, "tokens"), eng.cls_attention(imgs, "heads"),
                eng.cls_attention(imgs, "head_mean"), eng.intermediate(imgs, layers, "cls", 1), eng.intermediate(imgs, layers, "tokens", 0),
                eng.intermediate(imgs, [cfg.depth - 1], "map", 1)]

    before = others()
    for family in families(name):
        set_family(eng, oracle, name, family)
        eng.forward(imgs)
        for got, want in zip(others(), before):
            assert same_bits(got, want), family


# ---- state -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_reset_head_and_every_weight_install_restore_the_checkpoints_own_head(oracle, engines, dtype):
    name = "deep14"
    cfg = MODELS[name]
    eng = engines(name, dtype, max_batch=4)
    imgs = oracle_run(oracle, name, 3)[0]
    default, default_rows = eng.forward(imgs), eng.head_operand(3)
    assert default_rows.shape == (3, cfg.embed_dim) and same_bits(default_rows, eng.features(imgs, "cls"))
    eng.forward(imgs)
    default_logits = eng.logits(3)
    other = B.Engine(cfg, dtype=dtype, max_batch=4)
    try:
        other.load_weights(weights(name))
        installs = {"reset_head": eng.reset_head, "load_weights": lambda: eng.load_weights(weights(name)),
                    "load_weight_image": lambda: eng.load_weight_image(other.read_weight_image()),
                    "copy_weights": lambda: eng.copy_weights_from(other)}
        for what, install in installs.items():
            set_family(eng, oracle, name, "dinov2_4")
            assert not same_bits(eng.forward(imgs), default), what
            assert eng.head_operand(3).shape == (3, 5 * cfg.embed_dim)
            install()
            assert same_bits(eng.forward(imgs), default), what
            assert same_bits(eng.logits(3), default_logits) and same_bits(eng.head_operand(3), default_rows), what
        # a head is per engine: copying the weights of an engine with a head copies none
        set_family(other, oracle, name, "timm_avg")
        eng.copy_weights_from(other)
        assert same_bits(eng.forward(imgs), default)
        # one head after another on a resident backbone
        for family in families(name):
            _, _, _, _, ref = set_family(eng, oracle, name, family)
            assert (eng.forward(imgs).argmax(1) == ref[3][2].argmax(1)).all(), family
    finally:
        other.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_refused_heads_change_nothing(oracle, engines, dtype):
    name = "deep14"
    cfg = MODELS[name]
    eng = engines(name, dtype, max_batch=4)
    imgs = oracle_run(oracle, name, 3)[0]
    NC, D, depth = cfg.num_classes, cfg.embed_dim, cfg.depth
    w, b = np.ones((NC, 40 * D), np.float32), np.ones(NC, np.float32)
    L = B.lib()

    def raw(spec, weight=w, bias=b):
        return L.vit_engine_set_head(eng._h, None if spec is None else B.C.byref(spec), None if weight is None else weight.ctypes.data_as(B.f32p),
                                     None if bias is None else bias.ctypes.data_as(B.f32p))

    good = B.head_spec((depth - 1,), "avg")
    bad = {"no weight": (good, None, b), "no bias": (good, w, None), "null spec with a weight": (None, w, None),
           "null spec with a bias": (None, None, b), "too many layers": (B.head_spec(range(33), "none"), w, b),
           "negative count": (B.CHeadSpec(-1), w, b), "layer == depth": (B.head_spec((depth,), "none"), w, b),
           "negative layer": (B.head_spec((-1,), "none"), w, b), "layers not increasing": (B.head_spec((2, 1), "avg"), w, b),
           "a layer twice": (B.head_spec((1, 1), "avg"), w, b), "unknown pool": (B.head_spec((0,), 3), w, b),
           "negative pool": (B.head_spec((0,), -1), w, b), "reserved": (B.head_spec((0,), "avg", reserved=1), w, b),
           "empty operand": (B.head_spec((), "none"), w, b)}
    for state in ("own head", "dinov2_1"):
        if state != "own head":
            set_family(eng, oracle, name, state)
        before, rows = eng.forward(imgs), eng.head_operand(3)
        for what, (spec, weight, bias) in bad.items():
            assert raw(spec, weight, bias) == ERR_ARG, what
            if spec is not None:
                assert L.vit_engine_head_in_features(eng._h, B.C.byref(spec)) == (0 if "weight" not in what and "bias" not in what else 2 * D), what
            assert same_bits(eng.forward(imgs), before) and same_bits(eng.head_operand(3), rows), (state, what)
    msg = B.lib().vit_engine_last_error
    assert raw(B.head_spec((0, 2, 1), "avg")) == ERR_ARG and b"cls_layers[2] = 1" in msg(eng._h)
    assert raw(B.head_spec((0, depth), "avg")) == ERR_ARG and f"cls_layers[1] = {depth}".encode() in msg(eng._h)
    with pytest.raises(B.VitError):  # the binding checks the sizes it can
        eng.set_head(np.ones((NC, D), np.float32), b, (depth - 1,), "avg")
    fresh = B.Engine(cfg, dtype=dtype, max_batch=2)
    try:
        with pytest.raises(B.VitError) as err:
            fresh.set_head(np.ones((NC, 2 * D), np.float32), b, (depth - 1,), "avg")
        assert err.value.code == ERR_STATE
        with pytest.raises(B.VitError) as err:
            fresh.reset_head()
        assert err.value.code == ERR_STATE
        fresh.load_weights(weights(name))
        assert same_bits(fresh.forward(imgs[:2]), eng_default(eng, imgs)[:2])
    finally:
        fresh.close()


def eng_default(eng, imgs):
    eng.reset_head()
    return eng.forward(imgs)
