"""Engines of register-token models (VIT_REGISTER_TOKENS; DINOv2 `_reg4`): every output against tests/register_model.py, the float64
model that tests/test_register_model.py pins to transformers' Dinov2WithRegisters*, and one transformers model through INTEGRATION.md's
table.  The live oracle knows no registers.

Reduced configs of head_dim 64 (tests/register_model.py): REG_TINY (T = 9), REG_SMALL (T = 21), REG_ODD (image 42, R = 1, T = 11),
REG_16 (patch 16: the 16-byte gather and the bf16 patch-row GEMM, T = 21), REG_261 (224 / 14 with R = 4: T = 261, the sequence length
of the published checkpoints through the attention kernels).
Bars: the project's -- fp32: probabilities 1e-4 with the same top-1; logits, features and intermediate rows 1e-3 of max |ref|;
bf16: probabilities 2e-2, the same top-1 wherever the reference's top-2 gap exceeds 2e-2, rows 2e-2 of max |ref|
(tests/test_gpu_patch14_engine.py); class-token attention 1e-4 (fp32) / 2e-2 (bf16).  What the engine promises to keep
bit-identical is compared bitwise.
"""
import numpy as np
import pytest

import dense_head_model
import register_model
from engine_helpers import CONSTS, device_attention, device_features, device_forward, same_bits
from register_model import cls_attention_ref
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

PROB_TOL, LOGIT_REL, BF16_PROB_TOL, BF16_ROW_REL = 1e-4, 1e-3, 2e-2, 2e-2
ROW_BAR = {"f32": LOGIT_REL, "bf16": BF16_ROW_REL}
CLS_CAP = {"f32": 1e-4, "bf16": 2e-2}
CONFIGS = {"REG_TINY": register_model.REG_TINY, "REG_SMALL": register_model.REG_SMALL, "REG_ODD": register_model.REG_ODD,
           "REG_16": register_model.REG_16, "REG_261": register_model.REG_261}
W_SEED = 21
# Image seeds chosen on the CPU (register_model's probabilities, no GPU involved): the first seed from 7 on at which more than half of
# the five images have a top-2 gap above 2e-2; test_the_image_seeds_leave_most_images_clear asserts it.
IMG_SEED = {"REG_TINY": 7, "REG_SMALL": 7, "REG_ODD": 7, "REG_16": 7, "REG_261": 7}
ERR_ARG, ERR_WEIGHTS = 1, 2
_cache = {}


def rel_err(got, ref) -> float:
    return float(np.abs(got - ref).max()) / float(np.abs(ref).max())


def weights(name):
    if ("w", name) not in _cache:
        _cache[("w", name)] = synth.make_weights(CONFIGS[name], W_SEED)
    return _cache[("w", name)]


def images(name, n=5):
    if ("i", name) not in _cache:
        _cache[("i", name)] = synth.make_images(CONFIGS[name], 5, IMG_SEED[name])
    return _cache[("i", name)][:n]


def model(name):
    """register_model.forward on the five images, computed once per config and left unchanged."""
    if ("m", name) not in _cache:
        _cache[("m", name)] = register_model.forward(CONFIGS[name], images(name), weights(name))
    return _cache[("m", name)]


def tap_layers(cfg):
    """The first and the last layer: two layers on every config but REG_261, whose depth is 1 (one layer of the real sequence length)."""
    return sorted({0, cfg.depth - 1})


def model_rows(name, what, layer=None, norm=True):
    """The reference of one row output: features "cls" | "mean" | "tokens", or intermediate "cls" | "tokens" | "patches" | "map" of
    `layer`."""
    cfg, m, W = CONFIGS[name], model(name), weights(name)
    R = cfg.num_register_tokens
    if layer is None:
        return {"cls": m["norm"][:, 0], "mean": m["norm"][:, 1 + R:].mean(1), "tokens": m["norm"]}[what]
    rows = m["stages"][:, layer + 1]
    if norm:
        rows = register_model.layer_norm(rows, np.asarray(W[-4], np.float64), np.asarray(W[-3], np.float64), 1e-6)
    return {"cls": rows[:, 0], "tokens": rows, "patches": rows[:, 1 + R:],
            "map": np.stack([register_model.patch_map(cfg, r) for r in rows])}[what]


@pytest.fixture(scope="module")
def engines():
    cache = {}

    def get(name, **opt):
        key = (name, tuple(sorted(opt.items())))
        if key not in cache:
            cache[key] = B.Engine(CONFIGS[name], **opt)
            cache[key].load_weights(weights(name))
        return cache[key]

    yield get
    for eng in cache.values():
        eng.close()


def check_rows(eng, name, dtype, n=5):
    """Every row output of `eng` on the first n images against the model; returns the worst relative error."""
    cfg, imgs, bar, worst = CONFIGS[name], images(name, n), ROW_BAR[dtype], 0.0
    T, P, D = cfg.tokens, cfg.patches, cfg.embed_dim
    g = cfg.img_size // cfg.patch_size
    for kind, shape in (("cls", (n, D)), ("mean", (n, D)), ("tokens", (n, T, D))):
        got = eng.features(imgs, kind)
        err = rel_err(got, model_rows(name, kind)[:n])
        assert got.shape == shape and err <= bar, (kind, got.shape, err)
        worst = max(worst, err)
    layers = tap_layers(cfg)
    for norm in (0, 1):
        for kind, block in (("cls", (D,)), ("tokens", (T, D)), ("patches", (P, D)), ("map", (D, g, g))):
            got = eng.intermediate(imgs, layers, kind, bool(norm))
            assert got.shape == (n, len(layers)) + block, (kind, got.shape)
            for j, l in enumerate(layers):
                err = rel_err(got[:, j], model_rows(name, kind, l, norm)[:n])
                assert err <= bar, (kind, norm, l, err)
                worst = max(worst, err)
    return worst


# ---- 0: the image seeds, on the CPU side of the test -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CONFIGS))
def test_the_image_seeds_leave_most_images_clear(name):
    top2 = np.sort(model(name)["probs"], axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > BF16_PROB_TOL
    assert clear.sum() * 2 >= len(clear), (name, top2)


# ---- 1: fp32 engines against the model -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fp32_split", [0, -1], ids=["split", "fp32-mfma"])
@pytest.mark.parametrize("ln_fold", [0, -1], ids=["ln-auto", "ln-kernels"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_fp32_engines_match_the_register_model(engines, name, ln_fold, fp32_split):
    cfg = CONFIGS[name]
    eng = engines(name, max_batch=4, ln_fold=ln_fold, fp32_split=fp32_split)
    ref_p, ref_l = model(name)["probs"], model(name)["logits"]
    for n in (1, 3, 5):  # one chunk, a ragged one, the chunk loop
        probs = eng.forward(images(name, n))
        last = n % 4 or 4  # the logits tap holds the last chunk
        err, lerr = float(np.abs(probs - ref_p[:n]).max()), rel_err(eng.logits(last), ref_l[n - last:n])
        print(f"fp32 {name} n={n} ln_fold={ln_fold} fp32_split={fp32_split}: max |dprob| = {err:.3e}, logits {lerr:.3e}")
        assert err <= PROB_TOL and (probs.argmax(1) == ref_p[:n].argmax(1)).all(), (n, err)
        assert lerr <= LOGIT_REL, (n, lerr)
    worst = check_rows(eng, name, "f32")
    print(f"fp32 {name} ln_fold={ln_fold} fp32_split={fp32_split}: features / intermediate rows, worst {worst:.3e} of max |ref|")
    # the registers really are skipped: the mean over rows 1 .. is another vector, further away than the bar
    R = cfg.num_register_tokens
    wrong = model(name)["norm"][:, 1:].mean(1)
    got = eng.features(images(name), "mean")
    assert rel_err(model_rows(name, "mean"), wrong) > LOGIT_REL  # the two readings differ by more than the bar in the first place
    assert rel_err(got, wrong) > LOGIT_REL, (R, rel_err(got, wrong))


# ---- 2: bf16 engines -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ln_fold", [0, -1], ids=["ln-folded", "ln-kernels"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_bf16_engines_match_the_register_model(engines, name, ln_fold):
    eng = engines(name, max_batch=4, dtype="bf16", ln_fold=ln_fold)
    ref_p = model(name)["probs"]
    probs = eng.forward(images(name))
    err = float(np.abs(probs - ref_p).max())
    print(f"bf16 {name} ln_fold={ln_fold}: max |dprob| = {err:.3e}")
    assert err <= BF16_PROB_TOL, err
    top2 = np.sort(ref_p, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > BF16_PROB_TOL
    assert clear.sum() * 2 >= len(clear)
    assert (probs.argmax(1) == ref_p.argmax(1))[clear].all()
    assert err > 1e-6  # really the bf16 path: fp32 engines sit orders below
    worst = check_rows(eng, name, "bf16")
    print(f"bf16 {name} ln_fold={ln_fold}: features / intermediate rows, worst {worst:.3e} of max |ref|")
    assert worst > 1e-6


# ---- 3: heads --------------------------------------------------------------------------------------------------------------------------

def test_a_transformers_model_with_registers_maps_through_the_table_to_the_engine():
    """Dinov2WithRegistersForImageClassification (tests/test_register_model.py): tensor 0 = [cls_token | register_tokens], LayerScale
    folded, the classifier through set_head(cls_layers=(-1,), pool="avg"); the hidden states through intermediate TOKENS."""
    from test_register_model import hf_reference
    cfg, W, cw, cb, imgs, hidden, normed, ref = hf_reference()
    assert cfg == register_model.REG_TINY
    eng = B.Engine(cfg, max_batch=4)
    try:
        eng.load_weights(W)
        eng.set_head(cw, cb, (-1,), "avg")
        eng.forward(imgs)
        lerr = rel_err(eng.logits(len(imgs)), ref)
        herr = rel_err(eng.intermediate(imgs, [cfg.depth - 1], "tokens", False)[:, 0], hidden)
        nerr = rel_err(eng.features(imgs, "tokens"), normed)
        print(f"transformers Dinov2WithRegisters: logits {lerr:.3e}, hidden_states[-1] {herr:.3e}, last_hidden_state {nerr:.3e} of max |ref|")
        assert lerr <= LOGIT_REL and herr <= LOGIT_REL and nerr <= LOGIT_REL
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["REG_TINY", "REG_16"])
def test_pooled_heads_pool_the_patch_tokens_only(engines, name):
    cfg, m = CONFIGS[name], model(name)
    D, NC = cfg.embed_dim, cfg.num_classes
    rng = np.random.default_rng(17)
    eng = engines(name, max_batch=4)
    try:
        for pool, cls_layers, operand in (("avg", (-1,), m["operand"]), ("avg_fcnorm", (), m["fcnorm"]), ("avg", (), m["operand"][:, D:])):
            F = operand.shape[1]
            w = (rng.standard_normal((NC, F)) / np.sqrt(F)).astype(np.float32) * np.float32(3)
            b = rng.standard_normal(NC).astype(np.float32)
            eng.set_head(w, b, cls_layers, pool)
            eng.forward(images(name, 4))
            ref = operand[:4] @ w.astype(np.float64).T + b
            err = rel_err(eng.logits(4), ref)
            print(f"{name} head pool={pool} cls_layers={cls_layers}: logits {err:.3e} of max |ref|")
            assert err <= LOGIT_REL, (pool, err)
            assert rel_err(eng.head_operand(4), operand[:4]) <= LOGIT_REL
    finally:
        eng.reset_head()


@pytest.mark.parametrize("hname,layers", [("linear", (-1,)), ("ms", None)])
@pytest.mark.parametrize("name", ["REG_SMALL", "REG_ODD"])
def test_dense_heads_read_the_patch_rows_only(engines, name, hname, layers):
    cfg, m, W = CONFIGS[name], model(name), weights(name)
    layers = tuple(range(cfg.depth)) if layers is None else (cfg.depth - 1,)
    D, R, CLASSES, n = cfg.embed_dim, cfg.num_register_tokens, 21, 5
    g = cfg.img_size // cfg.patch_size
    F = len(layers) * D
    rng = np.random.default_rng(F)
    w = (rng.standard_normal((CLASSES, F)) / np.sqrt(F)).astype(np.float32) * np.float32(3)
    b = rng.standard_normal(CLASSES).astype(np.float32)
    eng = engines(name, max_batch=4)
    try:
        eng.set_dense_head(w, b, layers, True)
        grid = eng.dense(images(name), "grid")
        assert grid.shape == (n, CLASSES, g, g) and eng.dense_row_bytes("grid") == CLASSES * g * g * 4
        rows = np.concatenate([model_rows(name, "patches", l, 1) for l in layers], axis=2)  # [n][P][K * D]
        ref = (rows @ w.astype(np.float64).T + b).transpose(0, 2, 1).reshape(n, CLASSES, g, g)
        err = rel_err(grid, ref)
        print(f"{name} dense {hname}: grid {err:.3e} of max |ref|")
        assert err <= LOGIT_REL, err
        for oh, ow in ((cfg.img_size, cfg.img_size), (37, 53)):
            lab = eng.dense(images(name), "labels", (oh, ow))
            want = np.stack([dense_head_model.labels(dense_head_model.grid_to_logits(grid[i]), g, oh, ow) for i in range(n)])
            assert lab.shape == (n, oh, ow) and np.array_equal(lab, want), (oh, ow, int((lab != want).sum()))
    finally:
        eng.reset_dense_head()


# ---- 4: the class-token attention output -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["REG_TINY", "REG_261"])
def test_cls_attention_rows_hold_all_tokens_in_stored_order(engines, name, dtype):
    cfg, n = CONFIGS[name], 5
    T, heads, hd = cfg.tokens, cfg.num_heads, cfg.embed_dim // cfg.num_heads
    ref = np.concatenate([cls_attention_ref(q, 1, T, heads, hd) for q in model(name)["qkv_last"]])
    eng = engines(name, max_batch=4, dtype=dtype)
    got = eng.cls_attention(images(name), "heads")
    mean = eng.cls_attention(images(name), "head_mean")
    assert got.shape == (n, heads, T) and mean.shape == (n, T)
    for p in (got, mean):
        assert np.isfinite(p).all()
        assert float(np.abs(p.astype(np.float64).sum(-1) - 1.0).max()) <= T * 2.0 ** -23  # over all T: registers included
    err, merr = float(np.abs(got - ref).max()), float(np.abs(mean - ref.mean(1)).max())
    print(f"cls attention {name} {dtype}: heads {err:.3e}, head_mean {merr:.3e}")
    assert err <= CLS_CAP[dtype] and merr <= CLS_CAP[dtype]
    pruned = engines(name, max_batch=4, dtype=dtype, prune_last_layer=True)
    assert same_bits(pruned.cls_attention(images(name), "heads"), got)
    d4 = B.DeviceArray.from_numpy(images(name, 4))
    assert same_bits(device_attention(eng, d4, 4, "heads"), got[:4])


# ---- 5: nothing changes a bit ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["REG_TINY", "REG_16"])
def test_lanes_pruning_graph_position_and_entry_change_no_bit(engines, name, dtype):
    cfg = CONFIGS[name]
    plain = engines(name, max_batch=8, dtype=dtype)
    base = images(name)
    idx = np.array([0, 1, 0, 3, 0])  # image 0 at places 0, 2 and 4 of a batch of 5
    imgs = base[idx]
    layers = tap_layers(cfg)
    outs = {"probs": lambda e, x: e.forward(x), "cls": lambda e, x: e.features(x, "cls"), "mean": lambda e, x: e.features(x, "mean"),
            "tokens": lambda e, x: e.features(x, "tokens"), "map": lambda e, x: e.intermediate(x, layers, "map", True),
            "patches": lambda e, x: e.intermediate(x, layers, "patches", False)}
    want = {k: f(plain, imgs) for k, f in outs.items()}
    assert all(np.isfinite(v).all() for v in want.values())
    alone = {k: f(plain, base[:1]) for k, f in outs.items()}
    for place in (0, 2, 4):
        for k in outs:
            assert same_bits(want[k][place:place + 1], alone[k]), (k, place)
    try:
        plain.set_lanes(2)
        for k, f in outs.items():
            assert same_bits(f(plain, imgs), want[k]), k
    finally:
        plain.set_lanes(1)
    pruned = engines(name, max_batch=8, dtype=dtype, prune_last_layer=True)
    for k, f in outs.items():
        assert same_bits(f(pruned, imgs), want[k]), k
    # the device entry against the host entry, eager and as a replayed graph
    d5 = B.DeviceArray.from_numpy(imgs)
    dev, label, prob = device_forward(plain, d5, 5)
    assert same_bits(dev, want["probs"]) and (label == want["probs"].argmax(1)).all() and same_bits(prob, want["probs"].max(1))
    assert same_bits(device_features(plain, d5, 5, "mean"), want["mean"])
    assert same_bits(device_features(plain, d5, 5, "tokens"), want["tokens"])
    graph = engines(name, max_batch=8, dtype=dtype, use_graph=True)
    first = device_forward(graph, d5, 5)[0]
    second = device_forward(graph, d5, 5)[0]  # the replay
    assert same_bits(first, want["probs"]) and same_bits(second, want["probs"])
    gfeat = device_features(graph, d5, 5, "mean")
    assert same_bits(gfeat, want["mean"]) and same_bits(device_features(graph, d5, 5, "mean"), want["mean"])
    # 8-bit pixels and decoded images of the model's own size: the _u8 and _images entries against the fp32 entry on the same values
    rng = np.random.default_rng(5)
    S = cfg.img_size
    u8 = rng.integers(0, 256, (3, S, S, cfg.in_chans), dtype=np.uint8)
    f32 = B.images_u8_to_f32(u8)
    assert same_bits(plain.forward_u8(u8), plain.forward(f32))
    assert same_bits(plain.features_u8(u8, "mean"), plain.features(f32, "mean"))
    assert same_bits(plain.intermediate_u8(u8, layers, "map", True), plain.intermediate(f32, layers, "map", True))
    assert same_bits(plain.forward_images([im for im in u8], S, *CONSTS), plain.forward(f32))


# ---- 6: a checkpoint of another input size ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_position_embedding_of_another_grid_is_resampled_around_the_registers(dtype):
    """A [(4 * 4 + 1)][D] position embedding (a 56-pixel checkpoint) loaded into REG_TINY (g = 2): tensor 3 has no register rows, so
    the resampling is that of a model without; tensor 0, the prefix, arrives as it is."""
    cfg = register_model.REG_TINY
    D = cfg.embed_dim
    W = list(weights("REG_TINY"))
    W[3] = synth.round6(synth.uniform(W_SEED, 3, 17 * D, -0.087, 0.087)).reshape(17, D)
    eng = B.Engine(cfg, max_batch=4, dtype=dtype)
    try:
        eng.load_weights(W, pos_from=56, pos_mode="bicubic")
        back = eng.read_weight_image().tensors()
        want = B.pos_resample(W[3], 2, "bicubic")
        assert same_bits(back[3].reshape(5, D), want) and same_bits(back[0].reshape(5, D), W[0])
        imgs = images("REG_TINY")
        ref = register_model.forward(cfg, imgs, W[:3] + [want] + W[4:])
        probs = eng.forward(imgs)
        err = float(np.abs(probs - ref["probs"]).max())
        rerr = rel_err(eng.features(imgs, "tokens"), ref["norm"])
        print(f"resampled {dtype}: max |dprob| = {err:.3e}, tokens {rerr:.3e} of max |ref|")
        assert err <= (PROB_TOL if dtype == "f32" else BF16_PROB_TOL) and rerr <= ROW_BAR[dtype]
        # device to device, between engines of the same R at two input sizes
        big = B.Engine(synth.ModelConfig(**{**cfg.__dict__, "img_size": 56}), max_batch=2, dtype=dtype)
        try:
            big.load_weights(W)
            eng.copy_weights_from(big, "bicubic")
            assert same_bits(eng.forward(imgs), probs)
        finally:
            big.close()
    finally:
        eng.close()


# ---- 7: refusals -----------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_engine_usable(engines):
    name = "REG_TINY"
    cfg, W = CONFIGS[name], weights(name)
    D = cfg.embed_dim
    eng = engines(name, max_batch=4)
    want = eng.forward(images(name, 3))
    # tensor 0 of another size: the class token alone, a prefix of another R
    for bad in (W[0][0], np.concatenate([W[0], W[0][:1]])):
        with pytest.raises(B.VitError) as err:
            eng.load_weights([np.ascontiguousarray(bad)] + W[1:])
        assert err.value.code == ERR_WEIGHTS and "weight 0" in str(err.value) and f"expected {5 * D}" in str(err.value), str(err.value)
    # a position embedding with rows for the registers is no tensor 3 of this model
    with pytest.raises(B.VitError) as err:
        eng.load_weights(W[:3] + [np.zeros((cfg.tokens, D), np.float32)] + W[4:])
    assert err.value.code == ERR_WEIGHTS and "weight 3" in str(err.value), str(err.value)
    assert same_bits(eng.forward(images(name, 3)), want)
    # copy_weights between different R
    other_cfg = synth.ModelConfig(**{**cfg.__dict__, "num_register_tokens": 1})
    other = B.Engine(other_cfg, max_batch=4)
    try:
        other.load_weights(synth.make_weights(other_cfg, W_SEED))
        before = other.forward(images(name, 3))
        for mode in (None, "bicubic"):
            with pytest.raises(B.VitError) as err:
                other.copy_weights_from(eng, mode)
            assert err.value.code == ERR_ARG, str(err.value)
            with pytest.raises(B.VitError):
                eng.copy_weights_from(other, mode)
        assert same_bits(other.forward(images(name, 3)), before) and same_bits(eng.forward(images(name, 3)), want)
    finally:
        other.close()
    # R = 17
    with pytest.raises(B.VitError) as err:
        B.Engine(synth.ModelConfig(**{**cfg.__dict__, "num_register_tokens": 17}), max_batch=2)
    assert "register tokens" in str(err.value) and "bits 24..30" in str(err.value), str(err.value)
    assert same_bits(eng.forward(images(name, 3)), want)
