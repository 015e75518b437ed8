"""Engines loaded as CLIP image towers -- VIT_MLP_QUICKGELU, vit_engine_set_layernorm_eps(1e-5), vit_engine_set_pre_norm and the
projected embedding as features("head") -- against tests/clip_model.py, which tests/test_clip_model.py pins to transformers'
CLIPVisionModelWithProjection.  Two reduced towers (tiny: D 128, depth 2, 32 / 8, projection 64; small: D 256, depth 3, 56 / 14,
projection 96 -- the general patch embedding and the chunk loop), both with a pre-norm far from (1, 0), and one layer at the full width
of CLIP ViT-L/14.

Bars: fp32 probabilities 1e-4 (PROB_TOL) with the same top-1 -- the softmax over a projection means nothing for CLIP, but it is the
engine's oldest yardstick and still runs --, logits (= the embedding) and per-layer residual streams 1e-3 of max |ref| (LOGIT_REL), the
L2-normalised embedding 1e-3 of max |ref|; bf16 probabilities 2e-2 (tests/test_gpu_bf16.py) with the same top-1 where the margin exceeds
that.  For the bf16 L2-normalised embedding the project has no bar: the same quantity is measured on the GELU twin of the same
dimensions (same weights, VIT_MLP_GELU, no pre-norm, eps 1e-6, against its own model -- an engine the parent commit already runs) and
the CLIP tower may take 2 x that.  Everything the engine promises to keep bit-identical is compared bitwise.
Measured on an MI355X: profiles/r19/clip.md.
"""
import dataclasses

import numpy as np
import pytest

import clip_model
from clip_model import L14_LAYER, SMALL_CLIP, TINY_CLIP
from engine_helpers import device_features, device_forward, same_bits
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

PROB_TOL, LOGIT_REL, BF16_PROB_TOL = 1e-4, 1e-3, 2e-2
VIT_ERR_ARG, VIT_ERR_STATE = 1, 5
CONFIGS = {"tiny": TINY_CLIP, "small": SMALL_CLIP, "l14_layer": L14_LAYER}
SEED, EPS = 23, 1e-5
_cache = {}


def rel_err(got, ref) -> float:
    return float(np.abs(got - ref).max()) / float(np.abs(ref).max())


def weights(name):
    if ("w", name) not in _cache:
        _cache[("w", name)] = synth.make_weights(CONFIGS[name], SEED)
    return _cache[("w", name)]


def pre_norm(name):
    """gamma in (0.3, 2.0), beta in (-0.7, 0.7): far from the identity."""
    D = CONFIGS[name].embed_dim
    return synth.uniform(SEED, 9001, D, 0.3, 2.0), synth.uniform(SEED, 9002, D, -0.7, 0.7)


def model_run(name, n, **kw):
    """images and tests/clip_model.py's outputs for them, computed once per (model, n, variant)."""
    key = ("model", name, n, tuple(sorted(kw.items())))
    if key not in _cache:
        cfg = CONFIGS[name]
        imgs = synth.make_images(cfg, n, 100 + n)
        args = dict(pre=pre_norm(name), eps=EPS, act="quickgelu")
        args.update(kw)
        _cache[key] = (imgs, clip_model.forward(cfg, imgs, weights(name), **args))
    return _cache[key]


def clip_engine(name, **opt):
    """The documented loading order: epsilon (architecture), weights, pre-norm (every install removes it)."""
    eng = B.Engine(CONFIGS[name], **opt)
    eng.set_layernorm_eps(EPS)
    eng.load_weights(weights(name))
    eng.set_pre_norm(*pre_norm(name))
    return eng


@pytest.fixture(scope="module")
def engines():
    cache = {}

    def get(name, **opt):
        key = (name, tuple(sorted(opt.items())))
        if key not in cache:
            cache[key] = clip_engine(name, **opt)
        return cache[key]

    yield get
    for eng in cache.values():
        eng.close()


# ---- fp32 against the model ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fp32_split", [0, -1], ids=["split", "fp32-mfma"])
@pytest.mark.parametrize("ln_fold", [0, -1], ids=["ln-folded", "ln-kernels"])
@pytest.mark.parametrize("name", ["tiny", "small"])
def test_fp32_probabilities_embeddings_and_stages_match_the_model(engines, name, ln_fold, fp32_split):
    cfg = CONFIGS[name]
    eng = engines(name, max_batch=4, ln_fold=ln_fold, fp32_split=fp32_split)
    layers = list(range(cfg.depth))
    for n in (1, 3, 5):   # one chunk, a ragged one, the chunk loop
        imgs, ref = model_run(name, n)
        probs = eng.forward(imgs)
        err = float(np.abs(probs - ref["probs"]).max())
        last = n % 4 or 4  # the logits tap holds the last chunk
        lerr = rel_err(eng.logits(last), ref["embeds"][-last:])
        got = eng.intermediate(imgs, layers, "tokens", 0)   # [n][depth][T][D]: the residual stream behind every layer
        serr = max(rel_err(got[:, l], ref["stages"][:, l + 1]) for l in layers)
        head = eng.features(imgs, "head")
        assert head.shape == (n, cfg.num_classes) == eng.feature_shape(n, "head")
        assert same_bits(head[-last:], eng.logits(last))                       # without L2: the bits of read_logits
        unit = eng.features(imgs, "head", True)
        assert same_bits(eng.logits(last), head[-last:])                       # ... which keeps the un-normalised rows
        assert same_bits(unit, B.l2_normalize_rows(head))                      # with L2: the bits of the L2 kernel on them
        uerr = rel_err(unit, ref["unit"])
        print(f"fp32 {name} n={n} ln_fold={ln_fold} fp32_split={fp32_split}: max |dprob| = {err:.3e}, embedding {lerr:.3e}, "
              f"worst stage {serr:.3e}, unit embedding {uerr:.3e}")
        assert err <= PROB_TOL and (probs.argmax(1) == ref["probs"].argmax(1)).all(), (n, err)
        assert lerr <= LOGIT_REL and serr <= LOGIT_REL and uerr <= LOGIT_REL, (n, lerr, serr, uerr)


def test_each_piece_is_really_in_the_engine(engines):
    """The engine's answer moves by far more than the bar when a piece is taken away, and the model without that piece follows it."""
    name, n = "small", 3
    eng = clip_engine(name, max_batch=4)
    try:
        imgs, ref = model_run(name, n)
        full = eng.features(imgs, "head")
        eng.set_pre_norm(None, None)
        no_pre = eng.features(imgs, "head")
        assert rel_err(no_pre, ref["embeds"]) > 10 * LOGIT_REL
        assert rel_err(no_pre, model_run(name, n, pre=None)[1]["embeds"]) <= LOGIT_REL
        eng.set_pre_norm(*pre_norm(name))
        assert same_bits(eng.features(imgs, "head"), full)
        # epsilon: pixels and the additive tensors (cls, conv bias, pos) scaled until the rows the pre-norm sees have variances near
        # 1e-5, where the model itself tells 1e-5 from 1e-6 by far more than the bar
        tiny_imgs = (imgs * np.float32(4e-3)).astype(np.float32)
        Ws = list(weights(name))
        for i in (0, 2, 3):
            Ws[i] = (Ws[i] * np.float32(0.05)).astype(np.float32)
        want5 = clip_model.forward(CONFIGS[name], tiny_imgs, Ws, pre_norm(name), 1e-5)["embeds"]
        want6 = clip_model.forward(CONFIGS[name], tiny_imgs, Ws, pre_norm(name), 1e-6)["embeds"]
        assert rel_err(want6, want5) > 10 * LOGIT_REL
        eng.load_weights(Ws)
        eng.set_pre_norm(*pre_norm(name))
        got5 = eng.features(tiny_imgs, "head")
        eng.set_layernorm_eps(1e-6)
        got6 = eng.features(tiny_imgs, "head")
        print(f"eps sensitivity: model 1e-5 vs 1e-6 {rel_err(want6, want5):.3e}; engine vs model {rel_err(got5, want5):.3e} / {rel_err(got6, want6):.3e}")
        assert rel_err(got5, want5) <= LOGIT_REL and rel_err(got6, want6) <= LOGIT_REL
    finally:
        eng.close()
    twin = B.Engine(dataclasses.replace(CONFIGS[name], mlp="gelu"), max_batch=4)
    try:
        twin.set_layernorm_eps(EPS)
        twin.load_weights(weights(name))
        twin.set_pre_norm(*pre_norm(name))
        gelu = twin.features(imgs, "head")
        assert rel_err(gelu, ref["embeds"]) > LOGIT_REL          # (erf-GELU and QuickGELU are close cousins: 1.7e-3 on this tower)
        assert rel_err(gelu, model_run(name, n, act="gelu")[1]["embeds"]) <= LOGIT_REL       # OpenCLIP towers trained with plain GELU
    finally:
        twin.close()


# ---- bitwise identities ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["tiny", "small"])
def test_lanes_graph_pruning_entry_position_and_copy_change_no_bit(engines, name, dtype):
    cfg = CONFIGS[name]
    plain = engines(name, max_batch=8, dtype=dtype)
    base = synth.make_images(cfg, 4, 301)
    idx = np.array([0, 1, 2, 3, 3, 0, 2, 1, 1, 3, 0])   # 11 images: chunks of 8 and 3, every image at several places
    imgs = base[idx]
    want, head, unit = plain.forward(imgs), plain.features(imgs, "head"), plain.features(imgs, "head", True)
    assert np.isfinite(want).all() and np.isfinite(head).all()
    for k in range(4):   # a copy of one image at every batch position
        assert (want[idx == k] == want[idx == k][0]).all() and (head[idx == k] == head[idx == k][0]).all(), k
    # the device entry against the host entry
    d8 = B.DeviceArray.from_numpy(imgs[:8])
    dev, label, prob = device_forward(plain, d8, 8)
    assert same_bits(dev, want[:8]) and (label == want[:8].argmax(1)).all() and same_bits(prob, want[:8].max(1))
    assert same_bits(device_features(plain, d8, 8, "head"), head[:8]) and same_bits(device_features(plain, d8, 8, "head", True), unit[:8])
    try:
        plain.set_lanes(2)
        assert same_bits(plain.forward(imgs), want) and same_bits(plain.features(imgs, "head"), head)
    finally:
        plain.set_lanes(1)
    graph = engines(name, max_batch=8, dtype=dtype, use_graph=True)
    first = device_forward(graph, d8, 8)[0]
    second = device_forward(graph, d8, 8)[0]   # the replay
    assert same_bits(first, want[:8]) and same_bits(second, want[:8])
    d_out = B.DeviceArray((8, cfg.num_classes))
    for _ in range(2):   # the graph is keyed on the kind: the same n and pointers, another output
        assert same_bits(device_features(graph, d8, 8, "head", d_out=d_out), head[:8])
    assert same_bits(device_features(graph, d8, 8, "head", True, d_out=d_out), unit[:8])
    assert same_bits(device_forward(graph, d8, 8)[0], want[:8])
    pruned = engines(name, max_batch=8, dtype=dtype, prune_last_layer=True)
    assert same_bits(pruned.forward(imgs), want) and same_bits(pruned.features(imgs, "head"), head)
    copy = B.Engine(cfg, max_batch=8, dtype=dtype)
    try:
        copy.set_layernorm_eps(EPS)              # neither is carried by the copy calls
        copy.copy_weights_from(plain)
        assert not same_bits(copy.forward(imgs), want)
        copy.set_pre_norm(*pre_norm(name))
        assert same_bits(copy.forward(imgs), want) and same_bits(copy.features(imgs, "head", True), unit)
    finally:
        copy.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_eight_bit_input(engines, dtype):
    cfg = SMALL_CLIP
    eng = engines("small", max_batch=4, dtype=dtype)
    rng = np.random.default_rng(5)
    u8 = rng.integers(0, 256, (5, cfg.img_size, cfg.img_size, cfg.in_chans), dtype=np.uint8)
    f32 = B.images_u8_to_f32(u8)
    assert same_bits(eng.forward_u8(u8), eng.forward(f32))
    assert same_bits(eng.features_u8(u8, "head"), eng.features(f32, "head"))
    assert same_bits(eng.features_u8(u8, "head", True), eng.features(f32, "head", True))


# ---- the state rules -------------------------------------------------------------------------------------------------------------

def test_installs_remove_the_pre_norm_and_keep_the_epsilon_and_refusals_change_nothing():
    name = "tiny"
    cfg, W = CONFIGS[name], weights(name)
    imgs = synth.make_images(cfg, 3, 77)
    L = B.lib()
    eng = B.Engine(cfg, max_batch=4)
    never = B.Engine(cfg, max_batch=4)
    try:
        assert eng.get_layernorm_eps() == 1e-6                                  # the double, exactly
        with pytest.raises(B.VitError) as err:                                   # before any weights
            eng.set_pre_norm(*pre_norm(name))
        assert err.value.code == VIT_ERR_STATE
        eng.set_layernorm_eps(EPS)                                               # architecture: allowed before weights
        never.set_layernorm_eps(EPS)
        never.load_weights(W)
        bare = never.forward(imgs)
        eng.load_weights(W)
        assert eng.get_layernorm_eps() == EPS and same_bits(eng.forward(imgs), bare)
        eng.set_pre_norm(*pre_norm(name))
        with_pre = eng.forward(imgs)
        assert not same_bits(with_pre, bare)
        # every refusal leaves the previous state in force and the engine usable
        g, b = pre_norm(name)
        L.vit_engine_set_pre_norm.argtypes = [B.C.c_void_p, B.C.c_void_p, B.C.c_void_p]
        L.vit_engine_set_layernorm_eps.argtypes = [B.C.c_void_p, B.C.c_double]
        assert L.vit_engine_set_pre_norm(eng._h, g.ctypes.data, None) == VIT_ERR_ARG
        assert L.vit_engine_set_pre_norm(eng._h, None, b.ctypes.data) == VIT_ERR_ARG
        for bad in (0.0, -1e-5, float("nan"), float("inf")):
            assert L.vit_engine_set_layernorm_eps(eng._h, bad) == VIT_ERR_ARG, bad
        with pytest.raises(B.VitError):
            eng.features(imgs, 3)                                                # an unknown feature kind (3 is unassigned)
        with pytest.raises(B.VitError):
            eng.features(imgs, 5)
        with pytest.raises(B.VitError):
            eng.features(imgs, "tokens", True)
        assert eng.get_layernorm_eps() == EPS and same_bits(eng.forward(imgs), with_pre)
        # a weight install removes the pre-norm -- the outputs of an engine that never had one, bit for bit -- and keeps the epsilon
        eng.load_weights(W)
        assert eng.get_layernorm_eps() == EPS and same_bits(eng.forward(imgs), bare)
        eng.set_pre_norm(*pre_norm(name))
        assert same_bits(eng.forward(imgs), with_pre)
        eng.load_weight_image(B.WeightImage.build(cfg, W))
        assert same_bits(eng.forward(imgs), bare)
        eng.set_pre_norm(*pre_norm(name))
        eng.copy_weights_from(never)
        assert same_bits(eng.forward(imgs), bare)
        eng.set_pre_norm(*pre_norm(name))
        eng.set_pre_norm(None, None)                                             # and so does NULL, NULL
        assert same_bits(eng.forward(imgs), bare)
        # the epsilon is every LayerNorm's: back at the default the engine is the one it always was
        eng.set_layernorm_eps(1e-6)
        plain = B.Engine(cfg, max_batch=4)
        try:
            plain.load_weights(W)
            assert same_bits(eng.forward(imgs), plain.forward(imgs)) and same_bits(eng.features(imgs, "mean"), plain.features(imgs, "mean"))
        finally:
            plain.close()
    finally:
        eng.close()
        never.close()


def test_a_callers_head_is_honoured_by_head_features(engines):
    name = "small"
    cfg = CONFIGS[name]
    eng = clip_engine(name, max_batch=4)
    try:
        imgs, ref = model_run(name, 3)
        own = eng.features(imgs, "head")
        Wh = synth.uniform(SEED, 9100, cfg.num_classes * 2 * cfg.embed_dim, -0.2, 0.2).reshape(cfg.num_classes, 2 * cfg.embed_dim)
        bh = synth.uniform(SEED, 9101, cfg.num_classes, -0.1, 0.1)
        eng.set_head(Wh, bh, cls_layers=(-1,), pool="avg")
        got = eng.features(imgs, "head")
        assert same_bits(got, eng.logits(3)) and not same_bits(got, own)
        y = np.stack([clip_model.layer_norm(st[-1], weights(name)[-4], weights(name)[-3], EPS) for st in ref["stages"]])
        operand = np.concatenate([y[:, 0], y[:, 1:].mean(1)], axis=1)
        assert rel_err(got, operand @ Wh.astype(np.float64).T + bh) <= LOGIT_REL
        eng.reset_head()
        assert same_bits(eng.features(imgs, "head"), own)
    finally:
        eng.close()


def test_a_transformers_tower_maps_through_the_table_to_the_engine():
    """The tiny random CLIPVisionModelWithProjection of tests/test_clip_model.py, mapped by clip_model.from_transformers (INTEGRATION.md's
    table) and loaded with set_layernorm_eps, load_weights, set_pre_norm: features("head", l2) is image_embeds / ||image_embeds|| and
    the penultimate residual stream is hidden_states[-2], within LOGIT_REL of max |ref|."""
    from test_clip_model import hf_run, make_tower
    torch, model, images = make_tower()
    cfg, W, pre, eps = clip_model.from_transformers(model)
    ref_e, ref_h = hf_run(torch, model, images)
    unit = ref_e / np.linalg.norm(ref_e, axis=1, keepdims=True)
    for dtype in ("f32", "bf16"):
        eng = B.Engine(cfg, max_batch=4, dtype=dtype)
        try:
            eng.set_layernorm_eps(eps)
            eng.load_weights(W)
            eng.set_pre_norm(*pre)
            x = images.numpy()
            got = eng.features(x, "head", True)
            hid = eng.intermediate(x, [cfg.depth - 2], "tokens", 0)[:, 0]
            uerr, herr = rel_err(got, unit), rel_err(hid, ref_h)
            print(f"transformers tower, {dtype}: unit image_embeds {uerr:.3e}, hidden_states[-2] {herr:.3e} of max |ref|")
            if dtype == "f32":
                assert uerr <= LOGIT_REL and herr <= LOGIT_REL
                assert rel_err(eng.features(x, "head"), ref_e) <= LOGIT_REL
        finally:
            eng.close()


# ---- bf16 ------------------------------------------------------------------------------------------------------------------------

def check_bf16_probs(probs, ref, what):
    err = float(np.abs(probs - ref).max())
    assert err <= BF16_PROB_TOL, (what, err)
    top2 = np.sort(ref, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > BF16_PROB_TOL
    assert (probs.argmax(1) == ref.argmax(1))[clear].all(), what
    return err


@pytest.mark.parametrize("ln_fold", [0, -1], ids=["ln-folded", "ln-kernels"])
@pytest.mark.parametrize("name", ["tiny", "small"])
def test_bf16_probabilities_and_the_unit_embedding_against_the_gelu_twin(engines, name, ln_fold):
    cfg, n = CONFIGS[name], 6
    imgs, ref = model_run(name, n)
    eng = engines(name, max_batch=4, dtype="bf16", ln_fold=ln_fold)
    perr = check_bf16_probs(eng.forward(imgs), ref["probs"], f"{name} ln_fold={ln_fold}")
    uerr = float(np.abs(eng.features(imgs, "head", True) - ref["unit"]).max())
    # the twin: the same weights as a GELU model without pre-norm at eps 1e-6, against its own model
    twin_cfg = dataclasses.replace(cfg, mlp="gelu")
    twin_ref = model_run(name, n, pre=None, eps=1e-6, act="gelu")[1]
    twin = B.Engine(twin_cfg, max_batch=4, dtype="bf16", ln_fold=ln_fold)
    try:
        twin.load_weights(weights(name))
        terr = float(np.abs(twin.features(imgs, "head", True) - twin_ref["unit"]).max())
    finally:
        twin.close()
    print(f"bf16 {name} ln_fold={ln_fold}: max |dprob| {perr:.3e}; unit embedding max |d| CLIP {uerr:.3e}, GELU twin {terr:.3e}")
    assert uerr <= 2.0 * terr, (uerr, terr)


# ---- one layer at the full width of CLIP ViT-L/14 ---------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_one_layer_at_clip_l14_width(dtype):
    """embed 1024, 16 heads, hidden 4096, patch 14, projection 768: the real widths through the real tile shapes."""
    name, n = "l14_layer", 2
    imgs, ref = model_run(name, n)
    eng = clip_engine(name, max_batch=n, dtype=dtype)
    try:
        probs = eng.forward(imgs)
        if dtype == "bf16":
            check_bf16_probs(probs, ref["probs"], "l14 layer")
            return
        err, lerr = float(np.abs(probs - ref["probs"]).max()), rel_err(eng.features(imgs, "head"), ref["embeds"])
        serr = rel_err(eng.intermediate(imgs, [0], "tokens", 0)[:, 0], ref["stages"][:, 1])
        print(f"fp32 l14 layer: max |dprob| = {err:.3e}, embedding {lerr:.3e}, stage {serr:.3e}")
        assert err <= PROB_TOL and (probs.argmax(1) == ref["probs"].argmax(1)).all()
        assert lerr <= LOGIT_REL and serr <= LOGIT_REL
    finally:
        eng.close()
