"""Engines loaded as BEiT backbones (a bias per layer from binding.rel_pos_bias, epsilon 1e-12, LayerScale folded, zero position embedding
and K bias) against transformers' BeitModel in float64 with eager attention: hidden 128, 2 heads, 2 layers, intermediate 256, 144 px /
patch 16 (T = 82), LayerScale in (0.3, 1.5), tables in U(-2, 2), mapped by network_from_state_dict (INTEGRATION.md's table).  Compared:
last_hidden_state.  fp32 bar: 1e-3 of max |ref| (LOGIT_REL of test_gpu_clip_engine.py).  bf16: the same engine with no bias against the model
with zeroed tables is code the parent commit runs; the biased engine may take 2 x that.  Measured: profiles/r37/attention_bias.md."""
import functools

import numpy as np
import pytest

from engine_helpers import device_features, same_bits
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu
LOGIT_REL, VIT_ERR_ARG, VIT_ERR_STATE = 1e-3, 1, 5
EPS, N, GRID = 1e-12, 5, 9
CFG = synth.ModelConfig(img_size=144, patch_size=16, num_classes=10, embed_dim=128, depth=2, num_heads=2, hidden_dim=256)


def rel_err(got, ref) -> float:
    return float(np.abs(got - ref).max()) / float(np.abs(ref).max())


def network_from_state_dict(cfg, sd):
    """INTEGRATION.md's table: (W in Network order, LayerScale folded; the biases [heads][T][T]).  The final LayerNorm slot is the identity."""
    D = cfg.embed_dim
    W = [sd["embeddings.cls_token"], sd["embeddings.patch_embeddings.projection.weight"], sd["embeddings.patch_embeddings.projection.bias"],
         np.zeros(cfg.tokens * D)]
    ls, biases = [], []
    for l in range(cfg.depth):
        p, a = f"layers.{l}.", f"layers.{l}.attention."
        W += [sd[p + "layernorm_before.weight"], sd[p + "layernorm_before.bias"],
              np.concatenate([sd[a + "q_proj.weight"], sd[a + "k_proj.weight"], sd[a + "v_proj.weight"]]),
              np.concatenate([sd[a + "q_proj.bias"], np.zeros(D), sd[a + "v_proj.bias"]]),
              sd[a + "o_proj.weight"], sd[a + "o_proj.bias"], sd[p + "layernorm_after.weight"], sd[p + "layernorm_after.bias"],
              sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"], sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"]]
        ls += [sd[p + "lambda_1"], sd[p + "lambda_2"]]
        biases.append(B.rel_pos_bias(sd[p + "relative_position_bias.relative_position_bias_table"], cfg.img_size // cfg.patch_size))
    W += [np.ones(D), np.zeros(D), np.zeros(cfg.num_classes * D), np.zeros(cfg.num_classes)]
    return B.fold_layer_scale(cfg, [np.ascontiguousarray(w, np.float32).reshape(s) for w, s in zip(W, cfg.weight_shapes())], ls), biases


@functools.lru_cache(None)
def reference():
    """Once: (W, biases, images, last_hidden_state, the same with zeroed tables, the model's own expanded bias of layer 0, ours)"""
    import torch
    import transformers
    model = transformers.BeitModel(transformers.BeitConfig(
        hidden_size=CFG.embed_dim, intermediate_size=CFG.hidden_dim, num_hidden_layers=CFG.depth, num_attention_heads=CFG.num_heads,
        image_size=CFG.img_size, patch_size=CFG.patch_size, use_relative_position_bias=True, use_absolute_position_embeddings=False,
        layer_scale_init_value=0.1, layer_norm_eps=EPS, attn_implementation="eager")).eval().double()
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for name, p in model.named_parameters():   # matrices of unit gain, so that Q . K is far from flat; the rest small
            u = torch.rand(p.shape, generator=gen, dtype=torch.float64)
            p.copy_((u * 4 - 2) if name.endswith("bias_table") else u * 1.2 + 0.3 if "lambda_" in name else u + 0.5 if "layernorm" in name and name.endswith("weight")
                    else (u * 2 - 1) * (1.5 / np.sqrt(p.shape[-1]) if p.ndim >= 2 and "embeddings" not in name else 0.1))
    imgs = synth.make_images(CFG, N, 43)

    def run():
        with torch.no_grad():
            return model(pixel_values=torch.from_numpy(imgs).double()).last_hidden_state.numpy()

    sd = {k: v.numpy() for k, v in model.state_dict().items()}
    W, biases = network_from_state_dict(CFG, sd)
    with torch.no_grad():
        own = model.layers[0].relative_position_bias((GRID, GRID))[0].numpy()
        with_bias = run()
        for layer in model.layers:
            layer.relative_position_bias.relative_position_bias_table.zero_()
        return W, biases, imgs, with_bias, run(), own, biases[0]


def beit_engine(bias=True, **opt):   # the documented loading order: epsilon and the biases (architecture), then the weights
    eng = B.Engine(CFG, **opt)
    eng.set_layernorm_eps(EPS)
    for l in range(CFG.depth if bias else 0):
        eng.set_attention_bias(l, reference()[1][l])
    eng.load_weights(reference()[0])
    return eng


def tokens(eng, imgs):
    return eng.intermediate(imgs, [CFG.depth - 1], "tokens", False)[:, 0]


def test_rel_pos_bias_is_the_models_own_expansion():
    own, ours = reference()[5:]
    assert ours.shape == (CFG.num_heads, 1 + GRID * GRID, 1 + GRID * GRID) and np.array_equal(ours, own.astype(np.float32))


@pytest.mark.parametrize("fp32_split", [0, -1], ids=["split", "fp32-mfma"])
@pytest.mark.parametrize("ln_fold", [0, -1], ids=["ln-folded", "ln-kernels"])
def test_fp32_tokens_match_transformers(ln_fold, fp32_split):
    W, biases, imgs, ref, flat = reference()[:5]
    eng = beit_engine(max_batch=4, ln_fold=ln_fold, fp32_split=fp32_split)
    try:
        want = tokens(eng, imgs)
        err = rel_err(want, ref)
        B.lib().vit_engine_set_attention_bias.argtypes = [B.C.c_void_p, B.C.c_int, B.C.c_void_p]
        for bad in (-2, CFG.depth):   # refused, and no bit of the next forward changes
            assert B.lib().vit_engine_set_attention_bias(eng._h, bad, biases[0].ctypes.data) == VIT_ERR_ARG and same_bits(tokens(eng, imgs), want)
        eng.load_weights(W)           # an install keeps the biases
        assert all(eng.has_attention_bias(l) for l in range(CFG.depth)) and same_bits(tokens(eng, imgs), want)
        with pytest.raises(B.VitError) as refused:   # the class-attention kernel takes no bias: no wrong row
            eng.cls_attention(imgs, "heads")
        assert refused.value.code == VIT_ERR_STATE
        for l in range(CFG.depth):    # the piece is really there: without it the engine follows the model without it
            eng.set_attention_bias(l, None)
        off = tokens(eng, imgs)
        print(f"fp32 ln_fold={ln_fold} fp32_split={fp32_split}: tokens {err:.3e} of max |ref|; bias removed: {rel_err(off, ref):.3e}, from the model with zeroed tables {rel_err(off, flat):.3e}")
        assert err <= LOGIT_REL
        assert not any(eng.has_attention_bias(l) for l in range(-1, CFG.depth)) and eng.cls_attention(imgs, "heads").shape == (N, 2, CFG.tokens)
        assert rel_err(off, ref) > 10 * LOGIT_REL and rel_err(off, flat) <= LOGIT_REL
    finally:
        eng.close()


@pytest.mark.parametrize("ln_fold", [0, -1], ids=["ln-folded", "ln-kernels"])
def test_bf16_tokens_stay_within_twice_the_error_of_the_engine_without_bias(ln_fold):
    _, _, imgs, ref, flat = reference()[:5]
    eng, plain = beit_engine(max_batch=8, dtype="bf16", ln_fold=ln_fold), beit_engine(False, max_batch=8, dtype="bf16", ln_fold=ln_fold)
    try:
        err, base = rel_err(tokens(eng, imgs), ref), rel_err(tokens(plain, imgs), flat)
    finally:
        eng.close(), plain.close()
    print(f"bf16 ln_fold={ln_fold}: tokens {err:.3e} of max |ref| with the bias, {base:.3e} without")
    assert err <= 2.0 * base, (err, base)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_pruning_lanes_batch_position_sharing_and_graph_replay_change_no_bit(dtype):
    biases, imgs = reference()[1:3]
    idx = np.array([0, 1, 2, 3, 3, 0, 2, 1, 4, 3, 0])   # chunks of 8 and 3, every image at several places
    batch = imgs[idx]
    plain, pruned, graph = (beit_engine(max_batch=8, dtype=dtype, **o) for o in ({}, {"prune_last_layer": True}, {"use_graph": True}))
    try:
        def outputs(eng):
            return eng.features(batch, "cls"), tokens(eng, batch), eng.forward(batch)

        want = outputs(plain)
        assert all(np.isfinite(w).all() for w in want)
        for k in range(N):
            assert all((w[idx == k] == w[idx == k][0]).all() for w in want), k
        assert all(same_bits(g, w) for g, w in zip(outputs(pruned), want))
        plain.set_lanes(2)
        assert all(same_bits(g, w) for g, w in zip(outputs(plain), want))
        d8, d_out = B.DeviceArray.from_numpy(batch[:8]), B.DeviceArray((8, CFG.embed_dim))
        for last in (1, 1, 1, 0, 1):   # the capture, two replays, and no graph outlives a change of the setting
            if graph.has_attention_bias(CFG.depth - 1) != bool(last):
                graph.set_attention_bias(CFG.depth - 1, biases[-1] if last else None)
            assert same_bits(device_features(graph, d8, 8, "cls", d_out=d_out), want[0][:8]) == bool(last), last
        plain.set_attention_bias(-1, biases[0])   # one array for every layer is the same array set layer by layer
        shared = outputs(plain)
        assert plain.has_attention_bias(-1) and all(plain.has_attention_bias(l) for l in range(CFG.depth))
        plain.set_attention_bias(-1, None)
        for l in range(CFG.depth):
            plain.set_attention_bias(l, biases[0])
        assert not plain.has_attention_bias(-1) and all(same_bits(g, w) for g, w in zip(outputs(plain), shared)) and not same_bits(shared[1], want[1])
    finally:
        for eng in (plain, pruned, graph):
            eng.close()
