"""Engines loaded as DINOv3 backbones (vit_engine_set_rope(100), epsilon 1e-5, 4 registers, LayerScale folded, zero position embedding
and K bias) against transformers' DINOv3ViTModel in float64 with eager attention: tiny and random -- hidden 128, 2 heads, 2 layers,
intermediate 256, 32 px / patch 8, LayerScale in (0.3, 1.5) --, mapped by network_from_state_dict below (INTEGRATION.md's table).
Bars: fp32 tokens and class features 1e-3 of max |ref| (LOGIT_REL of tests/test_gpu_clip_engine.py), class-attention rows 1e-4 (PROB_TOL).
bf16 token streams have no bar here: the same bf16 engine with the rotation off is measured against the same model with cos = 1,
sin = 0 -- code the parent commit runs -- and the DINOv3 engine may take 2 x that (one more bf16 rounding of Q and K per layer).
Measured on an MI355X: profiles/r36/rope.md."""
import functools

import numpy as np
import pytest

from engine_helpers import device_features, same_bits
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu
LOGIT_REL, PROB_TOL, VIT_ERR_ARG = 1e-3, 1e-4, 1
THETA, EPS, N = 100.0, 1e-5, 5
CFG = synth.ModelConfig(img_size=32, patch_size=8, num_classes=10, embed_dim=128, depth=2, num_heads=2, hidden_dim=256, num_register_tokens=4)


def rel_err(got, ref) -> float:
    return float(np.abs(got - ref).max()) / float(np.abs(ref).max())


def network_from_state_dict(cfg, sd):
    """INTEGRATION.md's table for DINOv3ViTModel: W in Network order, LayerScale folded; position embedding, K bias and head are zero."""
    D = cfg.embed_dim
    W = [np.concatenate([sd["embeddings.cls_token"].reshape(1, D), sd["embeddings.register_tokens"].reshape(-1, D)]),
         sd["embeddings.patch_embeddings.weight"], sd["embeddings.patch_embeddings.bias"], np.zeros((cfg.patches + 1) * D)]
    ls = []
    for l in range(cfg.depth):
        p, a = f"model.layer.{l}.", f"model.layer.{l}.attention."
        W += [sd[p + "norm1.weight"], sd[p + "norm1.bias"],
              np.concatenate([sd[a + "q_proj.weight"], sd[a + "k_proj.weight"], sd[a + "v_proj.weight"]]),
              np.concatenate([sd[a + "q_proj.bias"], np.zeros(D), sd[a + "v_proj.bias"]]),
              sd[a + "o_proj.weight"], sd[a + "o_proj.bias"], sd[p + "norm2.weight"], sd[p + "norm2.bias"],
              sd[p + "mlp.up_proj.weight"], sd[p + "mlp.up_proj.bias"], sd[p + "mlp.down_proj.weight"], sd[p + "mlp.down_proj.bias"]]
        ls += [sd[p + "layer_scale1.lambda1"], sd[p + "layer_scale2.lambda1"]]
    W += [sd["norm.weight"], sd["norm.bias"], np.zeros(cfg.num_classes * D), np.zeros(cfg.num_classes)]
    return B.fold_layer_scale(cfg, [np.ascontiguousarray(w, np.float32).reshape(s) for w, s in zip(W, cfg.weight_shapes())], ls)


@functools.lru_cache(None)
def reference():
    """(W, images, outputs of the float64 model, outputs of the same model with cos = 1 and sin = 0), computed once."""
    import torch
    import transformers
    model = transformers.DINOv3ViTModel(transformers.DINOv3ViTConfig(
        hidden_size=CFG.embed_dim, intermediate_size=CFG.hidden_dim, num_hidden_layers=CFG.depth, num_attention_heads=CFG.num_heads,
        image_size=CFG.img_size, patch_size=CFG.patch_size, num_register_tokens=CFG.num_register_tokens, rope_theta=THETA,
        layer_norm_eps=EPS, hidden_act="gelu", attn_implementation="eager")).eval().double()
    gen = torch.Generator().manual_seed(3)
    with torch.no_grad():
        for name, p in model.named_parameters():   # matrices of unit gain, so that Q . K is far from flat; the rest small
            u = torch.rand(p.shape, generator=gen, dtype=torch.float64)
            p.copy_(u * 1.2 + 0.3 if name.endswith("lambda1") else u + 0.5 if "norm" in name and name.endswith("weight") else
                    (u * 2 - 1) * (1.5 / np.sqrt(p.shape[-1]) if p.ndim >= 2 and "embeddings" not in name else 0.1))
    imgs = synth.make_images(CFG, N, 41)

    def run():
        with torch.no_grad():
            o = model(pixel_values=torch.from_numpy(imgs).double(), output_attentions=True)
        return {"tokens": o.last_hidden_state.numpy(), "cls": o.pooler_output.numpy(), "attn": o.attentions[-1][:, :, 0, :].numpy()}

    with_rope, ones = run(), torch.ones(CFG.patches, CFG.embed_dim // CFG.num_heads, dtype=torch.float64)
    model.rope_embeddings.forward = lambda pixel_values: (ones, 0 * ones)
    return network_from_state_dict(CFG, {k: v.numpy() for k, v in model.state_dict().items()}), imgs, with_rope, run()


def dinov3_engine(**opt):   # the documented loading order: epsilon and rotation (architecture), then the weights
    eng = B.Engine(CFG, **opt)
    eng.set_layernorm_eps(EPS)
    eng.set_rope(THETA)
    eng.load_weights(reference()[0])
    return eng


def tokens(eng, imgs):
    return eng.intermediate(imgs, [CFG.depth - 1], "tokens", True)[:, 0]


@pytest.mark.parametrize("fp32_split", [0, -1], ids=["split", "fp32-mfma"])
@pytest.mark.parametrize("ln_fold", [0, -1], ids=["ln-folded", "ln-kernels"])
def test_fp32_tokens_class_features_and_attention_rows_match_transformers(ln_fold, fp32_split):
    W, imgs, ref, flat = reference()
    eng = dinov3_engine(max_batch=4, ln_fold=ln_fold, fp32_split=fp32_split)
    try:
        want = tokens(eng, imgs)
        terr, cerr = rel_err(want, ref["tokens"]), rel_err(eng.features(imgs, "cls"), ref["cls"])
        aerr = float(np.abs(eng.cls_attention(imgs, "heads") - ref["attn"]).max())
        B.lib().vit_engine_set_rope.argtypes = [B.C.c_void_p, B.C.c_double]
        for bad in (-1.0, float("nan")):   # refused, and no bit of the next forward changes
            assert B.lib().vit_engine_set_rope(eng._h, bad) == VIT_ERR_ARG and eng.get_rope() == THETA and same_bits(tokens(eng, imgs), want)
        eng.load_weights(W)                # an install keeps the setting
        assert eng.get_rope() == THETA and same_bits(tokens(eng, imgs), want)
        eng.set_rope(0)                    # the piece is really there: without it the engine follows the model without it
        off, aoff = tokens(eng, imgs), eng.cls_attention(imgs, "heads")
        print(f"fp32 ln_fold={ln_fold} fp32_split={fp32_split}: tokens {terr:.3e}, cls {cerr:.3e} of max |ref|, attention rows {aerr:.3e}; "
              f"rotation off: {rel_err(off, ref['tokens']):.3e} from the reference, {rel_err(off, flat['tokens']):.3e} from the model without")
        assert terr <= LOGIT_REL and cerr <= LOGIT_REL and aerr <= PROB_TOL
        assert eng.get_rope() == 0.0 and rel_err(off, ref["tokens"]) > 10 * LOGIT_REL and rel_err(off, flat["tokens"]) <= LOGIT_REL
        assert float(np.abs(aoff - ref["attn"]).max()) > 10 * PROB_TOL and float(np.abs(aoff - flat["attn"]).max()) <= PROB_TOL
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_pruning_lanes_batch_position_and_graph_replay_change_no_bit(dtype):
    imgs = reference()[1]
    idx = np.array([0, 1, 2, 3, 3, 0, 2, 1, 4, 3, 0])   # chunks of 8 and 3, every image at several places
    batch = imgs[idx]
    plain, pruned, graph = (dinov3_engine(max_batch=8, dtype=dtype, **o) for o in ({}, {"prune_last_layer": True}, {"use_graph": True}))
    try:
        def outputs(eng):
            return eng.features(batch, "cls"), tokens(eng, batch), eng.cls_attention(batch, "heads"), eng.forward(batch)

        want = outputs(plain)
        assert all(np.isfinite(w).all() for w in want)
        for k in range(N):
            assert all((w[idx == k] == w[idx == k][0]).all() for w in want), k
        assert all(same_bits(g, w) for g, w in zip(outputs(pruned), want))
        plain.set_lanes(2)
        assert all(same_bits(g, w) for g, w in zip(outputs(plain), want))
        d8, d_out = B.DeviceArray.from_numpy(batch[:8]), B.DeviceArray((8, CFG.embed_dim))
        for theta in (THETA, THETA, THETA, 0.0, THETA):   # the capture, two replays, and no graph outlives a change of the setting
            if graph.get_rope() != theta:
                graph.set_rope(theta)
            assert same_bits(device_features(graph, d8, 8, "cls", d_out=d_out), want[0][:8]) == (theta == THETA), theta
    finally:
        for eng in (plain, pruned, graph):
            eng.close()


@pytest.mark.parametrize("ln_fold", [0, -1], ids=["ln-folded", "ln-kernels"])
def test_bf16_tokens_stay_within_twice_the_error_of_the_engine_without_rotation(ln_fold):
    _, imgs, ref, flat = reference()
    eng = dinov3_engine(max_batch=8, dtype="bf16", ln_fold=ln_fold)
    try:
        err, aerr = rel_err(tokens(eng, imgs), ref["tokens"]), float(np.abs(eng.cls_attention(imgs, "heads") - ref["attn"]).max())
        eng.set_rope(0)
        base, abase = rel_err(tokens(eng, imgs), flat["tokens"]), float(np.abs(eng.cls_attention(imgs, "heads") - flat["attn"]).max())
    finally:
        eng.close()
    print(f"bf16 ln_fold={ln_fold}: tokens {err:.3e} of max |ref| with the rotation, {base:.3e} without; attention rows {aerr:.3e} / {abase:.3e}")
    assert err <= 2.0 * base, (err, base)
