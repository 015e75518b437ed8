"""tests/swiglu_model.py and the checkpoint mapping of INTEGRATION.md against code that is not this repository's: transformers'
Dinov2Model / Dinov2ForImageClassification with use_swiglu_ffn=True.

A small random model (hidden 128, 2 heads, depth 2, 28 px / patch 14, 10 labels, LayerScale on, eps 1e-6, mlp_ratio 3: the module
rounds its hidden width to (int(384 * 2 / 3) + 7) // 8 * 8 = 256).  Its state dict is mapped onto the Network order --
query / key / value stacked into in_proj, mlp.weights_in into the fc1 slots (+8, +9), mlp.weights_out into the fc2 slots (+10, +11)
-- and LayerScale is folded by binding.fold_layer_scale (ls1 into out_proj, ls2 into w3), so that the model runs without it.
Bar: the project's LOGIT_REL = 1e-3 of max |ref|, on the last hidden states and on the logits.
Measured on the build machine: last hidden state 1.4e-6, logits 9.7e-7 (the halves of w12 swapped: 0.64 and 0.78).
"""
import dataclasses

import numpy as np
import pytest

import head_model
import swiglu_model
from conftest import oracle_config
from patch14_model import TINY14
from vit_amd import binding as B
from vit_amd import synth

LOGIT_REL = 1e-3
CFG = dataclasses.replace(TINY14, hidden_dim=256, mlp="swiglu")


def rel_err(got, ref) -> float:
    return float(np.abs(got - ref).max()) / float(np.abs(ref).max())


@pytest.fixture(scope="module")
def pinned():
    """(model, folded W in Network order with a zero head of the backbone's own, classifier weight, bias, images)."""
    torch = pytest.importorskip("torch")
    transformers = pytest.importorskip("transformers")
    cfg = CFG
    hf = transformers.Dinov2Config(hidden_size=cfg.embed_dim, num_hidden_layers=cfg.depth, num_attention_heads=cfg.num_heads, mlp_ratio=3,
                                   image_size=cfg.img_size, patch_size=cfg.patch_size, num_labels=cfg.num_classes, layer_norm_eps=1e-6,
                                   layerscale_value=1.0, qkv_bias=True, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                                   drop_path_rate=0.0, use_swiglu_ffn=True)
    model = transformers.Dinov2ForImageClassification(hf).eval()
    gen = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("lambda1"):
                p.copy_(torch.rand(p.shape, generator=gen) * 1.45 + 0.05)
            elif "norm" in name and name.endswith("weight"):
                p.copy_(torch.rand(p.shape, generator=gen) + 0.5)
            elif p.ndim >= 2 and "embeddings" not in name:
                p.copy_((torch.rand(p.shape, generator=gen) * 2 - 1) * (1.5 / np.sqrt(p.shape[-1])))
            else:
                p.copy_((torch.rand(p.shape, generator=gen) * 2 - 1) * 0.1)
    sd = {k: v.detach().numpy().astype(np.float32) for k, v in model.state_dict().items()}
    assert sd["dinov2.encoder.layer.0.mlp.weights_in.weight"].shape == (2 * cfg.hidden_dim, cfg.embed_dim)
    assert sd["dinov2.encoder.layer.0.mlp.weights_out.weight"].shape == (cfg.embed_dim, cfg.hidden_dim)
    e = "dinov2.embeddings."
    W = [sd[e + "cls_token"].reshape(-1), sd[e + "patch_embeddings.projection.weight"].reshape(-1),
         sd[e + "patch_embeddings.projection.bias"], sd[e + "position_embeddings"].reshape(-1)]
    ls = []
    for l in range(cfg.depth):
        p = f"dinov2.encoder.layer.{l}."
        a = p + "attention.attention."
        W += [sd[p + "norm1.weight"], sd[p + "norm1.bias"],
              np.concatenate([sd[a + "query.weight"], sd[a + "key.weight"], sd[a + "value.weight"]]).reshape(-1),
              np.concatenate([sd[a + "query.bias"], sd[a + "key.bias"], sd[a + "value.bias"]]),
              sd[p + "attention.output.dense.weight"].reshape(-1), sd[p + "attention.output.dense.bias"],
              sd[p + "norm2.weight"], sd[p + "norm2.bias"],
              sd[p + "mlp.weights_in.weight"].reshape(-1), sd[p + "mlp.weights_in.bias"],
              sd[p + "mlp.weights_out.weight"].reshape(-1), sd[p + "mlp.weights_out.bias"]]
        ls += [sd[p + "layer_scale1.lambda1"], sd[p + "layer_scale2.lambda1"]]
    W += [sd["dinov2.layernorm.weight"], sd["dinov2.layernorm.bias"], np.zeros(cfg.num_classes * cfg.embed_dim, np.float32),
          np.zeros(cfg.num_classes, np.float32)]
    shapes = cfg.weight_shapes()
    assert [w.size for w in W] == [int(np.prod(s)) for s in shapes]
    W = B.fold_layer_scale(cfg, [np.ascontiguousarray(w, np.float32).reshape(s) for w, s in zip(W, shapes)], ls)
    return model, W, sd["classifier.weight"], sd["classifier.bias"], synth.make_images(cfg, 3, 47)


def run(oracle, W, cw, cb, imgs):
    """(last hidden states [n][T][D], logits [n][classes]) of the model on the folded tensors, with DINOv2's linear head."""
    cfg = CFG
    stages = [swiglu_model.forward_image(oracle, oracle_config(cfg), im, W)[2] for im in imgs]
    hidden = np.stack([oracle.layer_norm(np.ascontiguousarray(st[-1]), W[-4], W[-3]) for st in stages])
    cls_layers, pool = head_model.families(cfg.depth)["dinov2_1"]
    rows = head_model.operands(oracle, stages, W[-4], W[-3], cls_layers, pool)
    return hidden, head_model.logits(oracle, rows, cw, cb)


def test_swiglu_model_and_checkpoint_mapping_agree_with_transformers(oracle, pinned):
    """Measured on the build machine: max |d| / max |ref| = 1.4e-6 on the last hidden states, 9.7e-7 on the logits (bar 1e-3); with the
    two halves of every w12 swapped 0.64 and 0.78."""
    import torch
    model, W, cw, cb, imgs = pinned
    with torch.no_grad():
        px = torch.from_numpy(imgs)
        ref_hidden = model.dinov2(pixel_values=px).last_hidden_state.numpy()
        ref_logits = model(pixel_values=px).logits.numpy()
    hidden, logits = run(oracle, W, cw, cb, imgs)
    eh, el = rel_err(hidden, ref_hidden), rel_err(logits, ref_logits)
    print(f"swiglu vs transformers: last hidden {eh:.3e}, logits {el:.3e}, max |logit| = {np.abs(ref_logits).max():.3f}")
    assert float(np.abs(ref_logits).max()) > 0.1  # the comparison means something
    assert hidden.shape == ref_hidden.shape and eh <= LOGIT_REL
    assert logits.shape == ref_logits.shape and el <= LOGIT_REL
    # the order of the halves is pinned: value rows first misses the bar by orders of magnitude
    H, swapped = CFG.hidden_dim, list(W)
    for l in range(CFG.depth):
        w12, b12 = W[4 + 12 * l + 8], W[4 + 12 * l + 9]
        swapped[4 + 12 * l + 8] = np.ascontiguousarray(np.concatenate([w12[H:], w12[:H]]))
        swapped[4 + 12 * l + 9] = np.ascontiguousarray(np.concatenate([b12[H:], b12[:H]]))
    sh, sl = run(oracle, swapped, cw, cb, imgs)
    print(f"halves swapped: last hidden {rel_err(sh, ref_hidden):.3e}, logits {rel_err(sl, ref_logits):.3e}")
    assert rel_err(sh, ref_hidden) > 100 * LOGIT_REL and rel_err(sl, ref_logits) > 100 * LOGIT_REL


def test_the_gate_is_silu_of_the_first_half_times_the_second():
    """tests/swiglu_model.gate against torch's own silu on the module's chunk(2, dim=-1), to fp32 rounding."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(5)
    u = rng.uniform(-20, 20, (7, 2 * 24)).astype(np.float32)
    x1, x2 = torch.from_numpy(u).double().chunk(2, dim=-1)
    ref = (torch.nn.functional.silu(x1) * x2).numpy()
    got = swiglu_model.gate(u, 24)
    assert got.dtype == np.float32 and np.array_equal(got, ref.astype(np.float32))


def test_fold_layer_scale_accepts_the_swiglu_configuration_and_scales_w3_rows():
    cfg = CFG
    W = synth.make_weights(cfg, 3, native=False)
    ls = [np.full(cfg.embed_dim, 1.0 + 0.25 * i, np.float32) for i in range(2 * cfg.depth)]
    F = B.fold_layer_scale(cfg, W, ls)
    for l in range(cfg.depth):
        assert np.array_equal(F[4 + 12 * l + 10], np.float32(1.25 + 0.5 * l) * W[4 + 12 * l + 10])   # w3, by ls2
        assert np.array_equal(F[4 + 12 * l + 8], W[4 + 12 * l + 8]) and F[4 + 12 * l + 8].shape == (2 * cfg.hidden_dim, cfg.embed_dim)
    gelu_sized = list(W)
    gelu_sized[12] = np.ascontiguousarray(W[12][:cfg.hidden_dim])
    with pytest.raises(B.VitError):
        B.fold_layer_scale(cfg, gelu_sized, ls)
