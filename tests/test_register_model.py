"""tests/register_model.py against code that is not this repository's: transformers' Dinov2WithRegistersForImageClassification and
Dinov2WithRegistersBackbone.

A tiny random model as tests/test_head_model.py::tiny_dinov2 makes them (hidden 128, 2 heads, 2 layers, 28 px / patch 14, 10 labels,
LayerScale on, eps 1e-6) with R = 4 register tokens; its state dict is mapped onto the Network order by INTEGRATION.md's table --
cls_token and register_tokens stacked into tensor 0, LayerScale folded with vit_weights_fold_layer_scale.  Bar: the project's
LOGIT_REL = 1e-3 of max |ref|; the wrong reading (registers inside the mean) must miss by more than 100 times that.
"""
import numpy as np
import pytest

import register_model
from register_model import REG_TINY
from vit_amd import binding as B
from vit_amd import synth

LOGIT_REL = 1e-3


def rel_err(got, ref) -> float:
    return float(np.abs(got - ref).max()) / float(np.abs(ref).max())


def tiny_dinov2_reg(seed, cfg=REG_TINY):
    """(model, W in Network order with LayerScale folded and a zero head of the backbone's own, classifier weight, bias)."""
    torch = pytest.importorskip("torch")
    transformers = pytest.importorskip("transformers")
    hf = transformers.Dinov2WithRegistersConfig(
        hidden_size=cfg.embed_dim, num_hidden_layers=cfg.depth, num_attention_heads=cfg.num_heads, mlp_ratio=cfg.hidden_dim // cfg.embed_dim,
        image_size=cfg.img_size, patch_size=cfg.patch_size, num_labels=cfg.num_classes, layer_norm_eps=1e-6, layerscale_value=1.0,
        hidden_act="gelu", qkv_bias=True, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, drop_path_rate=0.0,
        use_swiglu_ffn=False, num_register_tokens=cfg.num_register_tokens)
    model = transformers.Dinov2WithRegistersForImageClassification(hf).eval()
    gen = torch.Generator().manual_seed(seed)
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
    W, ls = network_from_state_dict(cfg, sd, "dinov2_with_registers.")
    return model, B.fold_layer_scale(cfg, W, ls), sd["classifier.weight"], sd["classifier.bias"]


def network_from_state_dict(cfg, sd, root):
    """INTEGRATION.md's table for Dinov2WithRegisters*: (W in Network order, LayerScale vectors); the head slot is zero."""
    D = cfg.embed_dim
    e = root + "embeddings."
    assert sd[e + "register_tokens"].shape == (1, cfg.num_register_tokens, D)
    W = [np.concatenate([sd[e + "cls_token"].reshape(1, D), sd[e + "register_tokens"].reshape(-1, D)]).reshape(-1),
         sd[e + "patch_embeddings.projection.weight"].reshape(-1), sd[e + "patch_embeddings.projection.bias"],
         sd[e + "position_embeddings"].reshape(-1)]
    ls = []
    for l in range(cfg.depth):
        p = f"{root}encoder.layer.{l}."
        a = p + "attention.attention."
        W += [sd[p + "norm1.weight"], sd[p + "norm1.bias"],
              np.concatenate([sd[a + "query.weight"], sd[a + "key.weight"], sd[a + "value.weight"]]).reshape(-1),
              np.concatenate([sd[a + "query.bias"], sd[a + "key.bias"], sd[a + "value.bias"]]),
              sd[p + "attention.output.dense.weight"].reshape(-1), sd[p + "attention.output.dense.bias"],
              sd[p + "norm2.weight"], sd[p + "norm2.bias"],
              sd[p + "mlp.fc1.weight"].reshape(-1), sd[p + "mlp.fc1.bias"], sd[p + "mlp.fc2.weight"].reshape(-1), sd[p + "mlp.fc2.bias"]]
        ls += [sd[p + "layer_scale1.lambda1"], sd[p + "layer_scale2.lambda1"]]
    W += [sd[root + "layernorm.weight"], sd[root + "layernorm.bias"], np.zeros(cfg.num_classes * D, np.float32),
          np.zeros(cfg.num_classes, np.float32)]
    shapes = cfg.weight_shapes()
    assert [w.size for w in W] == [int(np.prod(s)) for s in shapes]
    return [np.ascontiguousarray(w, np.float32).reshape(s) for w, s in zip(W, shapes)], ls


_cache = {}


def hf_reference(seed=3, n=3, img_seed=41):
    """(cfg, W, classifier weight, bias, images, transformers' last hidden state [n][T][D], its logits [n][NC]), computed once."""
    key = (seed, n, img_seed)
    if key not in _cache:
        import torch
        model, W, cw, cb = tiny_dinov2_reg(seed)
        imgs = synth.make_images(REG_TINY, n, img_seed)
        with torch.no_grad():
            out = model(pixel_values=torch.from_numpy(imgs), output_hidden_states=True)
            # hidden_states[-1] is the residual stream behind the last layer; last_hidden_state = its final LayerNorm
            hidden = out.hidden_states[-1].numpy()
            normed = model.dinov2_with_registers(torch.from_numpy(imgs)).last_hidden_state.numpy()
        _cache[key] = (REG_TINY, W, cw, cb, imgs, hidden, normed, out.logits.numpy())
    return _cache[key]


def test_the_model_is_transformers_dinov2_with_registers():
    """hidden_states[-1], last_hidden_state and the logits, each within 1e-3 of max |ref| (the figures are printed)."""
    cfg, W, cw, cb, imgs, hidden, normed, ref = hf_reference()
    R, D = cfg.num_register_tokens, cfg.embed_dim
    assert hidden.shape == (3, 1 + R + cfg.patches, D) == (3, cfg.tokens, D)
    got = register_model.forward(cfg, imgs, W)
    herr, nerr = rel_err(got["stages"][:, -1], hidden), rel_err(got["norm"], normed)
    logits = got["operand"] @ cw.astype(np.float64).T + cb
    lerr = rel_err(logits, ref)
    print(f"registers vs transformers: hidden_states[-1] {herr:.3e}, last_hidden_state {nerr:.3e}, logits {lerr:.3e} of max |ref| = "
          f"{np.abs(ref).max():.3f}")
    assert float(np.abs(ref).max()) > 0.1  # the comparison means something
    assert herr <= LOGIT_REL and nerr <= LOGIT_REL and lerr <= LOGIT_REL
    # the wrong reading: the registers inside the mean
    wrong = register_model.forward(cfg, imgs, W, registers_in_mean=True)["operand"] @ cw.astype(np.float64).T + cb
    werr = rel_err(wrong, ref)
    print(f"registers inside the mean: {werr:.3e} of max |ref|")
    assert werr > 100 * LOGIT_REL


def test_the_register_rows_take_no_position_embedding():
    cfg, W, *_ = hf_reference()
    x = register_model.embed(cfg, synth.make_images(cfg, 1, 5)[0], W)
    R = cfg.num_register_tokens
    assert np.array_equal(x[1:1 + R], np.asarray(W[0], np.float64)[1:])
    assert np.array_equal(x[0], np.asarray(W[0], np.float64)[0] + np.asarray(W[3], np.float64)[0])
    assert x.shape == (cfg.tokens, cfg.embed_dim)


def test_the_backbone_maps_are_the_normalised_rows_behind_the_registers():
    """Dinov2WithRegistersBackbone (apply_layernorm, reshape_hidden_states): feature_maps[-1] = LayerNorm(rows 1 + R ..) as [D][g][g]."""
    import torch
    import transformers
    cfg, W, cw, cb, imgs, hidden, normed, _ = hf_reference()
    model = tiny_dinov2_reg(3)[0]
    hf = model.config
    hf.out_features, hf.apply_layernorm, hf.reshape_hidden_states = [f"stage{cfg.depth}"], True, True
    backbone = transformers.Dinov2WithRegistersBackbone(hf).eval()
    missing = backbone.load_state_dict({k[len("dinov2_with_registers."):]: v for k, v in model.state_dict().items()
                                        if k.startswith("dinov2_with_registers.")}, strict=False)
    assert not missing.unexpected_keys and not missing.missing_keys, missing
    with torch.no_grad():
        maps = backbone(torch.from_numpy(imgs)).feature_maps[-1].numpy()
    g = cfg.img_size // cfg.patch_size
    assert maps.shape == (3, cfg.embed_dim, g, g)
    got = np.stack([register_model.patch_map(cfg, rows) for rows in register_model.forward(cfg, imgs, W)["norm"]])
    err = rel_err(got, maps)
    print(f"backbone feature map: {err:.3e} of max |ref|")
    assert err <= LOGIT_REL
    # rows 1 .. (the registers taken for patches) is another selection: the first map entry would be a register row
    assert rel_err(np.stack([rows[1:1 + cfg.patches].T.reshape(-1, g, g) for rows in register_model.forward(cfg, imgs, W)["norm"]]),
                   maps) > 100 * LOGIT_REL
