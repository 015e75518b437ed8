"""tests/head_model.py against code that is not this repository's.

* `[cls | mean of the normalised patch tokens]`, "norm, then mean", against transformers' Dinov2ForImageClassification: a tiny random
  model (hidden 128, 2 heads, depth 2, 28 px / patch 14, 10 labels, LayerScale on, eps 1e-6) whose state dict is mapped onto the
  Network order here -- query / key / value stacked into in_proj, lambda1 into the LayerScale vectors of tests/layer_scale_model.py,
  `classifier` into the head.  Bar: the project's LOGIT_REL = 1e-3 of max |ref|.  Measured: max |d| / max |ref| = 1.0e-6.
* "mean, then norm" (timm's fc_norm) has no library on the build machine; it is held to ten lines of torch.
"""
import numpy as np
import pytest

import head_model
import layer_scale_model
from conftest import oracle_config
from patch14_model import TINY14
from vit_amd import synth

LOGIT_REL = 1e-3


def rel_err(got, ref) -> float:
    return float(np.abs(got - ref).max()) / float(np.abs(ref).max())


def tiny_dinov2(seed):
    """(model, W in Network order with a zero head of the backbone's own, LayerScale vectors, classifier weight, bias)."""
    torch = pytest.importorskip("torch")
    transformers = pytest.importorskip("transformers")
    cfg = TINY14
    hf = transformers.Dinov2Config(hidden_size=cfg.embed_dim, num_hidden_layers=cfg.depth, num_attention_heads=cfg.num_heads,
                                   mlp_ratio=cfg.hidden_dim // cfg.embed_dim, image_size=cfg.img_size, patch_size=cfg.patch_size,
                                   num_labels=cfg.num_classes, layer_norm_eps=1e-6, layerscale_value=1.0, hidden_act="gelu", qkv_bias=True,
                                   hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, drop_path_rate=0.0, use_swiglu_ffn=False)
    model = transformers.Dinov2ForImageClassification(hf).eval()
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
              sd[p + "mlp.fc1.weight"].reshape(-1), sd[p + "mlp.fc1.bias"], sd[p + "mlp.fc2.weight"].reshape(-1), sd[p + "mlp.fc2.bias"]]
        ls += [sd[p + "layer_scale1.lambda1"], sd[p + "layer_scale2.lambda1"]]
    W += [sd["dinov2.layernorm.weight"], sd["dinov2.layernorm.bias"], np.zeros(cfg.num_classes * cfg.embed_dim, np.float32),
          np.zeros(cfg.num_classes, np.float32)]
    shapes = [w.shape for w in synth.make_weights(cfg, 1)]  # the Network's tensors as the oracle's ops take them: [out][in] matrices
    assert [w.size for w in W] == [int(np.prod(s)) for s in shapes]
    W = [np.ascontiguousarray(w, np.float32).reshape(s) for w, s in zip(W, shapes)]
    return model, W, ls, sd["classifier.weight"], sd["classifier.bias"]


def test_dinov2_linear_head_is_cls_then_mean_of_the_normalised_patch_tokens(oracle):
    """Measured on the build machine: max |logits - transformers| / max |transformers| = 1.0e-6 (bar 1e-3)."""
    import torch
    cfg = TINY14
    model, W, ls, cw, cb = tiny_dinov2(seed=3)
    imgs = synth.make_images(cfg, 3, 41)
    with torch.no_grad():
        ref = model(pixel_values=torch.from_numpy(imgs)).logits.numpy()
    stages = [layer_scale_model.forward_image(oracle, oracle_config(cfg), im, W, ls)[2] for im in imgs]
    cls_layers, pool = head_model.families(cfg.depth)["dinov2_1"]
    rows = head_model.operands(oracle, stages, W[-4], W[-3], cls_layers, pool)
    assert rows.shape == (3, 2 * cfg.embed_dim) == (3, head_model.in_features(cfg.embed_dim, cls_layers, pool))
    got = head_model.logits(oracle, rows, cw, cb)
    err = rel_err(got, ref)
    print(f"dinov2 linear head: max |d| / max |ref| = {err:.3e}, max |ref| = {np.abs(ref).max():.3f}")
    assert float(np.abs(ref).max()) > 0.1  # the comparison means something
    assert err <= LOGIT_REL
    # the order of the blocks and the order of norm and mean are pinned: each wrong reading misses the bar by orders of magnitude
    swapped = np.concatenate([rows[:, cfg.embed_dim:], rows[:, :cfg.embed_dim]], 1)
    assert rel_err(head_model.logits(oracle, swapped, cw, cb), ref) > 100 * LOGIT_REL
    wrong = head_model.operands(oracle, stages, W[-4], W[-3], cls_layers, "avg_fcnorm")
    assert rel_err(head_model.logits(oracle, wrong, cw, cb), ref) > 100 * LOGIT_REL


def test_fcnorm_pools_first_and_normalises_the_pooled_row(oracle):
    import torch
    import torch.nn.functional as F
    cfg = TINY14
    W = synth.make_weights(cfg, 5)
    imgs = synth.make_images(cfg, 3, 43)
    stages = [oracle.forward_image(oracle_config(cfg), im, W, want_stages=True)[2] for im in imgs]
    tokens = torch.from_numpy(np.stack([st[-1] for st in stages])).double()
    g, b = torch.from_numpy(np.asarray(W[-4], np.float32)).double(), torch.from_numpy(np.asarray(W[-3], np.float32)).double()
    ref = F.layer_norm(tokens[:, 1:].mean(1), (cfg.embed_dim,), g, b, eps=1e-6).numpy()
    got = head_model.operands(oracle, stages, W[-4], W[-3], (), "avg_fcnorm")
    err = rel_err(got, ref)
    print(f"avg_fcnorm: max |d| / max |ref| = {err:.3e}")
    assert got.shape == ref.shape and err <= LOGIT_REL
    avg = F.layer_norm(tokens, (cfg.embed_dim,), g, b, eps=1e-6)[:, 1:].mean(1).numpy()
    assert rel_err(head_model.operands(oracle, stages, W[-4], W[-3], (), "avg"), avg) <= LOGIT_REL
    assert rel_err(avg, ref) > 100 * LOGIT_REL  # the two orders are different functions


def test_the_four_layer_head_reads_the_class_rows_of_the_last_four_layers_earliest_first(oracle):
    """DINOv2's create_linear_input: torch.cat([class_token for output, class_token in x_tokens_list[-4:]]) + the mean of the last."""
    rng = np.random.default_rng(7)
    depth, T, D = 5, 4, 8
    stages = rng.normal(0, 1, (depth + 1, T, D)).astype(np.float32)
    g, b = rng.uniform(0.5, 1.5, D).astype(np.float32), rng.uniform(-0.5, 0.5, D).astype(np.float32)
    cls_layers, pool = head_model.families(depth)["dinov2_4"]
    assert cls_layers == (1, 2, 3, 4) and pool == "avg"
    row = head_model.operand(oracle, stages, g, b, cls_layers, pool)
    assert row.shape == (5 * D,)
    for k, l in enumerate(cls_layers):
        assert np.array_equal(row[k * D:(k + 1) * D], oracle.layer_norm(np.ascontiguousarray(stages[l + 1][:1]), g, b)[0])
    assert np.allclose(row[4 * D:], oracle.layer_norm(np.ascontiguousarray(stages[-1]), g, b)[1:].mean(0), atol=1e-6)
