"""tests/headdim_model.py against code that is not this repository's: transformers.CLIPVisionModelWithProjection at head_dim 80 and 104.

Randomly initialised towers (hidden 320 / 416, 4 heads, 2 layers, 28 px / patch 14, eps 1e-5) with hidden_act "gelu" (OpenCLIP
ViT-H-14 / bigG-14) and "quick_gelu", every parameter re-randomised as in tests/test_clip_model.py, are mapped onto the engine's
weight order by clip_model.from_transformers and compared on image_embeds and hidden_states[-2].  Bar: LOGIT_REL = 1e-3 of max |ref|.

The model is SENSITIVE to the head_dim under the square root: sqrt(64) on the same tower moves the output by more than the bar.
"""
import numpy as np
import pytest

import headdim_model
from test_clip_model import LOGIT_REL, hf_run, rel_err

TOWERS = {80: 320, 104: 416}  # head_dim -> hidden_size at 4 heads


def make_tower(head_dim: int, hidden_act: str = "gelu"):
    """(torch, model, images): tests/test_gpu_headdim_engine.py loads the head_dim 80 one too."""
    torch = pytest.importorskip("torch")
    transformers = pytest.importorskip("transformers")
    D = TOWERS[head_dim]
    hf = transformers.CLIPVisionConfig(hidden_size=D, intermediate_size=2 * D, projection_dim=64, num_hidden_layers=2,
                                       num_attention_heads=4, num_channels=3, image_size=28, patch_size=14, hidden_act=hidden_act,
                                       layer_norm_eps=1e-5, attention_dropout=0.0)
    model = transformers.CLIPVisionModelWithProjection(hf).eval()
    gen = torch.Generator().manual_seed(37 + head_dim)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if "norm" in name and name.endswith("weight"):
                p.copy_(torch.rand(p.shape, generator=gen) * 1.5 + 0.25)
            elif "norm" in name:
                p.copy_((torch.rand(p.shape, generator=gen) * 2 - 1) * 0.5)
            elif p.ndim >= 2 and "embedding" not in name:
                p.copy_((torch.rand(p.shape, generator=gen) * 2 - 1) * (1.5 / np.sqrt(p.shape[-1])))
            else:
                p.copy_((torch.rand(p.shape, generator=gen) * 2 - 1) * 0.1)
    images = torch.rand((3, 3, 28, 28), generator=gen) * 4.7 - 2.1
    return torch, model, images


@pytest.mark.parametrize("hidden_act", ["gelu", "quick_gelu"])
@pytest.mark.parametrize("head_dim", sorted(TOWERS))
def test_the_model_is_transformers_clip_vision_tower(head_dim, hidden_act):
    torch, model, images = make_tower(head_dim, hidden_act)
    cfg, W, pre, eps = headdim_model.from_transformers(model)
    assert cfg.embed_dim // cfg.num_heads == head_dim and eps == 1e-5 and len(W) == cfg.n_weights
    assert [tuple(np.shape(w)) for w in W] == [tuple(s) for s in cfg.weight_shapes()]
    ref_e, ref_h = hf_run(torch, model, images)
    got = headdim_model.forward(cfg, images.numpy(), W, pre, eps, act=cfg.mlp)
    e_err, h_err = rel_err(got["embeds"], ref_e), rel_err(got["stages"][:, -2], ref_h)
    print(f"headdim_model (head_dim {head_dim}, {hidden_act}) vs transformers: image_embeds {e_err:.2e}, hidden_states[-2] {h_err:.2e}")
    assert e_err <= LOGIT_REL and h_err <= LOGIT_REL
    unit = ref_e / np.linalg.norm(ref_e, axis=1, keepdims=True)
    assert float(np.abs(got["unit"] - unit).max()) <= LOGIT_REL * float(np.abs(unit).max())
    # the square root of 64 in head_dim's place is another model
    wrong = headdim_model.forward(cfg, images.numpy(), W, pre, eps, act=cfg.mlp, score_dim=64)
    w_err = rel_err(wrong["embeds"], ref_e)
    print(f"  with sqrt(64): image_embeds {w_err:.2e}")
    assert w_err > LOGIT_REL


def test_head_dim_64_is_clip_model():
    """At 64 the general model is tests/clip_model.py to the last bit of float64 (one formula, two files)."""
    import clip_model
    from vit_amd import synth

    cfg = clip_model.TINY_CLIP
    W, x = synth.make_weights(cfg, 5), synth.make_images(cfg, 2, 6)
    a = clip_model.forward(cfg, x, W, None, 1e-5)
    b = headdim_model.forward(cfg, x, W, None, 1e-5, act="quickgelu")
    assert np.array_equal(a["embeds"], b["embeds"]) and np.array_equal(a["stages"], b["stages"])
