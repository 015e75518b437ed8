"""tests/clip_model.py against code that is not this repository's: transformers.CLIPVisionModelWithProjection.

A tiny random tower (hidden 128, 2 heads, 2 layers, intermediate 256, 32 px / patch 8, projection 64, quick_gelu, eps 1e-5) whose EVERY
parameter is re-randomised -- the LayerNorm weights and biases and class_embedding included, whose default initialisation (ones, zeros)
would hide a mapping mistake -- is mapped onto the engine's weight order by clip_model.from_transformers (INTEGRATION.md's table) and
compared on image_embeds and hidden_states[-2].  Bar: the project's LOGIT_REL = 1e-3 of max |ref| (tests/test_head_model.py).
Measured: image_embeds 4.1e-07, hidden_states[-2] 4.4e-07 of max |ref| (fp32 torch against the float64 model).

The model is also SENSITIVE to each of the three pieces: erf-GELU in QuickGELU's place, no pre-norm, or eps 1e-6 on an input scaled
until the rows' variances are about 1e-5 each move the output by more than the bar.
"""
import numpy as np
import pytest

import clip_model
from clip_model import TINY_CLIP

LOGIT_REL = 1e-3


def rel_err(got, ref) -> float:
    return float(np.abs(got - ref).max()) / float(np.abs(ref).max())


def make_tower():
    """(torch, model, images): the tiny random tower, every parameter re-randomised (tests/test_gpu_clip_engine.py loads it too)."""
    torch = pytest.importorskip("torch")
    transformers = pytest.importorskip("transformers")
    c = TINY_CLIP
    hf = transformers.CLIPVisionConfig(hidden_size=c.embed_dim, intermediate_size=c.hidden_dim, projection_dim=c.num_classes,
                                       num_hidden_layers=c.depth, num_attention_heads=c.num_heads, num_channels=c.in_chans,
                                       image_size=c.img_size, patch_size=c.patch_size, hidden_act="quick_gelu", layer_norm_eps=1e-5,
                                       attention_dropout=0.0)
    model = transformers.CLIPVisionModelWithProjection(hf).eval()
    gen = torch.Generator().manual_seed(31)
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
    images = (torch.rand((3, c.in_chans, c.img_size, c.img_size), generator=gen) * 4.7 - 2.1)
    return torch, model, images


@pytest.fixture(scope="module")
def tower():
    return make_tower()


def hf_run(torch, model, images):
    with torch.no_grad():
        out = model(pixel_values=images, output_hidden_states=True)
    return out.image_embeds.numpy().astype(np.float64), out.hidden_states[-2].numpy().astype(np.float64)


def test_the_model_is_transformers_clip_vision_tower(tower):
    torch, model, images = tower
    cfg, W, pre, eps = clip_model.from_transformers(model)
    assert cfg == TINY_CLIP and eps == 1e-5 and len(W) == cfg.n_weights
    assert [tuple(np.shape(w)) for w in W] == [tuple(s) for s in cfg.weight_shapes()]
    ref_e, ref_h = hf_run(torch, model, images)
    got = clip_model.forward(cfg, images.numpy(), W, pre, eps)
    e_err, h_err = rel_err(got["embeds"], ref_e), rel_err(got["stages"][:, -2], ref_h)
    print(f"clip_model vs transformers: image_embeds {e_err:.2e}, hidden_states[-2] {h_err:.2e} of max |ref|")
    assert e_err <= LOGIT_REL and h_err <= LOGIT_REL
    unit = ref_e / np.linalg.norm(ref_e, axis=1, keepdims=True)
    assert float(np.abs(got["unit"] - unit).max()) <= LOGIT_REL * float(np.abs(unit).max())
    assert np.allclose(got["probs"].sum(1), 1.0)


def test_each_piece_moves_the_output_by_more_than_the_bar(tower):
    torch, model, images = tower
    cfg, W, pre, eps = clip_model.from_transformers(model)
    x = images.numpy()
    ref = clip_model.forward(cfg, x, W, pre, eps)["embeds"]
    assert rel_err(clip_model.forward(cfg, x, W, pre, eps, act="gelu")["embeds"], ref) > LOGIT_REL
    assert rel_err(clip_model.forward(cfg, x, W, None, eps)["embeds"], ref) > LOGIT_REL
    # epsilon: at ordinary scales 1e-5 and 1e-6 both vanish beside the variance.  Scale the input AND the additive embeddings until the
    # rows the pre-norm sees have variances of about 1e-5; transformers must still agree, and 1e-6 must not.
    small = [w.copy() for w in W]
    row_var = float(np.var((clip_model.patches(cfg, x[0]) @ small[1].T + small[3][1:]), axis=1).mean())
    s = float(np.sqrt(1e-5 / row_var))
    with torch.no_grad():
        emb = model.vision_model.embeddings
        keep = (emb.class_embedding.clone(), emb.position_embedding.weight.clone())
        emb.class_embedding.mul_(s)
        emb.position_embedding.weight.mul_(s)
        try:
            xs = (images * s).float()
            ref_e, _ = hf_run(torch, model, xs)
        finally:
            emb.class_embedding.copy_(keep[0])
            emb.position_embedding.weight.copy_(keep[1])
    small[0] = keep[0].numpy() * np.float32(s)
    small[3] = keep[1].numpy() * np.float32(s)
    got5 = clip_model.forward(cfg, xs.numpy(), small, pre, 1e-5)["embeds"]
    got6 = clip_model.forward(cfg, xs.numpy(), small, pre, 1e-6)["embeds"]
    print(f"scaled input (row variance ~1e-5): eps 1e-5 vs transformers {rel_err(got5, ref_e):.2e}, eps 1e-6 {rel_err(got6, ref_e):.2e}")
    assert rel_err(got5, ref_e) <= LOGIT_REL
    assert rel_err(got6, ref_e) > LOGIT_REL
