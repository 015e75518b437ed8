"""A CLIP image tower in float64 numpy: what an engine loaded through INTEGRATION.md's CLIP mapping must reproduce.

    x = [cls | conv(image)] + pos                                       tensors 0..3 (the conv bias is zero in a CLIP checkpoint)
    x = layer_norm(x, pre)                                              ln_pre / pre_layrnorm: vit_engine_set_pre_norm (None: no such step)
    per layer l:  x = x + out_proj(attention(in_proj(layer_norm(x, ln1))))
                  x = x + fc2(act(fc1(layer_norm(x, ln2))))              act: "quickgelu" y * sigmoid(1.702 y) | "gelu" (erf)
    embeds = head(layer_norm(x[0], final))                              visual_projection in the head slot, zero bias: the logits
    probs = softmax(embeds);  unit = embeds / max(||embeds||, 1e-12)

Every LayerNorm uses the one `eps` (CLIP: 1e-5), added to the biased variance.  Weights are the engine's list (synth.ModelConfig.
weight_shapes order).  tests/test_clip_model.py pins this file to transformers.CLIPVisionModelWithProjection.
"""
import math

import numpy as np

from vit_amd import synth

# the reduced towers the tests share (head_dim stays 64)
TINY_CLIP = synth.ModelConfig(img_size=32, patch_size=8, num_classes=64, embed_dim=128, depth=2, num_heads=2, hidden_dim=256, mlp="quickgelu")
# patch 14: the general patch embedding; 17 tokens
SMALL_CLIP = synth.ModelConfig(img_size=56, patch_size=14, num_classes=96, embed_dim=256, depth=3, num_heads=4, hidden_dim=512, mlp="quickgelu")
# one layer at the full width of CLIP ViT-L/14: D 1024, hidden 4096 through the real tile shapes
L14_LAYER = synth.ModelConfig(img_size=28, patch_size=14, num_classes=768, embed_dim=1024, depth=1, num_heads=16, hidden_dim=4096, mlp="quickgelu")

_erf = np.vectorize(math.erf)


def layer_norm(x, g, b, eps):
    x = np.asarray(x, np.float64)
    mean = x.mean(-1, keepdims=True)
    var = ((x - mean) ** 2).mean(-1, keepdims=True)
    return (x - mean) / np.sqrt(var + eps) * np.asarray(g, np.float64) + np.asarray(b, np.float64)


def quick_gelu(y):
    with np.errstate(over="ignore"):
        return y / (1.0 + np.exp(-1.702 * y))


def gelu(y):
    return 0.5 * y * (1.0 + _erf(y / math.sqrt(2.0)))


def patches(cfg, image):
    """[patches][C * P * P], channel-major inside a patch: the rows the flattened conv weight multiplies."""
    C, S, P = cfg.in_chans, cfg.img_size, cfg.patch_size
    G = S // P
    im = np.asarray(image, np.float64).reshape(C, G, P, G, P)
    return im.transpose(1, 3, 0, 2, 4).reshape(G * G, C * P * P)


def forward_image(cfg, image, W, pre=None, eps=1e-5, act="quickgelu"):
    """dict: embeds [NC], probs [NC], unit [NC], stages [depth + 1][T][D] (stage 0: the stream layer 0 reads, behind the pre-norm)."""
    W = [np.asarray(w, np.float64) for w in W]
    D, H, heads = cfg.embed_dim, cfg.hidden_dim, cfg.num_heads
    f = {"quickgelu": quick_gelu, "gelu": gelu}[act]
    x = np.concatenate([W[0].reshape(1, D), patches(cfg, image) @ W[1].reshape(D, -1).T + W[2]]) + W[3].reshape(-1, D)
    if pre is not None:
        x = layer_norm(x, pre[0], pre[1], eps)
    stages = [x]
    for l in range(cfg.depth):
        w = W[4 + 12 * l:16 + 12 * l]
        qkv = layer_norm(x, w[0], w[1], eps) @ w[2].reshape(3 * D, D).T + w[3]
        att = np.empty_like(x)
        for h in range(heads):
            q, k, v = (qkv[:, i * D + h * 64:i * D + (h + 1) * 64] for i in range(3))
            s = q @ k.T / 8.0
            p = np.exp(s - s.max(-1, keepdims=True))
            att[:, h * 64:(h + 1) * 64] = (p / p.sum(-1, keepdims=True)) @ v
        x = x + att @ w[4].reshape(D, D).T + w[5]
        hid = f(layer_norm(x, w[6], w[7], eps) @ w[8].reshape(H, D).T + w[9])
        x = x + hid @ w[10].reshape(D, H).T + w[11]
        stages.append(x)
    embeds = layer_norm(x[0], W[-4], W[-3], eps) @ W[-2].reshape(cfg.num_classes, D).T + W[-1]
    e = np.exp(embeds - embeds.max())
    return {"embeds": embeds, "probs": e / e.sum(), "unit": embeds / max(float(np.linalg.norm(embeds)), 1e-12), "stages": np.stack(stages)}


def forward(cfg, images, W, pre=None, eps=1e-5, act="quickgelu"):
    out = [forward_image(cfg, im, W, pre, eps, act) for im in images]
    return {k: np.stack([o[k] for o in out]) for k in out[0]}


def from_transformers(model):
    """(ModelConfig, engine weight list, (pre gamma, pre beta), eps) of a transformers.CLIPVisionModelWithProjection: the mapping of
    INTEGRATION.md section 3, CLIP."""
    c = model.config
    act = {"quick_gelu": "quickgelu", "gelu": "gelu"}[c.hidden_act]
    cfg = synth.ModelConfig(img_size=c.image_size, patch_size=c.patch_size, in_chans=c.num_channels, num_classes=c.projection_dim,
                            embed_dim=c.hidden_size, depth=c.num_hidden_layers, num_heads=c.num_attention_heads,
                            hidden_dim=c.intermediate_size, mlp=act)
    sd = {k: v.detach().cpu().numpy().astype(np.float32) for k, v in model.state_dict().items()}
    vm, D = "vision_model.", c.hidden_size
    W = [sd[vm + "embeddings.class_embedding"], sd[vm + "embeddings.patch_embedding.weight"].reshape(D, -1),
         np.zeros(D, np.float32), sd[vm + "embeddings.position_embedding.weight"]]
    for l in range(c.num_hidden_layers):
        p = f"{vm}encoder.layers.{l}."
        W += [sd[p + "layer_norm1.weight"], sd[p + "layer_norm1.bias"],
              np.concatenate([sd[p + f"self_attn.{n}_proj.weight"] for n in "qkv"]),
              np.concatenate([sd[p + f"self_attn.{n}_proj.bias"] for n in "qkv"]),
              sd[p + "self_attn.out_proj.weight"], sd[p + "self_attn.out_proj.bias"],
              sd[p + "layer_norm2.weight"], sd[p + "layer_norm2.bias"],
              sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"], sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"]]
    W += [sd[vm + "post_layernorm.weight"], sd[vm + "post_layernorm.bias"], sd["visual_projection.weight"],
          np.zeros(c.projection_dim, np.float32)]
    return cfg, [np.ascontiguousarray(w) for w in W], (sd[vm + "pre_layrnorm.weight"], sd[vm + "pre_layrnorm.bias"]), float(c.layer_norm_eps)
