"""A ViT / CLIP image tower of any head_dim in float64 numpy: tests/clip_model.py with hd = embed_dim // num_heads in place of 64.

    per head h:  q, k, v = columns hd*h .. hd*(h+1) of the Q, K, V thirds of in_proj's output
                 att[:, hd*h ..] = softmax(q k^T / sqrt(hd)) v

Everything else (patch rows, LayerNorm with one eps, the activations, the head slot, the weight order) is clip_model's, imported.
`score_dim` replaces hd under the square root only: what a kernel with sqrt(64) wired in would compute on the same tower.
tests/test_headdim_model.py pins this file to transformers.CLIPVisionModelWithProjection at head_dim 80 and 104.
"""
import math

import numpy as np

from clip_model import from_transformers, gelu, layer_norm, patches, quick_gelu  # noqa: F401  (from_transformers: re-exported)
from vit_amd import synth

# the reduced towers of the engine tests: D % 64 == 0 and hidden % 64 == 0, so every ln_fold / dtype combination is open
HD80 = synth.ModelConfig(img_size=28, patch_size=14, num_classes=40, embed_dim=320, depth=2, num_heads=4, hidden_dim=640)
HD72 = synth.ModelConfig(img_size=32, patch_size=8, num_classes=40, embed_dim=576, depth=2, num_heads=8, hidden_dim=576)
HD104 = synth.ModelConfig(img_size=32, patch_size=16, num_classes=40, embed_dim=832, depth=1, num_heads=8, hidden_dim=832)
HD128 = synth.ModelConfig(img_size=64, patch_size=16, num_classes=40, embed_dim=256, depth=2, num_heads=2, hidden_dim=512)
HD80_257 = synth.ModelConfig(img_size=224, patch_size=14, num_classes=40, embed_dim=320, depth=1, num_heads=4, hidden_dim=640)
# one layer at the full width of ViT-H/14: D 1280, 16 heads of 80, hidden 5120
H14_LAYER = synth.ModelConfig(img_size=28, patch_size=14, num_classes=64, embed_dim=1280, depth=1, num_heads=16, hidden_dim=5120)


def attention(qkv, heads, score_dim=None):
    """[T][3D] -> [T][D] and the heads' probabilities [heads][T][T]."""
    qkv = np.asarray(qkv, np.float64)
    D = qkv.shape[1] // 3
    hd = D // heads
    att, probs = np.empty((qkv.shape[0], D)), []
    for h in range(heads):
        q, k, v = (qkv[:, i * D + h * hd:i * D + (h + 1) * hd] for i in range(3))
        s = q @ k.T / math.sqrt(score_dim or hd)
        p = np.exp(s - s.max(-1, keepdims=True))
        p = p / p.sum(-1, keepdims=True)
        probs.append(p)
        att[:, h * hd:(h + 1) * hd] = p @ v
    return att, np.stack(probs)


def forward_image(cfg, image, W, pre=None, eps=1e-6, act="gelu", score_dim=None):
    """dict: embeds [NC] (the logits), probs [NC], unit [NC], stages [depth + 1][T][D] (stage 0: the stream layer 0 reads, behind the
    pre-norm), qkv_last [T][3D] (in_proj's output in the last layer)."""
    W = [np.asarray(w, np.float64) for w in W]
    D, H, heads = cfg.embed_dim, cfg.hidden_dim, cfg.num_heads
    f = {"quickgelu": quick_gelu, "gelu": gelu}[act]
    x = np.concatenate([W[0].reshape(1, D), patches(cfg, image) @ W[1].reshape(D, -1).T + W[2]]) + W[3].reshape(-1, D)
    if pre is not None:
        x = layer_norm(x, pre[0], pre[1], eps)
    stages, qkv = [x], None
    for l in range(cfg.depth):
        w = W[4 + 12 * l:16 + 12 * l]
        qkv = layer_norm(x, w[0], w[1], eps) @ w[2].reshape(3 * D, D).T + w[3]
        x = x + attention(qkv, heads, score_dim)[0] @ w[4].reshape(D, D).T + w[5]
        hid = f(layer_norm(x, w[6], w[7], eps) @ w[8].reshape(H, D).T + w[9])
        x = x + hid @ w[10].reshape(D, H).T + w[11]
        stages.append(x)
    embeds = layer_norm(x[0], W[-4], W[-3], eps) @ W[-2].reshape(cfg.num_classes, D).T + W[-1]
    e = np.exp(embeds - embeds.max())
    return {"embeds": embeds, "probs": e / e.sum(), "unit": embeds / max(float(np.linalg.norm(embeds)), 1e-12),
            "stages": np.stack(stages), "qkv_last": qkv}


def forward(cfg, images, W, pre=None, eps=1e-6, act="gelu", score_dim=None):
    out = [forward_image(cfg, im, W, pre, eps, act, score_dim) for im in images]
    return {k: np.stack([o[k] for o in out]) for k in out[0]}


def cls_attention_ref(qkv, n, T, heads, head_dim):
    """float64: the class token's softmax row per image and head, [n][heads][T], of qkv [n * T][3 * heads * head_dim]."""
    qkv = np.asarray(qkv, np.float64).reshape(n, T, 3, heads, head_dim)
    s = np.einsum("nhd,nthd->nht", qkv[:, 0, 0], qkv[:, :, 1]) / math.sqrt(head_dim)
    p = np.exp(s - s.max(-1, keepdims=True))
    return p / p.sum(-1, keepdims=True)
