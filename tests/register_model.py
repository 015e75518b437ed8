"""A ViT with register tokens (DINOv2 `_reg4`, "Vision Transformers Need Registers") in float64 numpy: tests/headdim_model.py's
forward with the prefix rows inserted as transformers' Dinov2WithRegistersEmbeddings does it,

    x[0]         = prefix[0] + pos[0]                         the class token
    x[1 + r]     = prefix[1 + r]                r = 0..R-1    the register tokens: no position embedding
    x[1 + R + p] = conv_b + patch_p . conv_w + pos[1 + p]     the patch tokens

W[0] is the prefix [(1 + R)][D] (class token first, then the checkpoint's register_tokens in their order), W[3] the position
embedding [(P + 1)][D]; everything behind the embedding is headdim_model's, imported.  No output counts the registers among "the
patch tokens": the pooled operand is [cls | mean of rows 1 + R ..] of the normalised last stage, the maps are rows 1 + R ...
tests/test_register_model.py pins this file to transformers.Dinov2WithRegistersForImageClassification / ...Backbone.
"""
import numpy as np

from headdim_model import attention, cls_attention_ref, gelu, layer_norm, patches  # noqa: F401  (cls_attention_ref: re-exported)
from vit_amd import synth

# the reduced models of the engine tests: head_dim 64; D % 64 == 0 and hidden % 64 == 0, so every ln_fold / dtype combination is open
REG_TINY = synth.ModelConfig(img_size=28, patch_size=14, num_classes=10, embed_dim=128, depth=2, num_heads=2, hidden_dim=512,
                             num_register_tokens=4)  # T = 9
REG_SMALL = synth.ModelConfig(img_size=56, patch_size=14, num_classes=40, embed_dim=192, depth=3, num_heads=3, hidden_dim=768,
                              num_register_tokens=4)  # T = 21
REG_ODD = synth.ModelConfig(img_size=42, patch_size=14, num_classes=10, embed_dim=128, depth=2, num_heads=2, hidden_dim=256,
                            num_register_tokens=1)  # T = 11, img % 4 == 2
REG_16 = synth.ModelConfig(img_size=64, patch_size=16, num_classes=40, embed_dim=128, depth=2, num_heads=2, hidden_dim=512,
                           num_register_tokens=4)  # T = 21: the 16-byte gather and the bf16 patch-row GEMM
REG_261 = synth.ModelConfig(img_size=224, patch_size=14, num_classes=40, embed_dim=128, depth=1, num_heads=2, hidden_dim=256,
                            num_register_tokens=4)  # T = 261: the sequence length of the published checkpoints at 224


def embed(cfg, image, W):
    """[T][D]: the stream layer 0 reads."""
    D, R = cfg.embed_dim, cfg.num_register_tokens
    prefix, pos = np.asarray(W[0], np.float64).reshape(1 + R, D), np.asarray(W[3], np.float64).reshape(cfg.patches + 1, D)
    rows = patches(cfg, image) @ np.asarray(W[1], np.float64).reshape(D, -1).T + np.asarray(W[2], np.float64)
    return np.concatenate([prefix[:1] + pos[:1], prefix[1:], rows + pos[1:]])


def forward_image(cfg, image, W, eps=1e-6, registers_in_mean=False):
    """dict: stages [depth + 1][T][D], norm [T][D] (the final LayerNorm of every row of the last stage), qkv_last [T][3D], logits
    [NC] and probs [NC] of the checkpoint's own head over norm[0], operand [2D] = [norm[0] | mean of norm[1 + R ..]] (the linear
    head's input), fcnorm [D] = LayerNorm(mean of stages[-1][1 + R ..]).  registers_in_mean: the wrong reading, the mean over rows
    1 .. -- what an engine that took the registers for patches would pool."""
    W = [np.asarray(w, np.float64) for w in W]
    D, H, heads, R = cfg.embed_dim, cfg.hidden_dim, cfg.num_heads, cfg.num_register_tokens
    x = embed(cfg, image, W)
    stages, qkv = [x], None
    for l in range(cfg.depth):
        w = W[4 + 12 * l:16 + 12 * l]
        qkv = layer_norm(x, w[0], w[1], eps) @ w[2].reshape(3 * D, D).T + w[3]
        x = x + attention(qkv, heads)[0] @ w[4].reshape(D, D).T + w[5]
        hid = gelu(layer_norm(x, w[6], w[7], eps) @ w[8].reshape(H, D).T + w[9])
        x = x + hid @ w[10].reshape(D, H).T + w[11]
        stages.append(x)
    norm = layer_norm(x, W[-4], W[-3], eps)
    first = 1 if registers_in_mean else 1 + R
    logits = norm[0] @ W[-2].reshape(cfg.num_classes, D).T + W[-1]
    e = np.exp(logits - logits.max())
    return {"stages": np.stack(stages), "norm": norm, "qkv_last": qkv, "logits": logits, "probs": e / e.sum(),
            "operand": np.concatenate([norm[0], norm[first:].mean(0)]),
            "fcnorm": layer_norm(x[first:].mean(0), W[-4], W[-3], eps)}


def forward(cfg, images, W, eps=1e-6, registers_in_mean=False):
    out = [forward_image(cfg, im, W, eps, registers_in_mean) for im in images]
    return {k: np.stack([o[k] for o in out]) for k in out[0]}


def patch_map(cfg, rows):
    """[T][D] rows -> [D][g][g]: the patch rows 1 + R .. as a channel-major raster (Dinov2WithRegistersBackbone's feature map)."""
    g = cfg.img_size // cfg.patch_size
    return np.asarray(rows)[1 + cfg.num_register_tokens:].T.reshape(-1, g, g)
