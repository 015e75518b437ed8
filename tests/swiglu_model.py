"""A ViT whose MLP is the fused SwiGLU block (Dinov2SwiGLUFFN of transformers, SwiGLUFFNFused of DINOv2), built from the oracle's own
ops: what an engine of the kind VIT_MLP_SWIGLU must reproduce.

    x = embed(image)
    per layer l:  x = x + ls1_l * multihead_attn(layer_norm(x, ln1), in_proj, out_proj)
                  u = linear(layer_norm(x, ln2), W12, b12)             W12 [2H][D]: tensors 4 + 12 l + 8, + 9 (the fc1 slots)
                  h = silu(u[:, :H]) * u[:, H:]                        float64 numpy, rounded once to fp32
                  x = x + ls2_l * linear(h, W3, b3)                    W3 [D][H]:   tensors 4 + 12 l + 10, + 11 (the fc2 slots)
    logits = linear(layer_norm(x)[0], head);  probs = softmax(logits)

chunk(2, dim=-1) of the reference modules puts the gate in the first H outputs of w12 and the value in the last H.  ls (2 * depth
vectors [dim], tests/layer_scale_model.py's order) is optional: None runs the block without LayerScale, which is also what a
checkpoint folded by vit_weights_fold_layer_scale is.  The return value has the shape of pyoracle.forward_image(..., want_stages=True):
(probs, logits, stages [depth + 1][tokens][dim]).
"""
import dataclasses

import numpy as np

from vit_amd import synth

# the reduced SwiGLU models the tests share (head_dim stays 64): a few hundred KB of weights
TINY_SG = dataclasses.replace(synth.VIT_TINY, hidden_dim=192, mlp="swiglu")    # 2H = 384: no power of two
SMALL_SG = dataclasses.replace(synth.VIT_SMALL, hidden_dim=512, mlp="swiglu")
# one layer at the full width of DINOv2 ViT-g/14: N = 8192, K = 4096, D = 1536 through the fold, the split image and both GEMM families
G14_LAYER = synth.ModelConfig(img_size=28, patch_size=14, num_classes=10, embed_dim=1536, depth=1, num_heads=24, hidden_dim=4096,
                              mlp="swiglu")


def gate(u, H):
    """h = silu(u[:, :H]) * u[:, H:2H] in float64, rounded once to fp32 (u: any float array [rows][>= 2H])."""
    u = np.asarray(u)
    g, v = u[:, :H].astype(np.float64), u[:, H:2 * H].astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return ((g / (1.0 + np.exp(-g))) * v).astype(np.float32)


def forward_image(oracle, ocfg, image, W, ls=None):
    H = ocfg.hidden_dim
    x = oracle.embed(ocfg, np.ascontiguousarray(image, np.float32), W)
    stages = [x]
    for l in range(ocfg.depth):
        w = [np.ascontiguousarray(t, np.float32) for t in W[4 + 12 * l:16 + 12 * l]]
        attn = oracle.multihead_attn(oracle.layer_norm(x, w[0], w[1]), w[2], w[3], w[4], w[5], ocfg.num_heads)
        x = (x + (attn if ls is None else ls[2 * l][None, :] * attn)).astype(np.float32)
        u = oracle.linear(oracle.layer_norm(x, w[6], w[7]), w[8].reshape(2 * H, -1), w[9])
        mlp = oracle.linear(np.ascontiguousarray(gate(u, H)), w[10].reshape(-1, H), w[11])
        x = (x + (mlp if ls is None else ls[2 * l + 1][None, :] * mlp)).astype(np.float32)
        stages.append(x)
    y = oracle.layer_norm(x, W[-4], W[-3])
    logits = oracle.linear(y[:1], np.ascontiguousarray(W[-2], np.float32).reshape(ocfg.num_classes, -1), W[-1])[0]
    return oracle.softmax(logits), logits, np.stack(stages)


def forward(oracle, ocfg, images, W, ls=None):
    """(probs [n][classes], logits [n][classes], stages [n][depth + 1][tokens][dim])."""
    out = [forward_image(oracle, ocfg, im, W, ls) for im in images]
    return tuple(np.stack([o[k] for o in out]) for k in range(3))
