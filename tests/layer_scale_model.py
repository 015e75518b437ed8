"""A ViT with LayerScale (DINOv2, CaiT), UNFOLDED, built from the oracle's own ops: what vit_weights_fold_layer_scale must reproduce.

    x = embed(image)
    per layer l:  x = x + ls1_l * multihead_attn(layer_norm(x, ln1), in_proj, out_proj)
                  x = x + ls2_l * mlp_block(layer_norm(x, ln2), fc1, fc2)
    logits = linear(layer_norm(x)[0], head);  probs = softmax(logits)

ls1_l / ls2_l scale the branch per channel ([dim]); the products and the sums are fp32 numpy operations.  The return value has the
shape of pyoracle.forward_image(..., want_stages=True): (probs, logits, stages [depth + 1][tokens][dim]).
"""
import numpy as np


def scales(cfg, seed, lo=0.05, hi=1.5):
    """2 * depth vectors [embed_dim], U(lo, hi): ls1 of layer 0, ls2 of layer 0, ls1 of layer 1, ..."""
    rng = np.random.default_rng(seed)
    return [rng.uniform(lo, hi, cfg.embed_dim).astype(np.float32) for _ in range(2 * cfg.depth)]


def forward_image(oracle, ocfg, image, W, ls):
    x = oracle.embed(ocfg, np.ascontiguousarray(image, np.float32), W)
    stages = [x]
    for l in range(ocfg.depth):
        w = [np.ascontiguousarray(t, np.float32) for t in W[4 + 12 * l:16 + 12 * l]]
        attn = oracle.multihead_attn(oracle.layer_norm(x, w[0], w[1]), w[2], w[3], w[4], w[5], ocfg.num_heads)
        x = (x + ls[2 * l][None, :] * attn).astype(np.float32)
        mlp = oracle.mlp_block(oracle.layer_norm(x, w[6], w[7]), w[8], w[9], w[10], w[11])
        x = (x + ls[2 * l + 1][None, :] * mlp).astype(np.float32)
        stages.append(x)
    y = oracle.layer_norm(x, W[-4], W[-3])
    logits = oracle.linear(y[:1], np.ascontiguousarray(W[-2], np.float32).reshape(ocfg.num_classes, -1), W[-1])[0]
    return oracle.softmax(logits), logits, np.stack(stages)
