"""Pooled and multi-layer classifier heads (vit_engine_set_head), restated on the oracle's own ops.

`stages` is what pyoracle.forward_image(..., want_stages=True) returns for ONE image ([depth + 1][tokens][dim]; stages[l + 1] is the
residual stream behind encoder layer l) -- or, for a LayerScale model, what layer_scale_model.forward_image returns in its place.
With f = oracle.layer_norm with the final LayerNorm's gamma and beta, P = tokens - 1:

    operand = [ f(stages[l + 1][0]) for l in cls_layers | pooled ]
    pooled  = mean_t f(stages[-1][t]), t = 1..P          "avg"         norm, then mean (DINOv2 linear heads, timm global_pool='avg')
            = f(mean_t stages[-1][t])                    "avg_fcnorm"  mean, then norm (timm fc_norm)
    logits  = oracle.linear(operand, weight, bias)

The means are taken in float64 and rounded once: the reference carries no summation order of its own.
"""
import numpy as np

POOLS = ("none", "avg", "avg_fcnorm")


def families(depth):
    """The specs of vit_engine.h's table: name -> (cls_layers, pool).  The 4-layer head needs depth >= 4."""
    f = {"dinov2_1": ((depth - 1,), "avg"), "timm_avg": ((), "avg"), "timm_fcnorm": ((), "avg_fcnorm"), "probe": ((depth - 1,), "none")}
    if depth >= 4:
        f["dinov2_4"] = (tuple(range(depth - 4, depth)), "avg")
    return f


def in_features(dim, cls_layers, pool):
    return (len(cls_layers) + (pool != "none")) * dim


def operand(oracle, stages, gamma, beta, cls_layers, pool):
    """The head's operand row of one image, fp32 [in_features]."""
    assert pool in POOLS
    gamma, beta = np.ascontiguousarray(gamma, np.float32), np.ascontiguousarray(beta, np.float32)
    stages = np.ascontiguousarray(stages, np.float32)
    blocks = [oracle.layer_norm(np.ascontiguousarray(stages[l + 1][:1]), gamma, beta)[0] for l in cls_layers]
    last = np.ascontiguousarray(stages[-1])
    if pool == "avg":
        blocks.append(oracle.layer_norm(last, gamma, beta)[1:].mean(0, dtype=np.float64).astype(np.float32))
    elif pool == "avg_fcnorm":
        pooled = last[1:].mean(0, dtype=np.float64).astype(np.float32)
        blocks.append(oracle.layer_norm(np.ascontiguousarray(pooled[None]), gamma, beta)[0])
    return np.concatenate(blocks).astype(np.float32)


def operands(oracle, stages_per_image, gamma, beta, cls_layers, pool):
    return np.stack([operand(oracle, st, gamma, beta, cls_layers, pool) for st in stages_per_image])


def logits(oracle, rows, weight, bias):
    """rows [n][in_features] -> [n][num_classes] through the oracle's linear."""
    rows = np.ascontiguousarray(rows, np.float32)
    weight = np.ascontiguousarray(weight, np.float32).reshape(-1, rows.shape[1])
    return oracle.linear(rows, weight, np.ascontiguousarray(bias, np.float32))


def probs(oracle, lg):
    return np.stack([oracle.softmax(np.ascontiguousarray(r)) for r in lg])


def make_head(num_classes, width, seed):
    """A head's (weight [num_classes][width], bias): the scale of a trained linear layer, logits of a few units."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(-1.0, 1.0, (num_classes, width)).astype(np.float32) * np.float32(2.0 / np.sqrt(width))
    return w, rng.uniform(-0.5, 0.5, num_classes).astype(np.float32)
