"""The attention-pool head (vit_engine_set_map_head) in float64 numpy, UNFOLDED: q, k and v projections and a softmax per head, as
torch.nn.MultiheadAttention computes them -- so a mistake in the engine's fold (a_h = hd^-0.5 Wk_h^T q_h, V applied to the pooled
row) shows against it.  y: the final-LayerNorm tokens [n][keys][D] the head attends over; w: the tensors of binding.MAP_HEAD_TENSORS."""
import math

import numpy as np


def act(x, kind):
    if kind == "gelu":
        return 0.5 * x * (1.0 + np.vectorize(math.erf)(x / math.sqrt(2.0)))
    return 0.5 * x * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def attention(y, w, heads):
    """concat_h(sum_t p[h][t] v_t,h): [n][D], the rows out_proj reads."""
    y = np.asarray(y, np.float64)
    n, _, D = y.shape
    hd = D // heads
    W, b = np.asarray(w["in_proj_weight"], np.float64), np.asarray(w["in_proj_bias"], np.float64)
    q = (W[:D] @ np.asarray(w["probe"], np.float64).reshape(D) + b[:D]).reshape(heads, hd)
    k = (y @ W[D:2 * D].T + b[D:2 * D]).reshape(n, -1, heads, hd)
    v = (y @ W[2 * D:].T + b[2 * D:]).reshape(n, -1, heads, hd)
    s = np.einsum("hd,nthd->nht", q, k) / math.sqrt(hd)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return np.einsum("nht,nthd->nhd", p, v).reshape(n, D)


def layer_norm(a, g, b, eps):
    mu, var = a.mean(-1, keepdims=True), a.var(-1, keepdims=True)
    return (a - mu) / np.sqrt(var + eps) * np.asarray(g, np.float64) + np.asarray(b, np.float64)


def head(y, w, heads, kind="gelu", eps=1e-6):
    """The whole head: out = a + fc2(act(fc1(LayerNorm(a)))), a = Wo o + bo; without fc1 in w: out = a."""
    f = {k: np.asarray(v, np.float64) for k, v in w.items() if v is not None}
    a = attention(y, w, heads) @ f["out_proj_weight"].T + f["out_proj_bias"]
    if "fc1_weight" not in f:
        return a
    hid = act(layer_norm(a, f["ln_weight"], f["ln_bias"], eps) @ f["fc1_weight"].T + f["fc1_bias"], kind)
    return a + hid @ f["fc2_weight"].T + f["fc2_bias"]
