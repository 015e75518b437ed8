"""LayerScale folded into out_proj and fc2 on the host (vit_weights_fold_layer_scale, binding.fold_layer_scale).

CPU: the fold is one fp32 multiply per element, bit for bit numpy's; nothing else moves; a refused call writes nothing; the oracle on the
folded weights stays within 2e-6 (max |d| / max |ref| per stage) of the unfolded model built from the oracle's ops
(tests/layer_scale_model.py) -- ten times the 2.1e-7 measured when the fold was designed.
GPU: engines that loaded the folded weights against the unfolded model, at the forward bars of tests/test_gpu_forward.py and
tests/test_gpu_bf16.py: fp32 probabilities 1e-4 and rows 1e-3 relative; bf16 probabilities 2e-2 and the same top-1.  bf16 rows have
no project bar: they are held to 2e-2 of max |ref| (the probability figure taken relatively; a bf16 rounding is 2^-8 = 3.9e-3).
"""

import numpy as np
import pytest

import layer_scale_model as LS
from conftest import oracle_config
from patch14_model import SMALL14, TINY14
from vit_amd import binding as B
from vit_amd import synth

FOLD_REL = 2e-6
PROB_TOL, LOGIT_REL, BF16_PROB_TOL = 1e-4, 1e-3, 2e-2
BF16_ROW_REL = 2e-2
MODELS = {"tiny14": TINY14, "small14": SMALL14}
_cache = {}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def model(name):
    """(cfg, weights, scales, folded weights, two images)"""
    if name not in _cache:
        cfg = MODELS[name]
        W = synth.make_weights(cfg, 41)
        ls = LS.scales(cfg, 42)
        _cache[name] = (cfg, W, ls, B.fold_layer_scale(cfg, W, ls), synth.make_images(cfg, 2, 43))
    return _cache[name]


def unfolded(oracle, name):
    key = ("unfolded", name)
    if key not in _cache:
        cfg, W, ls, _, imgs = model(name)
        _cache[key] = [LS.forward_image(oracle, oracle_config(cfg), im, W, ls) for im in imgs]
    return _cache[key]


@pytest.mark.parametrize("name", list(MODELS))
def test_fold_is_one_fp32_multiply_per_element_and_moves_nothing_else(name):
    cfg, W, ls, folded, _ = model(name)
    assert len(folded) == cfg.n_weights
    touched = set()
    for l in range(cfg.depth):
        for s, (wi, bi) in zip((ls[2 * l], ls[2 * l + 1]), ((4 + 12 * l + 4, 4 + 12 * l + 5), (4 + 12 * l + 10, 4 + 12 * l + 11))):
            assert np.array_equal(bits(folded[wi]), bits(np.float32(s)[:, None] * W[wi])), (l, wi)
            assert np.array_equal(bits(folded[bi]), bits(np.float32(s) * W[bi])), (l, bi)
            assert not np.array_equal(bits(folded[wi]), bits(W[wi]))
            touched |= {wi, bi}
    assert len(touched) == 4 * cfg.depth
    for i in range(cfg.n_weights):
        if i not in touched:
            assert folded[i].shape == W[i].shape and np.array_equal(bits(folded[i]), bits(W[i])), i
    # in place through the raw call: the same bits, the scales unchanged
    own, own_ls = [w.copy() for w in W], [s.copy() for s in ls]
    assert B.fold_layer_scale_raw(cfg, own, own_ls) == 0
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(own, folded))
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(own_ls, ls))


def test_every_refused_call_leaves_all_bytes_unchanged():
    cfg, W, ls, _, _ = model("tiny14")
    D = cfg.embed_dim
    base_w, base_s = [w.copy() for w in W], [s.copy() for s in ls]

    def with_(lst, i, value):
        out = list(lst)
        out[i] = value
        return out

    def poisoned(a, value):
        a = a.copy()
        a.reshape(-1)[a.size // 2] = value
        return a

    out_w, fc2_b, ln_w = 4 + 4, 4 + 12 + 11, 4 + 6
    cases = {
        "NULL weights": dict(weights=None, count=cfg.n_weights),
        "NULL scales": dict(scales=None, scale_count=2 * cfg.depth),
        "one tensor short": dict(count=cfg.n_weights - 1),
        "one tensor more": dict(weights=base_w + [base_w[-1].copy()]),
        "one scale short": dict(scale_count=2 * cfg.depth - 1),
        "one scale more": dict(scales=base_s + [base_s[-1].copy()]),
        "depth scales": dict(scales=base_s[:cfg.depth]),
        "out_proj weight absent": dict(weights=with_(base_w, out_w, None)),
        "a LayerNorm weight absent": dict(weights=with_(base_w, ln_w, None)),
        "fc2 bias of the wrong size": dict(weights=with_(base_w, fc2_b, np.zeros(D + 1, np.float32))),
        "out_proj weight of the wrong size": dict(weights=with_(base_w, out_w, np.zeros((D, D - 1), np.float32))),
        "position embedding of another grid": dict(weights=with_(base_w, 3, np.zeros((cfg.tokens + 1, D), np.float32))),
        "NaN in fc2 bias": dict(weights=with_(base_w, fc2_b, poisoned(base_w[fc2_b], np.nan))),
        "Inf in out_proj weight": dict(weights=with_(base_w, out_w, poisoned(base_w[out_w], np.inf))),
        "Inf in the last tensor": dict(weights=with_(base_w, cfg.n_weights - 1, poisoned(base_w[-1], -np.inf))),
        "scale absent": dict(scales=with_(base_s, 1, None)),
        "scale of the wrong size": dict(scales=with_(base_s, 2, np.ones(D - 1, np.float32))),
        "NaN in the last scale": dict(scales=with_(base_s, 2 * cfg.depth - 1, poisoned(base_s[-1], np.nan))),
        "Inf in the first scale": dict(scales=with_(base_s, 0, poisoned(base_s[0], np.inf))),
    }
    for name, kw in cases.items():
        w, s = kw.get("weights", base_w), kw.get("scales", base_s)
        before = [None if a is None else a.tobytes() for a in (w or [])], [None if a is None else a.tobytes() for a in (s or [])]
        rc = B.fold_layer_scale_raw(cfg, w, s, kw.get("count"), kw.get("scale_count"))
        assert rc != 0, name
        after = [None if a is None else a.tobytes() for a in (w or [])], [None if a is None else a.tobytes() for a in (s or [])]
        assert before == after, name
    # a NULL config, and the wrapper's error for a refused call
    w_arr, _kw = B.networks_from(base_w)
    s_arr, _ks = B.networks_from(base_s)
    assert B.lib().vit_weights_fold_layer_scale(None, w_arr, cfg.n_weights, s_arr, 2 * cfg.depth) != 0
    with pytest.raises(B.VitError, match="refused"):
        B.fold_layer_scale(cfg, base_w, base_s[:-1])
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(base_w, W))  # nothing above wrote through
    assert B.fold_layer_scale_raw(cfg, base_w, base_s) == 0                    # and the untouched set still folds


@pytest.mark.parametrize("name", list(MODELS))
def test_oracle_on_folded_weights_matches_the_unfolded_model(oracle, name):
    cfg, _, _, folded, imgs = model(name)
    ocfg = oracle_config(cfg)
    worst = 0.0
    for im, (ref_p, ref_l, ref_st) in zip(imgs, unfolded(oracle, name)):
        probs, logits, stages = oracle.forward_image(ocfg, im, folded, want_stages=True)
        for l in range(cfg.depth + 1):
            err = float(np.abs(stages[l].astype(np.float64) - ref_st[l]).max()) / float(np.abs(ref_st[l]).max())
            worst = max(worst, err)
            assert err <= FOLD_REL, (name, l, err)
        assert np.array_equal(bits(stages[0]), bits(ref_st[0]))  # the embedding knows nothing of the scales
        assert float(np.abs(logits - ref_l).max()) <= FOLD_REL * float(np.abs(ref_l).max())
        assert float(np.abs(probs - ref_p).max()) <= FOLD_REL
    print(f"{name}: folded against unfolded, worst stage max |d| / max |ref| = {worst:.3e}")
    assert worst > 0.0  # the fold moves roundings: two different computations were compared


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", list(MODELS))
def test_engine_with_folded_weights_matches_the_unfolded_model(oracle, name, dtype):
    cfg, _, _, folded, imgs = model(name)
    ref = unfolded(oracle, name)
    ref_p = np.stack([r[0] for r in ref])
    ref_rows = np.stack([oracle.layer_norm(r[2][cfg.depth], folded[-4], folded[-3]) for r in ref])
    eng = B.Engine(cfg, max_batch=4, dtype=dtype)
    try:
        eng.load_weights(folded)
        probs, rows = eng.forward(imgs), eng.features(imgs, "tokens")
    finally:
        eng.close()
    perr = float(np.abs(probs - ref_p).max())
    rerr = float(np.abs(rows - ref_rows).max()) / float(np.abs(ref_rows).max())
    print(f"{dtype} {name} folded LayerScale: max |dprob| = {perr:.3e}, last-layer tokens max |d| / max |ref| = {rerr:.3e}")
    assert perr <= (PROB_TOL if dtype == "f32" else BF16_PROB_TOL)
    assert (probs.argmax(1) == ref_p.argmax(1)).all()
    assert rerr <= (LOGIT_REL if dtype == "f32" else BF16_ROW_REL)
