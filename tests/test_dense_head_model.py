"""tests/dense_head_model.py against PyTorch, and the BatchNorm fold (vit_dense_head_fold_batchnorm) against its statement: no GPU.

Labels.  The model's values carry at most about 6 fp32 roundings of relative size 2^-24 each (two axis weights, two products, a
sum, again for the rows), about 3.6e-7 of max|logit|; PyTorch's CPU kernel rounds in another order, so two values can move against
each other by about 7.2e-7 of max|logit|.  Labels must therefore agree wherever the top-2 margin of PyTorch's interpolated logits
exceeds 1e-5 * max|logit|, more than 10x that.  (The weight l1 = src - i0 also inherits the rounding of src, half an ulp of a value
up to g: the test prints the largest difference between the two sets of values, 1.0e-6 of max|logit| at g = 37, a tenth of the
margin.)  At most 0.1 % of the pixels may fall under the margin: a condition on the inputs, asserted here, which the seeds below meet.
"""
import numpy as np
import pytest
import torch

import dense_head_model as M
from vit_amd import binding as B

# g, out_h, out_w, classes
SIZES = [(4, 64, 64, 21), (4, 37, 53, 21), (16, 224, 224, 150), (37, 74, 70, 19), (5, 5, 5, 3), (8, 3, 2, 3)]
SEEDS = {(4, 64, 64, 21): 1, (4, 37, 53, 21): 2, (16, 224, 224, 150): 3, (37, 74, 70, 19): 4, (5, 5, 5, 3): 5, (8, 3, 2, 3): 6}
NAN, INF = np.float32(np.nan), np.float32(np.inf)


def seeded_logits(g, classes, seed, n=None):
    rng = np.random.default_rng(seed)
    shape = (g * g, classes) if n is None else (n, g * g, classes)
    return rng.standard_normal(shape).astype(np.float32)


def torch_values(logits, g, out_h, out_w):
    """F.interpolate(bilinear, align_corners=False) of the [classes][g][g] maps -> float32 [out_h][out_w][classes]."""
    maps = torch.from_numpy(np.ascontiguousarray(logits.T).reshape(1, -1, g, g))
    up = torch.nn.functional.interpolate(maps, size=(out_h, out_w), mode="bilinear", align_corners=False)
    return up, up[0].permute(1, 2, 0).numpy()


@pytest.mark.parametrize("g,out_h,out_w,classes", SIZES)
def test_labels_agree_with_torch_interpolate_argmax_outside_the_margin(g, out_h, out_w, classes):
    logits = seeded_logits(g, classes, SEEDS[(g, out_h, out_w, classes)])
    up, vals = torch_values(logits, g, out_h, out_w)
    want = up.argmax(1)[0].numpy()
    got = M.labels(logits, g, out_h, out_w)
    assert got.dtype == np.uint8 and got.shape == (out_h, out_w)
    top2 = np.sort(vals, axis=-1)[..., -2:]
    margin = top2[..., 1] - top2[..., 0]
    clear = margin > 1e-5 * float(np.abs(logits).max())
    under = int((~clear).sum())
    print(f"g={g} out={out_h}x{out_w} classes={classes}: {under} of {clear.size} pixels under the margin, "
          f"{int((got != want).sum())} labels differ, max |dv| = {float(np.abs(M.upsample(logits, g, out_h, out_w) - vals).max()):.3e}")
    assert under <= clear.size // 1000, "the inputs do not meet the margin condition: pick another seed"
    assert np.array_equal(got[clear], want[clear].astype(np.uint8))


def test_axis_taps_are_the_stated_fp32_arithmetic():
    for g, out in ((4, 64), (16, 224), (37, 518), (8, 3), (5, 5), (1, 7), (37, 70)):
        i0, i1, l0, l1 = M.axis_taps(g, out)
        assert l0.dtype == l1.dtype == np.float32
        for d in range(out):
            scale = np.float32(g) / np.float32(out)
            src = np.float32(scale * np.float32(np.float32(d) + np.float32(0.5))) - np.float32(0.5)
            src = np.float32(0) if src < 0 else np.float32(src)
            assert i0[d] == int(src) and i1[d] == int(src) + (int(src) < g - 1)
            assert l1[d] == np.float32(src - np.float32(int(src))) and l0[d] == np.float32(np.float32(1) - l1[d])
        assert i0.min() >= 0 and i1.max() <= g - 1 and (np.diff(i0) >= 0).all() and (np.diff(i1) >= 0).all()
    i0, i1, l0, l1 = M.axis_taps(5, 5)  # the identity: every pixel is its own cell
    assert i0.tolist() == [0, 1, 2, 3, 4] and (l1 == 0).all() and (l0 == 1).all()


def test_equal_classes_give_the_lower_label():
    v = np.zeros((2, 3, 5), np.float32)
    assert (M.argmax_labels(v) == 0).all()
    v[..., 2] = v[..., 4] = 1.5
    assert (M.argmax_labels(v) == 2).all()
    v[..., 1] = -0.0
    v[..., 2] = v[..., 4] = 0.0   # -0.0 == 0.0: class 0 (0.0) ties all of them
    assert (M.argmax_labels(v) == 0).all()
    # through the interpolation too: two identical class maps
    logits = seeded_logits(4, 6, 11)
    logits[:, 1] = logits[:, 4] = logits.max() + 1
    assert (M.labels(logits, 4, 9, 7) == 1).all()


def test_a_nan_class_is_skipped_all_nan_gives_255_and_inf_wins():
    v = np.array([[0.5, NAN, 0.25], [NAN, NAN, NAN], [1.0, INF, 2.0], [-INF, NAN, -INF], [NAN, -INF, NAN], [INF, INF, NAN]], np.float32)
    assert M.argmax_labels(v).tolist() == [0, 255, 1, 0, 1, 0]
    g, classes = 4, 5
    logits = seeded_logits(g, classes, 12)
    logits[:, 3] = NAN                      # one NaN class: never chosen, the others as without it
    clean = np.delete(logits, 3, axis=1)
    got, ref = M.labels(logits, g, 16, 12), M.labels(clean, g, 16, 12)
    assert (got != 3).all() and np.array_equal(np.where(got > 3, got - 1, got), ref)
    assert (M.labels(np.full((g * g, classes), NAN, np.float32), g, 8, 8) == M.NO_LABEL).all()
    logits = seeded_logits(g, classes, 13)
    logits[:, 2] = INF                      # +Inf everywhere: l * Inf = Inf where l > 0, and 0 * Inf = NaN only beside a zero weight
    lab = M.labels(logits, g, 16, 16)
    vals = M.upsample(logits, g, 16, 16)[..., 2]
    assert np.array_equal(lab == 2, vals == INF) and (lab == 2).sum() > 0
    assert (lab[np.isnan(vals)] != 2).all()


# ---- the BatchNorm fold --------------------------------------------------------------------------------------------------------

def fold_inputs(classes, K, seed):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return f(classes, K), f(classes), (1 + 0.2 * f(K)).astype(np.float32), f(K), f(K), (0.5 + rng.random(K)).astype(np.float32)


@pytest.mark.parametrize("classes,K,eps", [(21, 192, 1e-5), (3, 7, 1e-3), (1, 1, 0.0), (150, 1536, 1e-5)])
def test_fold_is_bit_for_bit_the_stated_double_arithmetic(classes, K, eps):
    W, b, gamma, beta, mean, var = fold_inputs(classes, K, classes + K)
    want_w, want_b = M.fold_batchnorm(W, b, gamma, beta, mean, var, eps)
    got_w, got_b = B.fold_batchnorm(W, b, gamma, beta, mean, var, eps)
    assert got_w.dtype == got_b.dtype == np.float32 and got_w.shape == W.shape and got_b.shape == b.shape
    assert np.array_equal(got_w.view(np.uint32), want_w.view(np.uint32))
    assert np.array_equal(got_b.view(np.uint32), want_b.view(np.uint32))
    assert not np.shares_memory(got_w, W)   # the wrapper folds a copy; the raw call folds in place
    w2, b2 = W.copy(), b.copy()
    assert B.fold_batchnorm_raw(w2, b2, classes, K, gamma, beta, mean, var, eps) == 0
    assert np.array_equal(w2.view(np.uint32), want_w.view(np.uint32)) and np.array_equal(b2.view(np.uint32), want_b.view(np.uint32))


def test_fold_equals_torch_batchnorm_then_conv_within_the_fp32_rounding_of_the_result():
    classes, K, eps = 21, 96, 1e-5
    W, b, gamma, beta, mean, var = fold_inputs(classes, K, 5)
    bn = torch.nn.BatchNorm2d(K, eps=eps).double().eval()
    conv = torch.nn.Conv2d(K, classes, 1).double()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(gamma)); bn.bias.copy_(torch.from_numpy(beta))
        bn.running_mean.copy_(torch.from_numpy(mean)); bn.running_var.copy_(torch.from_numpy(var))
        conv.weight.copy_(torch.from_numpy(W).reshape(classes, K, 1, 1)); conv.bias.copy_(torch.from_numpy(b))
        x = torch.from_numpy(np.random.default_rng(6).standard_normal((1, K, 4, 4)))
        want = conv(bn(x))[0].permute(1, 2, 0).reshape(-1, classes).numpy()
    fw, fb = B.fold_batchnorm(W, b, gamma, beta, mean, var, eps)
    xs = x[0].permute(1, 2, 0).reshape(-1, K).numpy()
    got = xs @ fw.astype(np.float64).T + fb.astype(np.float64)
    # every folded weight and bias is the exact double value rounded once to fp32: a relative 2^-24 on each term of the sum
    bound = 2.0 ** -24 * (np.abs(xs) @ np.abs(fw.astype(np.float64)).T + np.abs(fb.astype(np.float64))) * 1.001 + 1e-13
    assert (np.abs(got - want) <= bound).all(), float((np.abs(got - want) / bound).max())


def test_a_refused_fold_leaves_every_byte_unchanged():
    classes, K = 4, 8
    W, b, gamma, beta, mean, var = fold_inputs(classes, K, 9)

    def refused(**bad):
        a = dict(weight=W.copy(), bias=b.copy(), classes=classes, in_features=K, gamma=gamma.copy(), beta=beta, mean=mean, var=var.copy(), eps=1e-5)
        a.update(bad)
        w0 = None if a["weight"] is None else a["weight"].copy()
        b0 = None if a["bias"] is None else a["bias"].copy()
        assert B.fold_batchnorm_raw(**a) != 0, bad
        assert w0 is None or np.array_equal(a["weight"].view(np.uint32), w0.view(np.uint32))
        assert b0 is None or np.array_equal(a["bias"].view(np.uint32), b0.view(np.uint32))

    refused(weight=None); refused(bias=None); refused(gamma=None); refused(beta=None); refused(mean=None); refused(var=None)
    refused(classes=0); refused(in_features=0); refused(classes=-1)
    refused(eps=-1e-5); refused(eps=float("nan")); refused(eps=float("inf"))
    g2 = gamma.copy(); g2[K - 1] = NAN
    refused(gamma=g2)
    v2 = var.copy(); v2[K - 1] = -1.0          # var + eps <= 0, found behind K - 1 good channels: nothing was written on the way
    refused(var=v2)
    v3 = var.copy(); v3[0] = 0.0
    refused(var=v3, eps=0.0)
    w2 = W.copy(); w2[classes - 1, K - 1] = INF
    refused(weight=w2)
    with pytest.raises(B.VitError):
        B.fold_batchnorm(W, b, gamma[:-1], beta[:-1], mean[:-1], var[:-1])
