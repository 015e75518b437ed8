"""Engines with mxfp8 = 1 (QKV, out_proj, fc1, fc2 of every layer through vithip_gemm_mxfp8) against the float64 forward of
tests/mxfp8_model.py: embed 128, 2 heads, 2 layers, hidden 256, 144 px / patch 16 (T = 82), 5 images, features("cls").

    ref   the float64 forward;   qref  the same with both operands of the four linears quantised (quantize_mx)
    e_q = rel_err(qref, ref)     the format's own cost, on the CPU
    e_b = rel_err(bf16 engine with ln_fold = -1, ref)   code the parent commit runs

Bar: rel_err(mxfp8 engine, ref) <= 2 e_q + 2 e_b -- bf16-level differences upstream flip individual fp8 roundings, which adds noise
of the order of the quantisation noise itself.  Measured: profiles/r38/mxfp8.md."""
import functools

import numpy as np
import pytest

from engine_helpers import same_bits
from mxfp8_model import forward_cls, quantize_both
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu
VIT_ERR_ARG, N = 1, 5
CFG = synth.ModelConfig(img_size=144, patch_size=16, num_classes=10, embed_dim=128, depth=2, num_heads=2, hidden_dim=256)


def rel_err(got, ref) -> float:
    return float(np.abs(got - ref).max()) / float(np.abs(ref).max())


def cls_rows(W, imgs, **opt):
    eng = B.Engine(CFG, max_batch=8, dtype="bf16", **opt)
    try:
        eng.load_weights(W)
        first = eng.features(imgs, "cls")
        eng.load_weights(W)   # a second install makes the same images
        assert same_bits(eng.features(imgs, "cls"), first)
        return first
    finally:
        eng.close()


@functools.lru_cache(None)
def reference():
    """Once: (W, images, ref, the bar 2 e_q + 2 e_b, the bf16 engine's rows)"""
    W, imgs = synth.make_weights(CFG, seed=38), synth.make_images(CFG, N, 39)
    ref = forward_cls(CFG, W, imgs)
    bf16 = cls_rows(W, imgs, ln_fold=-1)
    e_q, e_b = rel_err(forward_cls(CFG, W, imgs, quantize_both), ref), rel_err(bf16, ref)
    print(f"e_q = {e_q:.3e} (format, CPU), e_b = {e_b:.3e} (bf16 engine, ln_fold = -1)")
    return W, imgs, ref, 2 * e_q + 2 * e_b, bf16


@pytest.mark.parametrize("pruned", [False, True], ids=["full", "pruned"])
def test_class_rows_within_the_formats_cost_and_not_the_bf16_engines_bits(pruned):
    W, imgs, ref, bar, bf16 = reference()
    got = cls_rows(W, imgs, mxfp8=1, prune_last_layer=pruned)
    err = rel_err(got, ref)
    print(f"mxfp8 engine, pruned = {pruned}: {err:.3e} of max |ref|, bar {bar:.3e}")
    assert err <= bar
    assert not same_bits(got, bf16)


@pytest.mark.parametrize("cfg, opt", [(CFG, dict(dtype="f32")), (CFG, dict(dtype="bf16", ln_fold=1)),
                                      (synth.ModelConfig(img_size=64, patch_size=16, num_classes=10, embed_dim=96, depth=1, num_heads=1, hidden_dim=256),
                                       dict(dtype="bf16"))], ids=["fp32", "ln_fold=1", "embed_dim=96"])
def test_create_refuses(cfg, opt):
    with pytest.raises(B.VitError) as refused:
        B.Engine(cfg, max_batch=4, mxfp8=1, **opt)
    assert refused.value.code == VIT_ERR_ARG
