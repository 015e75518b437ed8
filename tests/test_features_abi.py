"""Embedding outputs (vit_engine_features_*, vithip_layernorm_pool_f32): what can be checked without a GPU.

The exported symbols, the layout of vit_feature_spec against its ctypes mirror, vit_engine_options unchanged, and the numpy
restatement of the MEAN contract that the GPU tests compare the kernel with (tests/test_gpu_pool_kernel.py,
tests/test_gpu_features.py) -- pinned here to the oracle's LayerNorm, so that the reference of those tests is itself checked.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import oracle_config
from vit_amd import binding as B
from vit_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

POOL_REL = 2e-5  # "fp32 accumulation order only", the bar of tests/test_gpu_bf16.py for reordered fp32 sums


def layernorm_rows_f32(x, gamma, beta):
    """LayerNorm rows in fp32 by the kernels' formula: var = E[x^2] - mean^2, inv_std = 1 / sqrtf((double)var + 1e-6)."""
    x = np.asarray(x, np.float32)
    dim = np.float32(x.shape[-1])
    mean = x.sum(-1, dtype=np.float32, keepdims=True) / dim
    var = (x * x).sum(-1, dtype=np.float32, keepdims=True) / dim - mean * mean
    inv_std = np.float32(1.0) / np.sqrt((var.astype(np.float64) + 1e-6).astype(np.float32))
    return ((x - mean) * inv_std * np.asarray(gamma, np.float32) + np.asarray(beta, np.float32)).astype(np.float32)


def l2_normalize_f64(rows):
    """row / max(||row||_2, 1e-12) in float64 (torch.nn.functional.normalize)."""
    rows = np.asarray(rows, np.float64)
    return rows / np.maximum(np.sqrt((rows * rows).sum(-1, keepdims=True)), 1e-12)


def pool_reference(x, gamma, beta, images, tokens, first_tok=1, l2_normalize=False):
    """The MEAN contract: x [images * tokens][dim] -> float64 [images][dim], the mean over tokens first_tok.. of the fp32
    LayerNorm rows, accumulated in float64; optionally L2-normalised in float64."""
    y = layernorm_rows_f32(x, gamma, beta).reshape(images, tokens, -1)
    out = y[:, first_tok:].mean(1, dtype=np.float64)
    return l2_normalize_f64(out) if l2_normalize else out


def test_library_exports_the_feature_entry_points_and_the_pooling_launcher():
    syms = subprocess.run(["nm", "-D", "--defined-only", B.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
    for want in ("vit_engine_features_device", "vit_engine_features_host", "vit_engine_features_device_u8",
                 "vit_engine_features_host_u8", "vit_engine_feature_row_elems", "vithip_layernorm_pool_f32",
                 "vithip_layernorm_pool_f32_workspace_floats", "vithip_l2_normalize_rows_f32"):
        assert want in names, want


def test_feature_spec_mirror_has_the_layout_of_the_header_and_the_options_are_unchanged(tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "vit_engine.h"', "int main(void) {",
             '    printf("size %zu\\n", sizeof(vit_feature_spec));', '    printf("options %zu\\n", sizeof(vit_engine_options));',
             '    printf("kinds %d %d %d\\n", VIT_FEAT_CLS, VIT_FEAT_MEAN, VIT_FEAT_TOKENS);']
    for name, *_ in B.CFeatureSpec._fields_:
        lines.append(f'    printf("{name} %zu\\n", offsetof(vit_feature_spec, {name}));')
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "spec.c", tmp_path / "spec"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    out = {ln.split()[0]: ln.split()[1:] for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()}
    assert int(out["size"][0]) == C.sizeof(B.CFeatureSpec)
    for name, *_ in B.CFeatureSpec._fields_:
        assert int(out[name][0]) == getattr(B.CFeatureSpec, name).offset, name
    assert [int(v) for v in out["kinds"]] == [B.FEATURE_KINDS[k] for k in ("cls", "mean", "tokens")]
    # the choice of output is per call: vit_engine_options gained no field (12 ints before and after)
    assert int(out["options"][0]) == C.sizeof(B.COptions) == 12 * C.sizeof(C.c_int)


def test_workspace_query_counts_segments_of_sixteen_tokens():
    f = B.lib().vithip_layernorm_pool_f32_workspace_floats
    assert f(1, 197, 1, 768) == 13 * 768          # 196 patch tokens: 12 whole segments and one of 4
    assert f(256, 197, 0, 768) == 256 * 13 * 768  # 197 rows
    assert f(300, 2, 1, 64) == 300 * 64
    assert f(5, 577, 1, 1024) == 5 * 36 * 1024
    assert f(0, 197, 1, 768) == 0 and f(1, 1, 1, 768) == 0 and f(1, 5, -1, 64) == 0


def test_pool_restatement_agrees_with_the_oracle_layer_norm(oracle):
    """The reference of the GPU tests against the oracle: LayerNorm of the encoder output of VIT_TINY by pyoracle, float64 mean."""
    cfg = synth.VIT_TINY
    W = synth.make_weights(cfg, 21)
    ocfg = oracle_config(cfg)
    imgs = synth.make_images(cfg, 3, 105)
    for l2 in (False, True):
        for first_tok in (0, 1):
            x = np.stack([oracle.forward_image(ocfg, im, W, want_stages=True)[2][cfg.depth] for im in imgs])  # [n][T][D]
            y = np.stack([oracle.layer_norm(xi, W[-4], W[-3]) for xi in x])
            ref = y[:, first_tok:].mean(1, dtype=np.float64)
            if l2:
                ref = l2_normalize_f64(ref)
            got = pool_reference(x.reshape(-1, cfg.embed_dim), W[-4], W[-3], len(imgs), cfg.tokens, first_tok, l2)
            err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
            print(f"restatement vs oracle: first_tok={first_tok} l2={l2}: max |d| = {err:.3e} of {scale:.3e}")
            assert err <= POOL_REL * scale
    # and the class row of that tensor is what the oracle's classifier reads: its logits, bit for bit
    probs, logits, stages = oracle.forward_image(ocfg, imgs[0], W, want_stages=True)
    cls = oracle.layer_norm(stages[cfg.depth], W[-4], W[-3])[0:1]
    assert np.array_equal(oracle.linear(cls, W[-2], W[-1])[0], logits)


def test_pooling_scratch_always_fits_the_bf16_rows_it_replaces():
    """The engine takes the pooling scratch from a lane's own rows of y: n * T * D elements of 2 bytes on a bf16 engine.  One fp32
    [D] row per 16 patch tokens never needs more, for any token count from 2 up (host/vit_engine.c checks it per call as well)."""
    f = B.lib().vithip_layernorm_pool_f32_workspace_floats
    for tokens in list(range(2, 70)) + [197, 577, 1025, 4097]:
        for n, dim in ((1, 64), (3, 192), (7, 768), (2, 2048)):
            need = f(n, tokens, 1, dim) * 4
            assert 0 < need <= n * tokens * dim * 2, (n, tokens, dim, need)
