"""Class-token attention maps (vit_engine_cls_attention_*, vithip_cls_attention_*): what can be checked without a GPU.

The exported symbols, the layout of vit_attention_spec against its ctypes mirror, vit_engine_options and vit_feature_spec unchanged,
and the numpy restatement of the contract that the GPU tests compare kernel and engine with (tests/test_gpu_cls_attention.py) --
pinned here to the oracle's attention, so that the reference of those tests is itself checked.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from conftest import oracle_config
from vit_amd import binding as B
from vit_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cls_attention_ref(qkv, T, heads, q_scaled=False):
    """The contract in float64: qkv [n * T][3 * heads * 64], columns [Q | K | V] -> p [n][heads][T], the softmax row of query 0:
    s_t = (q . k_t) / sqrtf(64), p_t = exp(s_t - max) / sum exp(s_t - max).  q_scaled: the Q columns hold QSCALE * q and
    p_t = 2^(q . k_t - max) / sum."""
    qkv = np.asarray(qkv, np.float64)
    n = qkv.shape[0] // T
    assert qkv.shape == (n * T, 3 * heads * 64)
    r = qkv.reshape(n, T, 3, heads, 64)
    s = np.einsum("nhd,nthd->nht", r[:, 0, 0], r[:, :, 1])
    if not q_scaled:
        s = s / 8.0  # sqrtf(64)
    s = s - s.max(-1, keepdims=True)
    e = np.exp2(s) if q_scaled else np.exp(s)
    return e / e.sum(-1, keepdims=True)


def head_mean_ref(p):
    """[n][heads][T] float64 -> [n][T]: the mean over the heads."""
    return np.asarray(p, np.float64).mean(1)


def oracle_last_qkv(oracle, cfg, image, W):
    """[T][3D] fp32: what the oracle's last encoder layer multiplies: in_proj of the LayerNorm of its input, by the oracle's own
    functions."""
    stages = oracle.forward_image(oracle_config(cfg), image, W, want_stages=True)[2]
    lw = W[4 + 12 * (cfg.depth - 1):]
    return oracle.linear(oracle.layer_norm(stages[cfg.depth - 1], lw[0], lw[1]), lw[2], lw[3])


def oracle_cls_attention(oracle, cfg, images, W):
    """[n][heads][T] float64: the restatement on the oracle's last-layer q and k."""
    return np.concatenate([cls_attention_ref(oracle_last_qkv(oracle, cfg, im, W), cfg.tokens, cfg.num_heads) for im in images])


def test_library_exports_the_attention_entry_points_and_the_launchers():
    syms = subprocess.run(["nm", "-D", "--defined-only", B.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
    for want in ("vit_engine_attention_row_elems", "vit_engine_cls_attention_device", "vit_engine_cls_attention_host",
                 "vit_engine_cls_attention_device_u8", "vit_engine_cls_attention_host_u8", "vit_engine_cls_attention_device_images",
                 "vit_engine_cls_attention_host_images", "vithip_cls_attention_f32", "vithip_cls_attention_bf16"):
        assert want in names, want


def test_attention_spec_mirror_has_the_layout_of_the_header_and_nothing_else_moved(tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "vit_engine.h"', "int main(void) {",
             '    printf("size %zu\\n", sizeof(vit_attention_spec));', '    printf("options %zu\\n", sizeof(vit_engine_options));',
             '    printf("feature %zu\\n", sizeof(vit_feature_spec));', '    printf("kinds %d %d\\n", VIT_ATTN_HEADS, VIT_ATTN_HEAD_MEAN);']
    for name, *_ in B.CAttentionSpec._fields_:
        lines.append(f'    printf("{name} %zu\\n", offsetof(vit_attention_spec, {name}));')
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "spec.c", tmp_path / "spec"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    out = {ln.split()[0]: ln.split()[1:] for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()}
    assert int(out["size"][0]) == C.sizeof(B.CAttentionSpec) == 8
    assert [name for name, *_ in B.CAttentionSpec._fields_] == ["kind", "reserved"]
    for name, *_ in B.CAttentionSpec._fields_:
        assert int(out[name][0]) == getattr(B.CAttentionSpec, name).offset, name
    assert [int(v) for v in out["kinds"]] == [0, 1] == [B.ATTENTION_KINDS[k] for k in ("heads", "head_mean")]
    # the choice of output is per call and has its own spec: the options (12 ints) and the feature spec are what they were
    assert int(out["options"][0]) == C.sizeof(B.COptions) == 12 * C.sizeof(C.c_int)
    assert int(out["feature"][0]) == C.sizeof(B.CFeatureSpec) == 8


def test_restatement_is_the_first_row_of_the_oracle_attention(oracle):
    """sum_t p[h][t] * V[t][64h..] must be row 0 of the oracle's attention_core on the same q, k, v: the restatement is the
    reference's softmax row (ViT_seq.c:156-190), shown with oracle functions only."""
    for cfg, seed in ((synth.VIT_TINY, 105), (synth.VIT_SMALL, 106)):
        W = synth.make_weights(cfg, 21)
        image = synth.make_images(cfg, 1, seed)[0]
        T, D, heads = cfg.tokens, cfg.embed_dim, cfg.num_heads
        qkv = oracle_last_qkv(oracle, cfg, image, W)
        assert qkv.shape == (T, 3 * D)
        q, k, v = (np.ascontiguousarray(qkv[:, i * D:(i + 1) * D]) for i in range(3))
        ref = oracle.attention_core(q, k, v, heads)[0].astype(np.float64)
        p = cls_attention_ref(qkv, T, heads)[0]  # [heads][T]
        assert p.shape == (heads, T) and float(np.abs(p.sum(-1) - 1.0).max()) <= 1e-12
        got = np.concatenate([p[h] @ v[:, 64 * h:64 * h + 64].astype(np.float64) for h in range(heads)])
        err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
        print(f"restatement vs oracle attention_core row 0: max |d| = {err:.3e} of {scale:.3e}")
        assert err <= 1e-6 * scale
        assert float((p.max(-1) - p.min(-1)).min()) > 1e-3  # no head's row is the uniform 1 / T
        assert np.allclose(head_mean_ref(p[None])[0], p.sum(0) / heads, rtol=0, atol=1e-15)


def test_q_scaled_restatement_is_the_plain_one_on_scaled_queries():
    rng = np.random.default_rng(3)
    T, heads = 9, 2
    qkv = rng.standard_normal((2 * T, 3 * heads * 64))
    scaled = qkv.copy()
    scaled[:, :heads * 64] *= B.QSCALE
    d = np.abs(cls_attention_ref(scaled, T, heads, q_scaled=True) - cls_attention_ref(qkv, T, heads)).max()
    assert float(d) <= 1e-9  # QSCALE is (1 / 8) * log2(e) rounded to fp32: 3e-8 relative on scores of a few units
