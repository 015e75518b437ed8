"""What the CLIP image-tower support adds to the ABI, checked without a GPU: the enum values, the exported symbols, vit_config's size,
the MLP kind VIT_MLP_QUICKGELU through the packing macros and the binding, the cache file of a QuickGELU model (version 3, the kind in
the eighth header word; a version-3 file loads only under its own kind), and vit_engine_create's answer to the kinds that stay refused (2 among them)."""
import ctypes as C
import dataclasses
import os
import struct
import subprocess

import numpy as np
import pytest

from clip_model import SMALL_CLIP, TINY_CLIP
from vit_amd import binding as B
from vit_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIT_ERR_ARG = 1
GELU_TWIN = dataclasses.replace(TINY_CLIP, mlp="gelu")
# the same eight dimensions as a SwiGLU model: fc1 has 2H rows there, so the sizes differ; H is halved to make the FILE sizes differ too
SWIGLU_TWIN = dataclasses.replace(TINY_CLIP, mlp="swiglu")


def compiled(tmp_path, body, fmt_count):
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text("\n".join(["#include <stdio.h>", "#include <stddef.h>", '#include "vit_types.h"', '#include "vit_engine.h"',
                              '#include "vit_hip_kernels.h"', "int main(void) {"] + body + ["    return 0;", "}"]))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert len(out) == fmt_count
    return out


def test_enum_values_and_the_kind_in_hidden_dim(tmp_path):
    out = compiled(tmp_path, [
        "    vit_config b16 = {224, 16, 3, 512, 768, 12, 12, VIT_HIDDEN_DIM_OF(3072, VIT_MLP_QUICKGELU)};",
        '    printf("%d %d %d %d %d %d %d ", VIT_MLP_GELU, VIT_MLP_SWIGLU, VIT_MLP_QUICKGELU, VIT_FEAT_CLS, VIT_FEAT_MEAN, VIT_FEAT_TOKENS, VIT_FEAT_HEAD);',
        '    printf("%d %d %d %d %d %d %d %d ", VITHIP_EPI_BIAS, VITHIP_EPI_BIAS_GELU, VITHIP_EPI_BIAS_RESIDUAL, VITHIP_EPI_BIAS_QGELU,',
        "           VITHIP_BF16_EPI_BF16, VITHIP_BF16_EPI_BF16_GELU, VITHIP_BF16_EPI_F32_RESIDUAL, VITHIP_BF16_EPI_BF16_QGELU);",
        '    printf("%zu %d %d %d %d %.17g\\n", sizeof(vit_config), b16.hidden_dim, VIT_MLP_KIND(&b16), VIT_HIDDEN_DIM(&b16), VIT_FC1_ROWS(&b16), VITHIP_LN_EPS);',
    ], 21)
    assert list(map(int, out[:7])) == [0, 1, 3, 0, 1, 2, 4]     # MLP kind 2 and feature kind 3 stay unassigned: refused, as callers know them
    assert list(map(int, out[7:15])) == [0, 1, 2, 6, 0, 1, 2, 4]
    assert (B.EPI_BIAS_QGELU, B.BF16_EPI_BF16_QGELU, B.FEATURE_KINDS["head"], synth.MLP_CODES["quickgelu"]) == (6, 4, 4, 3)
    size, hidden, kind, width, fc1_rows = map(int, out[15:20])
    assert size == C.sizeof(B.CConfig) == 8 * C.sizeof(C.c_int)             # unchanged: the kind travels in hidden_dim
    assert (hidden, kind, width, fc1_rows) == (3072 | (3 << 24), 3, 3072, 3072)   # fc1 keeps H rows
    assert float(out[20]) == 1e-6                                            # the double, exactly
    assert B.CConfig.of(synth.CLIP_B16).hidden_dim == hidden and synth.CLIP_B16.fc1_rows == 3072
    assert B.CConfig.of(TINY_CLIP).hidden_dim == TINY_CLIP.hidden_dim | (3 << 24)


def test_the_presets_are_openai_clip_b16_and_l14():
    b, l = synth.CLIP_B16, synth.CLIP_L14
    assert (b.img_size, b.patch_size, b.embed_dim, b.depth, b.num_heads, b.hidden_dim, b.num_classes, b.mlp) == (224, 16, 768, 12, 12, 3072, 512, "quickgelu")
    assert (l.img_size, l.patch_size, l.embed_dim, l.depth, l.num_heads, l.hidden_dim, l.num_classes, l.mlp) == (224, 14, 1024, 24, 16, 4096, 768, "quickgelu")
    assert b.tokens == 197 and l.tokens == 257 and b.weight_shapes()[12] == (3072, 768) and l.weight_shapes()[-2] == (768, 1024)
    # the layout and the MAC count of the GELU model of the same dimensions
    assert b.weight_shapes() == dataclasses.replace(b, mlp="gelu").weight_shapes()
    L = B.lib()
    for cfg in (b, l, TINY_CLIP, SMALL_CLIP):
        cc, cg = B.CConfig.of(cfg), B.CConfig.of(dataclasses.replace(cfg, mlp="gelu"))
        assert [L.vit_config_weight_size(C.byref(cc), i) for i in range(cfg.n_weights)] == [int(np.prod(s)) for s in cfg.weight_shapes()]
        assert L.vit_config_macs_per_image(C.byref(cc)) == L.vit_config_macs_per_image(C.byref(cg)) == cfg.macs_per_image


def test_library_exports_the_new_entry_points():
    syms = subprocess.run(["nm", "-D", "--defined-only", B.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
    want = {"vit_engine_set_layernorm_eps", "vit_engine_get_layernorm_eps", "vit_engine_set_pre_norm"}
    old = ["vithip_layernorm_f32", "vithip_layernorm_f32_bf16out", "vithip_rowstats_f32", "vithip_rowstats_bf16", "vithip_rowstats_finalize",
           "vithip_rowstats_finalize_f32", "vithip_layernorm_pool_f32", "vithip_pool_layernorm_f32", "vithip_tap_f32"]
    want |= set(old) | {n + "_eps" for n in old}     # one convention: every sibling is <name>_eps
    assert want <= names, sorted(want - names)


def file_header(path):
    head = open(path, "rb").read(48)
    magic, version = struct.unpack("<II", head[:8])
    assert magic == 0x57544956
    return version, struct.unpack("<8i", head[16:48])


def test_cache_file_version_and_kind(tmp_path):
    qg, gelu = TINY_CLIP, GELU_TWIN
    Wq = synth.make_weights(qg, 5, native=False)
    img_q, img_g = B.WeightImage.build(qg, Wq), B.WeightImage.build(gelu, Wq)      # the same tensors: only the kind differs
    p_q, p_g = str(tmp_path / "qg.cache"), str(tmp_path / "gelu.cache")
    assert img_q.save(p_q) == 0 and img_g.save(p_g) == 0
    vq, dq = file_header(p_q)
    vg, dg = file_header(p_g)
    assert (vg, vq) == (2, 3)
    assert dg[7] == qg.hidden_dim and dq[7] == qg.hidden_dim | (3 << 24) and dq[:7] == dg[:7]
    assert open(p_q, "rb").read()[80:] == open(p_g, "rb").read()[80:]            # and the payload is the GELU layout, byte for byte
    back = B.WeightImage.load(qg, p_q)
    assert back is not None and bytes(back.c.cfg) == bytes(img_q.c.cfg)
    assert np.array_equal(back.f32_section().view(np.uint32), img_q.f32_section().view(np.uint32))
    # a version-3 file loads only under its own kind; a version-2 file only as a GELU model
    assert B.WeightImage.load(gelu, p_q) is None and B.WeightImage.load(qg, p_g) is None
    assert B.WeightImage.load(SWIGLU_TWIN, p_q) is None
    sg = dataclasses.replace(qg, hidden_dim=qg.hidden_dim // 2, mlp="swiglu")       # 2H rows of fc1: the same file size as H of qg ...
    p_s = str(tmp_path / "sg.cache")
    assert B.WeightImage.build(sg, synth.make_weights(sg, 5, native=False)).save(p_s) == 0
    assert file_header(p_s)[0] == 3 and B.WeightImage.load(qg, p_s) is None and B.WeightImage.load(sg, p_q) is None
    raw = bytearray(open(p_q, "rb").read())                                        # ... and a forged kind word does not pass either
    raw[16 + 28:16 + 32] = struct.pack("<i", qg.hidden_dim | (1 << 24))
    forged = str(tmp_path / "forged.cache")
    open(forged, "wb").write(bytes(raw))
    assert B.WeightImage.load(qg, forged) is None


def test_create_accepts_quickgelu_by_its_checks_and_refuses_the_other_kinds_naming_the_three():
    L = B.lib()
    assert synth.MLP_KINDS == {"gelu": 0, "swiglu": 1} and synth.MLP_CODES == {"gelu": 0, "swiglu": 1, "quickgelu": 3}
    for kind in (2, 4, 9, 127):
        h = C.c_void_p()
        cc = B.CConfig.of(dataclasses.replace(TINY_CLIP, mlp=kind))
        rc = L.vit_engine_create(C.byref(h), C.byref(cc), None)
        msg = L.vit_engine_last_error(h).decode() if h else ""
        if h:
            L.vit_engine_destroy(h)
        assert rc == VIT_ERR_ARG and "MLP kind" in msg and str(kind) in msg, (rc, msg)
        assert all(n in msg for n in ("VIT_MLP_GELU", "VIT_MLP_SWIGLU", "VIT_MLP_QUICKGELU")), msg
    with pytest.raises(ValueError):
        synth.ModelConfig(mlp="tanhgelu")
    assert synth.ModelConfig(mlp="quickgelu").fc1_rows == 3072
