"""The SwiGLU MLP kind (VIT_MLP_SWIGLU in the top bits of vit_config.hidden_dim), what can be checked without a GPU: the packing, the tensor
sizes and MAC counts that follow from it, the two weight generators, the weight image and its cache file (version 2 stays the
GELU format, bit for bit; version 3 is the same header for a SwiGLU model), and vit_engine_create's answer to an unknown kind."""
import ctypes as C
import dataclasses
import os
import struct
import subprocess

import numpy as np
import pytest

from swiglu_model import SMALL_SG, TINY_SG
from vit_amd import binding as B
from vit_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIT_ERR_ARG = 1
GELU_TWIN = dataclasses.replace(TINY_SG, mlp="gelu")   # the same eight dimensions


def test_vit_config_keeps_its_eight_ints_and_hidden_dim_carries_the_kind(tmp_path):
    """The struct does not grow (compiled callers, positional initialisers and the pinned sizes of the other ABI tests stay): the
    kind sits in bits 24..30 of hidden_dim, and the header's macros and the binding pack it alike."""
    names = [n for n, *_ in B.CConfig._fields_]
    assert names == ["img_size", "patch_size", "in_chans", "num_classes", "embed_dim", "depth", "num_heads", "hidden_dim"]
    src, exe = tmp_path / "cfg.c", tmp_path / "cfg"
    src.write_text("\n".join([
        "#include <stdio.h>", "#include <stddef.h>", '#include "vit_types.h"', "int main(void) {",
        "    vit_config b16 = {224, 16, 3, 1000, 768, 12, 12, 3072};   /* the positional initialiser of the eight dimensions */",
        "    vit_config g14 = {224, 14, 3, 1000, 1536, 40, 24, VIT_HIDDEN_DIM_OF(4096, VIT_MLP_SWIGLU)};",
        '    printf("%zu %zu %d %d %d %d %d %d %d %d %d %d\\n", sizeof(vit_config), offsetof(vit_config, hidden_dim), VIT_MLP_GELU, VIT_MLP_SWIGLU,',
        "           VIT_MLP_SHIFT, VIT_MLP_KIND(&b16), VIT_HIDDEN_DIM(&b16), VIT_FC1_ROWS(&b16), g14.hidden_dim, VIT_MLP_KIND(&g14),",
        "           VIT_HIDDEN_DIM(&g14), VIT_FC1_ROWS(&g14));", "    return 0;", "}"]))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    size, off_hidden, gelu, swiglu, shift = out[:5]
    assert size == C.sizeof(B.CConfig) == 8 * C.sizeof(C.c_int) and off_hidden == B.CConfig.hidden_dim.offset == size - C.sizeof(C.c_int)
    assert (gelu, swiglu, shift) == (0, 1, 24) and synth.MLP_KINDS == {"gelu": gelu, "swiglu": swiglu} and synth.MLP_SHIFT == shift
    assert out[5:8] == [0, 3072, 3072]                                   # a plain width is a GELU model
    assert out[8:] == [4096 | (1 << 24), 1, 4096, 8192]
    assert B.CConfig.of(synth.VIT_G14).hidden_dim == out[8] and synth.VIT_G14.hidden_dim == 4096
    assert B.CConfig.of(TINY_SG).hidden_dim == TINY_SG.hidden_dim | (1 << 24) and B.CConfig.of(synth.VIT_TINY).hidden_dim == synth.VIT_TINY.hidden_dim
    assert synth.ModelConfig().mlp == "gelu" and B.lib().vit_config_b16().hidden_dim == 3072


def test_the_preset_is_dinov2_vit_g14():
    g = synth.VIT_G14
    assert (g.img_size, g.patch_size, g.embed_dim, g.depth, g.num_heads, g.hidden_dim, g.mlp) == (224, 14, 1536, 40, 24, 4096, "swiglu")
    shapes = g.weight_shapes()
    assert shapes[12] == (8192, 1536) and shapes[13] == (8192,) and shapes[14] == (1536, 4096) and shapes[15] == (1536,)
    assert g.tokens == 257 and g.n_weights == 4 + 12 * 40 + 4 and g.fc1_rows == 8192


@pytest.mark.parametrize("cfg", [TINY_SG, SMALL_SG, synth.VIT_G14], ids=["tiny_sg", "small_sg", "g14"])
def test_weight_sizes_and_macs_use_two_h_for_fc1(cfg):
    L = B.lib()
    cc = B.CConfig.of(cfg)
    D, H, T = cfg.embed_dim, cfg.hidden_dim, cfg.tokens
    for l in (0, cfg.depth - 1):
        got = [L.vit_config_weight_size(C.byref(cc), 4 + 12 * l + k) for k in (8, 9, 10, 11)]
        assert got == [2 * H * D, 2 * H, D * H, D]
    shapes = cfg.weight_shapes()
    assert [L.vit_config_weight_size(C.byref(cc), i) for i in range(cfg.n_weights)] == [int(np.prod(s)) for s in shapes]
    hd = D // cfg.num_heads
    per_layer = T * D * 3 * D + 2 * cfg.num_heads * T * T * hd + T * D * D + T * D * 2 * H + T * H * D
    want = (T - 1) * cfg.patch_dim * D + cfg.depth * per_layer + D * cfg.num_classes
    assert L.vit_config_macs_per_image(C.byref(cc)) == want == cfg.macs_per_image
    saved = (T - 1) * (D * D + 2 * cfg.num_heads * T * hd + D * D + D * 2 * H + H * D)
    assert L.vit_config_macs_per_image_pruned(C.byref(cc)) == want - saved


def test_gelu_configurations_keep_their_sizes_and_macs():
    L = B.lib()
    for cfg in (synth.VIT_B16, synth.VIT_TINY, GELU_TWIN):
        cc = B.CConfig.of(cfg)
        D, H, T = cfg.embed_dim, cfg.hidden_dim, cfg.tokens
        assert [L.vit_config_weight_size(C.byref(cc), 4 + k) for k in (8, 9, 10, 11)] == [H * D, H, D * H, D]
        assert cfg.weight_shapes()[12:16] == [(H, D), (H,), (D, H), (D,)]
        hd = D // cfg.num_heads
        per_layer = T * D * 3 * D + 2 * cfg.num_heads * T * T * hd + T * D * D + 2 * T * D * H
        assert L.vit_config_macs_per_image(C.byref(cc)) == cfg.macs_per_image == (T - 1) * cfg.patch_dim * D + cfg.depth * per_layer + D * cfg.num_classes
    assert synth.VIT_B16.macs_per_image == 17_563_828_224


@pytest.mark.parametrize("cfg", [TINY_SG, SMALL_SG], ids=["tiny_sg", "small_sg"])
def test_c_and_python_generators_give_the_same_bytes(cfg):
    c = B.synth_weights_c(cfg, 77)
    py = synth.make_weights(cfg, 77, native=False)
    assert len(c) == len(py) == cfg.n_weights
    for i, (a, b) in enumerate(zip(c, py)):
        assert a.size == b.size == int(np.prod(cfg.weight_shapes()[i])), i
        assert np.array_equal(np.asarray(a).reshape(-1).view(np.uint32), b.reshape(-1).view(np.uint32)), i


def file_version(path):
    with open(path, "rb") as f:
        magic, version = struct.unpack("<II", f.read(8))
    assert magic == 0x57544956
    return version


def test_weight_image_round_trip_and_the_version_carries_the_mlp_kind(tmp_path):
    sg, gelu = TINY_SG, GELU_TWIN
    Wsg, Wg = synth.make_weights(sg, 5, native=False), synth.make_weights(gelu, 5, native=False)
    img_sg, img_g = B.WeightImage.build(sg, Wsg), B.WeightImage.build(gelu, Wg)
    assert img_sg.c.cfg.hidden_dim >> 24 == 1 and img_g.c.cfg.hidden_dim == gelu.hidden_dim
    for a, b in zip(img_sg.tensors(), Wsg):
        assert np.array_equal(a, b.reshape(-1))
    p_sg, p_g = str(tmp_path / "sg.cache"), str(tmp_path / "gelu.cache")
    assert img_sg.save(p_sg) == 0 and img_g.save(p_g) == 0
    assert file_version(p_g) == 2 and file_version(p_sg) == 3
    back = B.WeightImage.load(sg, p_sg)
    assert back is not None and back.c.cfg.hidden_dim == sg.hidden_dim | (1 << 24)
    assert np.array_equal(back.f32_section().view(np.uint32), img_sg.f32_section().view(np.uint32))
    assert np.array_equal(back.bf16_section(), img_sg.bf16_section())
    assert bytes(back.c.cfg) == bytes(img_sg.c.cfg)
    back_g = B.WeightImage.load(gelu, p_g)
    assert back_g is not None and np.array_equal(back_g.f32_section().view(np.uint32), img_g.f32_section().view(np.uint32))
    # each file is refused under the other configuration of equal dimensions
    assert B.WeightImage.load(gelu, p_sg) is None and B.WeightImage.load(sg, p_g) is None
    # ... also when the version word is forged: the payload sizes disagree
    raw = bytearray(open(p_g, "rb").read())
    raw[4:8] = struct.pack("<I", 3)
    forged = str(tmp_path / "forged.cache")
    open(forged, "wb").write(bytes(raw))
    assert B.WeightImage.load(sg, forged) is None


def test_a_gelu_file_has_the_header_it_always_had(tmp_path):
    """The 80 header bytes of a GELU model's cache file, field by field: version 2, the eight dimensions, nothing about the MLP kind."""
    cfg = synth.VIT_TINY
    img = B.WeightImage.build(cfg, synth.make_weights(cfg, 9, native=False))
    path = str(tmp_path / "tiny.cache")
    assert img.save(path) == 0
    head = open(path, "rb").read(80)
    magic, version, count, n_sources = struct.unpack("<4I", head[:16])
    dims = struct.unpack("<8i", head[16:48])
    f32_floats, gemm_floats, bf16_elems, payload = struct.unpack("<4Q", head[48:80])
    assert (magic, version, count, n_sources) == (0x57544956, 2, cfg.n_weights, 0)
    assert dims == (cfg.img_size, cfg.patch_size, cfg.in_chans, cfg.num_classes, cfg.embed_dim, cfg.depth, cfg.num_heads, cfg.hidden_dim)
    assert (f32_floats, gemm_floats, bf16_elems, payload) == (img.c.f32_floats, img.c.gemm_floats, img.c.bf16_elems, 4096)
    assert os.path.getsize(path) == 4096 + 4 * f32_floats + 2 * bf16_elems


def test_a_gelu_sized_fc1_tensor_is_refused_by_the_image_builder():
    W = synth.make_weights(TINY_SG, 5, native=False)
    W[12] = np.ascontiguousarray(W[12][:TINY_SG.hidden_dim])   # H x D: what a GELU model of these dimensions holds
    with pytest.raises(B.VitError):
        B.WeightImage.build(TINY_SG, W)
    with pytest.raises(B.VitError):   # and the other way round
        B.WeightImage.build(GELU_TWIN, synth.make_weights(TINY_SG, 5, native=False))


def test_create_refuses_an_unknown_mlp_kind_and_names_where_it_sits():
    L = B.lib()
    for kind in (7, 127, 2):
        h = C.c_void_p()
        cc = B.CConfig.of(dataclasses.replace(TINY_SG, mlp=kind))
        assert cc.hidden_dim >> 24 == kind
        rc = L.vit_engine_create(C.byref(h), C.byref(cc), None)
        msg = L.vit_engine_last_error(h).decode() if h else ""
        if h:
            L.vit_engine_destroy(h)
        assert rc == VIT_ERR_ARG and "MLP kind" in msg and "hidden_dim" in msg and str(kind) in msg, (rc, msg)
    with pytest.raises(ValueError):
        synth.ModelConfig(mlp="geglu")


def test_library_exports_the_two_launchers_and_they_refuse_bad_arguments_before_any_hip_call():
    syms = subprocess.run(["nm", "-D", "--defined-only", B.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
    assert {"vithip_swiglu_f32", "vithip_swiglu_bf16"} <= names
    INVALID = 1   # hipErrorInvalidValue
    p = 0x10000   # never dereferenced: every call below is refused on its arguments
    for bf16, v in ((False, 4), (True, 8)):
        assert B.swiglu_raw(p, 4 * v, p + 4096, 2 * v, 0, 2 * v, bf16) == INVALID          # rows = 0
        assert B.swiglu_raw(p, 4 * v, p + 4096, 2 * v, 1, 2 * v - 2, bf16) == INVALID      # H % vec
        assert B.swiglu_raw(p, 4 * v - v, p + 4096, 2 * v, 1, 2 * v, bf16) == INVALID      # ldu < 2H
        assert B.swiglu_raw(p, 4 * v, p + 4096, v, 1, 2 * v, bf16) == INVALID              # ldh < H
        assert B.swiglu_raw(p, 4 * v + 2, p + 4096, 2 * v, 1, 2 * v, bf16) == INVALID      # ldu % vec
        assert B.swiglu_raw(p + 4, 4 * v, p + 4096, 2 * v, 1, 2 * v, bf16) == INVALID      # u misaligned
        assert B.swiglu_raw(p, 4 * v, p + 4096 + 8, 2 * v, 1, 2 * v, bf16) == INVALID      # h misaligned
        assert B.swiglu_raw(p, 4 * v, p + 16, 4 * v, 2, 2 * v, bf16) == INVALID            # partial overlap
        assert B.swiglu_raw(p, 4 * v, p, 8 * v, 2, 2 * v, bf16) == INVALID                 # same base, another leading dimension
        assert B.swiglu_raw(None, 4 * v, p, 2 * v, 1, 2 * v, bf16) == INVALID              # NULL
