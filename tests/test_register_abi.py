"""Register tokens (VIT_REGISTER_TOKENS in vit_config.patch_size): what can be checked without a GPU -- the macros, the model constants
at R = 0, 1, 4, vit_engine_create's answer to R = 17 (the check runs before the engine looks for a device), the C generator's bytes,
and the cache file: byte for byte the old one without registers, version 3 and bound to its own R with them.
"""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from register_model import REG_ODD, REG_TINY
from vit_amd import binding as B
from vit_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIT_ERR_ARG = 1


def with_registers(cfg, R):
    return synth.ModelConfig(**{**cfg.__dict__, "num_register_tokens": R})


def macro(name):
    text = open(os.path.join(ROOT, "include", "vit_types.h")).read()
    m = re.search(r"#define\s+" + name + r"\b(?:\([^)]*\))?\s+(.*)", text)
    assert m, name
    return m.group(1).strip()


def test_the_macros_round_trip_and_the_binding_packs_what_they_read():
    assert macro("VIT_REG_SHIFT") == "24" and synth.REG_SHIFT == 24
    assert macro("VIT_MAX_REGISTER_TOKENS") == "16" and synth.MAX_REGISTER_TOKENS == 16
    assert macro("VIT_PATCH_SIZE_OF") == "((int)(patch) | ((int)(regs) << VIT_REG_SHIFT))"
    assert macro("VIT_PATCH_SIZE") == "((cfg)->patch_size & ((1 << VIT_REG_SHIFT) - 1))"
    assert macro("VIT_REGISTER_TOKENS") == "((cfg)->patch_size >> VIT_REG_SHIFT)"
    for patch in (8, 14, 16, 32):
        for R in (0, 1, 4, 16):
            cc = B.CConfig.of(synth.ModelConfig(patch_size=patch, num_register_tokens=R))
            assert cc.patch_size == patch | (R << 24)
            assert cc.patch_size & ((1 << 24) - 1) == patch and cc.patch_size >> 24 == R
    assert B.CConfig.of(synth.VIT_B16).patch_size == 16  # a plain patch size is a model without registers
    assert C.sizeof(B.CConfig) == 8 * C.sizeof(C.c_int)  # the struct keeps its eight ints


def test_the_header_of_the_new_entries_matches_the_binding_and_the_library_exports_them():
    syms = subprocess.run(["nm", "-D", "--defined-only", B.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
    for want in ("vithip_patch_embed_f32_reg", "vithip_patch_embed_f32_general_reg", "vithip_patch_embed_bf16_reg",
                 "vithip_tap_f32_prefix_eps", "vit_config_patches"):
        assert want in names, want
    text = open(os.path.join(ROOT, "include", "vit_hip_kernels.h")).read()
    for name, tail in (("vithip_patch_embed_f32_reg", ["int embed_dim", "int num_registers"]),
                       ("vithip_patch_embed_f32_general_reg", ["int embed_dim", "int num_registers"]),
                       ("vithip_patch_embed_bf16_reg", ["int embed_dim", "int num_registers"]),
                       ("vithip_tap_f32_prefix_eps", ["int tokens", "int prefix", "int dim", "int layout", "double eps"])):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        assert params[-len(tail):] == tail, (name, params)
        assert "const float *prefix" in params or name.startswith("vithip_tap"), params


@pytest.mark.parametrize("R", [0, 1, 4])
def test_model_constants_with_registers(R):
    L = B.lib()
    L.vit_config_patches.argtypes = [C.POINTER(B.CConfig)]
    L.vit_config_tokens.argtypes = [C.POINTER(B.CConfig)]
    for base in (synth.VIT_B16, synth.ModelConfig(patch_size=14), REG_TINY, REG_ODD, synth.VIT_G14):
        cfg = with_registers(base, R)
        cc = B.CConfig.of(cfg)
        g = cfg.img_size // cfg.patch_size
        assert L.vit_config_patches(C.byref(cc)) == g * g == cfg.patches
        assert L.vit_config_tokens(C.byref(cc)) == g * g + 1 + R == cfg.tokens
        sizes = [L.vit_config_weight_size(C.byref(cc), i) for i in range(cfg.n_weights)]
        assert sizes == [int(np.prod(s)) for s in cfg.weight_shapes()]
        D = cfg.embed_dim
        assert sizes[0] == (1 + R) * D and sizes[3] == (g * g + 1) * D  # the prefix; registers have no position embedding
        assert L.vit_config_weight_size(C.byref(cc), cfg.n_weights) == 0
        # exact MACs: the conv over P patches, the layers over T = 1 + R + P rows
        T, P, H, H1, hd = g * g + 1 + R, g * g, cfg.hidden_dim, cfg.fc1_rows, D // cfg.num_heads
        layer = T * D * 3 * D + 2 * cfg.num_heads * T * T * hd + T * D * D + T * D * H1 + T * H * D
        want = P * cfg.patch_dim * D + cfg.depth * layer + D * cfg.num_classes
        assert L.vit_config_macs_per_image(C.byref(cc)) == want == cfg.macs_per_image
        saved = (T - 1) * (D * D + 2 * cfg.num_heads * T * hd + D * D + D * H1 + H * D)  # the pruned last layer keeps one row of T
        assert L.vit_config_macs_per_image_pruned(C.byref(cc)) == want - saved
    if R == 0:
        assert synth.VIT_B16.macs_per_image == 17_563_828_224 and synth.VIT_B16.weight_shapes()[0] == (768,)
    assert synth.DINOV2_B14_REG4.tokens == 261 and synth.DINOV2_B14_REG4.patches == 256
    assert synth.DINOV2_B14_REG4.weight_shapes()[0] == (5, 768) and synth.DINOV2_B14_REG4.weight_shapes()[3] == (257, 768)


def create(cfg):
    """(code, message) of vit_engine_create; the engine, if one came back, is destroyed."""
    L = B.lib()
    h = C.c_void_p()
    cc = B.CConfig.of(cfg)
    rc = L.vit_engine_create(C.byref(h), C.byref(cc), None)
    msg = L.vit_engine_last_error(h).decode() if h else ""
    if h:
        L.vit_engine_destroy(h)
    return rc, msg


@pytest.mark.parametrize("R", [17, 100, 127])
def test_create_refuses_too_many_registers_by_name(R):
    rc, msg = create(with_registers(REG_TINY, R))
    assert rc == VIT_ERR_ARG, (rc, msg)
    assert "patch_size" in msg and "bits 24..30" in msg and f"{R} register tokens" in msg and "VIT_REGISTER_TOKENS" in msg, msg


@pytest.mark.parametrize("R", [0, 1, 4, 16])
def test_create_gets_past_the_config_check_with_registers(R):
    """Without a device the call then fails on the device, with a device it succeeds: never VIT_ERR_ARG about the configuration."""
    rc, msg = create(with_registers(REG_TINY, R))
    assert "register" not in msg and "patch" not in msg and "geometry" not in msg, (rc, msg)
    if rc != 0:
        assert rc != VIT_ERR_ARG or "device" in msg, (rc, msg)


def test_the_c_generator_gives_the_python_bytes_for_a_register_model():
    cfg = REG_TINY
    want = synth.make_weights(cfg, 21, native=False)
    assert want[0].shape == (5, cfg.embed_dim) and want[3].shape == (cfg.patches + 1, cfg.embed_dim)
    for a, b in zip(B.synth_weights_c(cfg, 21), want):
        assert a.shape == b.shape and np.array_equal(a, b)
    L = B.lib()
    nets = (B.CNetwork * cfg.n_weights)()
    assert L.vit_synth_weights(C.byref(B.CConfig.of(cfg)), 21, nets, cfg.n_weights) == 0
    for i, b in enumerate(want):
        assert nets[i].size == b.size and np.array_equal(np.ctypeslib.as_array(nets[i].data, shape=(b.size,)), b.ravel())
    L.free_weights(nets, cfg.n_weights)
    # the class row and every other tensor are those of the model without registers: the streams are per tensor, the prefix only grows
    plain = synth.make_weights(with_registers(cfg, 0), 21, native=False)
    assert np.array_equal(want[0][0], plain[0]) and all(np.array_equal(a, b) for a, b in zip(want[1:], plain[1:]))


def old_cache_file(cfg, W):
    """The bytes a cache file has had since version 2 / 3, restated: header, zero fill up to 4096, the fp32 section with every tensor
    in a slot of 128 floats (GEMM operands first), their bf16 copies."""
    n = cfg.n_weights
    gemm = [i for i in range(n) if i == 1 or (4 <= i < 4 + 12 * cfg.depth and (i - 4) % 12 in (2, 4, 8, 10))]
    order = gemm + [i for i in range(n) if i not in gemm]
    f32, gemm_floats = [], 0
    for i in order:
        w = np.asarray(W[i], np.float32).ravel()
        f32 += [w, np.zeros(-w.size % 128, np.float32)]
        if i == gemm[-1]:
            gemm_floats = sum(a.size for a in f32)
    f32 = np.concatenate(f32)
    kind = synth.MLP_CODES[cfg.mlp]
    words = (cfg.img_size, cfg.patch_size, cfg.in_chans, cfg.num_classes, cfg.embed_dim, cfg.depth, cfg.num_heads,
             cfg.hidden_dim | (kind << 24))
    head = struct.pack("<4I8i4Q", 0x57544956, 3 if kind else 2, n, 0, *words, f32.size, gemm_floats, gemm_floats, 4096)
    return head + bytes(4096 - len(head)) + f32.tobytes() + B.to_bf16_bits(f32[:gemm_floats]).tobytes()


@pytest.mark.parametrize("mlp", ["gelu", "swiglu", "quickgelu"])
def test_a_cache_file_without_registers_is_byte_for_byte_the_old_one(tmp_path, mlp):
    cfg = synth.ModelConfig(img_size=28, patch_size=14, num_classes=10, embed_dim=128, depth=2, num_heads=2, hidden_dim=256, mlp=mlp)
    W = synth.make_weights(cfg, 3, native=False)
    path = str(tmp_path / "w.cache")
    assert B.WeightImage.build(cfg, W, with_bf16=True).save(path) == 0
    got = open(path, "rb").read()
    want = old_cache_file(cfg, W)
    assert struct.unpack_from("<I", got, 4)[0] == (2 if mlp == "gelu" else 3)
    assert len(got) == len(want) and got == want


def test_a_register_model_writes_version_3_and_loads_under_its_own_count_only(tmp_path):
    cfg = REG_TINY
    W = synth.make_weights(cfg, 3, native=False)
    img = B.WeightImage.build(cfg, W, with_bf16=True)
    for t, w in zip(img.tensors(), W):
        assert np.array_equal(t, w.ravel())
    path = str(tmp_path / "w.cache")
    assert img.save(path) == 0
    raw = open(path, "rb").read()
    magic, version = struct.unpack_from("<II", raw, 0)
    assert magic == 0x57544956 and version == 3
    assert struct.unpack_from("<8i", raw, 16)[1] == 14 | (4 << 24)  # what a reader of plain patch sizes sees: no patch size at all
    back = B.WeightImage.load(cfg, path)
    assert back is not None and np.array_equal(back.f32_section(), img.f32_section())
    assert np.array_equal(back.bf16_section(), img.bf16_section())
    for R in (0, 1, 5):
        assert B.WeightImage.load(with_registers(cfg, R), path) is None, R
    # ... and a file of the model without registers is refused under a count
    plain = with_registers(cfg, 0)
    ppath = str(tmp_path / "p.cache")
    assert B.WeightImage.build(plain, synth.make_weights(plain, 3, native=False)).save(ppath) == 0
    assert B.WeightImage.load(plain, ppath) is not None and B.WeightImage.load(cfg, ppath) is None
    # a prefix of another size is no weight set of this model
    with pytest.raises(B.VitError):
        B.WeightImage.build(cfg, [W[0][:1]] + W[1:])
    with pytest.raises(B.VitError):
        B.WeightImage.build(with_registers(cfg, 17), W)
