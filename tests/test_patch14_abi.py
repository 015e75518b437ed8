"""Patch-14 support (vithip_patch_embed_f32_general, vit_weights_fold_layer_scale, the engine's geometry rule): what can be checked
without a GPU -- the exported symbols, the header prototypes against the binding's argument lists, and vit_engine_create's
answers to odd and to even patch geometries (the check runs before the engine looks for a device).
"""
import ctypes as C
import os
import re
import subprocess

import pytest

from patch14_model import ODD14, SMALL14, TINY14
from vit_amd import binding as B
from vit_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIT_ERR_ARG = 1


def prototype(header, name):
    """The parameter declarations of `name` in include/<header>."""
    text = open(os.path.join(ROOT, "include", header)).read()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in {header}"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def ctype_of(decl):
    if "*" in decl or "[" in decl or decl.startswith("vithip_stream_t"):
        return "pointer"
    assert decl.startswith("int "), decl
    return "int"


def test_library_exports_the_two_new_symbols():
    syms = subprocess.run(["nm", "-D", "--defined-only", B.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
    for want in ("vithip_patch_embed_f32_general", "vit_weights_fold_layer_scale", "vithip_patch_embed_f32"):
        assert want in names, want


def test_header_prototypes_match_the_binding():
    L = B.lib()
    general, old = prototype("vit_hip_kernels.h", "vithip_patch_embed_f32_general"), prototype("vit_hip_kernels.h", "vithip_patch_embed_f32")
    assert general == old  # the same signature, name for name
    assert [p.split()[-1].lstrip("*") for p in general] == ["stream", "images", "conv_w", "conv_b", "cls", "pos", "x", "n_images", "img_size",
                                                           "patch_size", "in_chans", "embed_dim"]
    assert [ctype_of(p) for p in general] == ["pointer"] * 7 + ["int"] * 5
    assert list(L.vithip_patch_embed_f32_general.argtypes) == list(L.vithip_patch_embed_f32.argtypes) == [C.c_void_p] * 7 + [C.c_int] * 5
    fold = prototype("vit_io.h", "vit_weights_fold_layer_scale")
    assert fold == ["const vit_config *cfg", "Network weights[]", "int count", "const Network scales[]", "int scale_count"]
    assert list(L.vit_weights_fold_layer_scale.argtypes) == [C.POINTER(B.CConfig), C.POINTER(B.CNetwork), C.c_int, C.POINTER(B.CNetwork),
                                                             C.c_int]
    assert C.sizeof(B.CNetwork) == C.sizeof(C.c_void_p) + C.sizeof(C.c_size_t)


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


@pytest.mark.parametrize("img,patch", [(28, 7), (21, 7), (15, 3), (35, 5)])
def test_create_refuses_odd_geometries_and_names_the_rule(img, patch):
    cfg = synth.ModelConfig(img_size=img, patch_size=patch, num_classes=10, embed_dim=128, depth=2, num_heads=2, hidden_dim=256)
    rc, msg = create(cfg)
    assert rc == VIT_ERR_ARG, (rc, msg)
    assert "geometry" in msg and "even" in msg and f"patch_size {patch}" in msg and f"img_size {img}" in msg, msg


def test_create_still_refuses_an_image_that_is_no_multiple_of_the_patch():
    rc, msg = create(synth.ModelConfig(img_size=30, patch_size=14, num_classes=10, embed_dim=128, depth=2, num_heads=2, hidden_dim=256))
    assert rc == VIT_ERR_ARG and "multiple of patch_size" in msg, (rc, msg)


@pytest.mark.parametrize("cfg", [TINY14, SMALL14, ODD14, synth.ModelConfig(patch_size=14), synth.ModelConfig(img_size=518, patch_size=14),
                                 synth.VIT_TINY], ids=["tiny14", "small14", "odd14", "b14-224", "b14-518", "tiny16"])
def test_create_gets_past_the_geometry_check_at_even_patches(cfg):
    """Without a device the call then fails on the device, with a device it succeeds: never VIT_ERR_ARG about the geometry."""
    rc, msg = create(cfg)
    assert "geometry" not in msg and "patch" not in msg, (rc, msg)
    if rc != 0:
        assert rc != VIT_ERR_ARG or "device" in msg, (rc, msg)
