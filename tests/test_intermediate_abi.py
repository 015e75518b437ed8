"""Intermediate-layer outputs (vit_engine_intermediate_*, vithip_tap_f32): what can be checked without a GPU.

The exported symbols, the layout of vit_intermediate_spec against its ctypes mirror, vit_engine_options unchanged, the binding's
argument lists, and the numpy restatement of the four layouts (tests/tap_model.py) that the GPU tests compare the kernel and the
engine with -- pinned here to the oracle's LayerNorm and to itself across layouts.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import tap_model
from conftest import oracle_config
from vit_amd import binding as B
from vit_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["vit_engine_intermediate_" + place + inp for place in ("device", "host") for inp in ("", "_u8", "_images")]


def test_library_exports_the_six_calls_the_row_width_and_the_tap_launcher():
    syms = subprocess.run(["nm", "-D", "--defined-only", B.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
    for want in CALLS + ["vit_engine_intermediate_row_elems", "vithip_tap_f32"]:
        assert want in names, want


def test_binding_declares_the_six_calls_like_the_features_calls_with_the_spec_exchanged():
    L = B.lib()
    for name in CALLS:
        got = list(getattr(L, name).argtypes)
        like = list(getattr(L, name.replace("intermediate", "features")).argtypes)
        assert got == [C.POINTER(B.CIntermediateSpec) if t is C.POINTER(B.CFeatureSpec) else t for t in like], name
        assert C.POINTER(B.CIntermediateSpec) in got
    assert L.vit_engine_intermediate_row_elems.restype is C.c_size_t
    assert list(L.vit_engine_intermediate_row_elems.argtypes) == [C.c_void_p, C.POINTER(B.CIntermediateSpec)]
    assert list(L.vithip_tap_f32.argtypes) == [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p] + [C.c_int] * 4


def test_intermediate_spec_mirror_has_the_layout_of_the_header_and_the_options_are_unchanged(tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "vit_engine.h"', '#include "vit_hip_kernels.h"', "int main(void) {",
             '    printf("size %zu\\n", sizeof(vit_intermediate_spec));', '    printf("options %zu\\n", sizeof(vit_engine_options));',
             '    printf("max_taps %d\\n", VIT_MAX_TAPS);',
             '    printf("kinds %d %d %d %d\\n", VIT_TAP_CLS, VIT_TAP_TOKENS, VIT_TAP_PATCHES, VIT_TAP_MAP);',
             '    printf("layouts %d %d %d %d\\n", VITHIP_TAP_CLS, VITHIP_TAP_TOKENS, VITHIP_TAP_PATCHES, VITHIP_TAP_MAP);']
    for name, *_ in B.CIntermediateSpec._fields_:
        lines.append(f'    printf("{name} %zu\\n", offsetof(vit_intermediate_spec, {name}));')
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "spec.c", tmp_path / "spec"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    out = {ln.split()[0]: ln.split()[1:] for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()}
    assert int(out["size"][0]) == C.sizeof(B.CIntermediateSpec) == (4 + 32) * C.sizeof(C.c_int)
    assert int(out["max_taps"][0]) == B.VIT_MAX_TAPS == 32
    for name, *_ in B.CIntermediateSpec._fields_:
        assert int(out[name][0]) == getattr(B.CIntermediateSpec, name).offset, name
    assert [int(v) for v in out["kinds"]] == [int(v) for v in out["layouts"]] == [B.TAP_KINDS[k] for k in tap_model.LAYOUTS]
    # the choice of output is per call: vit_engine_options gained no field (12 ints before and after)
    assert int(out["options"][0]) == C.sizeof(B.COptions) == 12 * C.sizeof(C.c_int)


def test_spec_builder_resolves_negative_layers_against_the_depth_and_passes_the_rest_through():
    s = B.intermediate_spec((2, 5, -4, -1), "map", True, depth=12)
    assert (s.kind, s.norm, s.num_layers, s.reserved) == (3, 1, 4, 0)
    assert list(s.layers)[:5] == [2, 5, 8, 11, 0] and not any(list(s.layers)[4:])
    s = B.intermediate_spec([3], 7, False)
    assert (s.kind, s.norm, s.num_layers, s.layers[0]) == (7, 0, 1, 3)
    assert B.intermediate_spec((-1,), "cls").layers[0] == -1          # no depth: left for the C side to refuse
    assert B.intermediate_spec(range(40), "cls").num_layers == 40      # more than the struct holds: refused there too
    assert B.tap_block(3, 17, 192, "map") == (192, 16) and B.tap_block(3, 17, 192, "cls") == (192,)
    assert B.tap_block(3, 17, 192, "tokens") == (17, 192) and B.tap_block(3, 17, 192, "patches") == (16, 192)


@pytest.mark.parametrize("norm", [0, 1])
def test_layouts_of_the_restatement_agree_with_each_other_and_with_the_oracle(oracle, norm):
    cfg = synth.VIT_TINY
    W = synth.make_weights(cfg, 21)
    ocfg = oracle_config(cfg)
    imgs = synth.make_images(cfg, 3, 105)
    stages = [oracle.forward_image(ocfg, im, W, want_stages=True)[2] for im in imgs]
    assert len(stages[0]) == cfg.depth + 1  # the embedding, then the stream behind every layer
    layers = list(range(cfg.depth))
    g = cfg.img_size // cfg.patch_size
    got = {k: tap_model.intermediate_reference(oracle, stages, layers, W[-4], W[-3], k, norm, grid=g) for k in tap_model.LAYOUTS}
    n, K, T, D = len(imgs), cfg.depth, cfg.tokens, cfg.embed_dim
    assert got["cls"].shape == (n, K, D) and got["tokens"].shape == (n, K, T, D)
    assert got["patches"].shape == (n, K, T - 1, D) and got["map"].shape == (n, K, D, g, g)
    assert np.array_equal(got["cls"], got["tokens"][:, :, 0])
    assert np.array_equal(got["patches"], got["tokens"][:, :, 1:])
    assert np.array_equal(got["map"].reshape(n, K, D, T - 1), got["patches"].transpose(0, 1, 3, 2))
    for i in range(n):
        for j, l in enumerate(layers):
            want = oracle.layer_norm(stages[i][l + 1], W[-4], W[-3]) if norm else stages[i][l + 1]
            assert np.array_equal(got["tokens"][i, j], want)
            # raster order: patch (r, c) of the grid is token 1 + r * g + c
            assert np.array_equal(got["map"][i, j][:, 1, 0], want[1 + g])
    # the last layer, normalised, is what the features reference of tests/test_gpu_features.py reads
    if norm:
        y = oracle.layer_norm(stages[0][cfg.depth], W[-4], W[-3])
        assert np.array_equal(got["tokens"][0, -1], y)


def test_arrange_moves_no_bit_and_block_sizes_add_up():
    rng = np.random.default_rng(3)
    for images, tokens, dim in ((1, 2, 4), (3, 10, 8), (2, 17, 12)):
        x = rng.standard_normal((images * tokens, dim)).astype(np.float32)
        for k in tap_model.LAYOUTS:
            a = tap_model.arrange(x, images, tokens, k)
            assert a.dtype == np.float32 and a[0].size == tap_model.block_elems(tokens, dim, k) == int(np.prod(B.tap_block(images, tokens, dim, k)))
        m, p = tap_model.arrange(x, images, tokens, "map"), tap_model.arrange(x, images, tokens, "patches")
        for i in range(images):
            assert np.array_equal(m[i].T, p[i])
            assert np.array_equal(p[i], x[i * tokens + 1:(i + 1) * tokens])
            assert np.array_equal(tap_model.arrange(x, images, tokens, "cls")[i], x[i * tokens])
