"""Classifier heads (vit_engine_set_head, vithip_pool_layernorm_f32): what can be checked of the interface without a GPU -- the
exported symbols, the enum values and the layout of vit_head_spec against a C compile, that the other structs kept their sizes, the
argument lists of the binding, the width query and the calls on a NULL engine, and the launcher's refusals, which come before any HIP
call.
"""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np

from vit_amd import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["vit_engine_head_in_features", "vit_engine_set_head", "vit_engine_read_head_operand",
                "vithip_pool_layernorm_f32", "vithip_pool_layernorm_f32_workspace_floats"]
HIP_INVALID_VALUE = 1


def test_libraries_export_the_engine_symbols_and_the_launcher():
    here = os.path.dirname(B.LIB_PATH)
    for path in {B.LIB_PATH, os.path.join(here, "libvit_mi355x.so"), os.path.join(here, "libvit_mi355x_probe.so")}:
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        names = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
        for want in ENTRY_POINTS + ["vithip_layernorm_pool_f32", "vit_engine_read_logits", "vit_engine_forward_device"]:
            assert want in names, (path, want)


def test_enum_values_spec_layout_and_unchanged_struct_sizes(tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "vit_engine.h"', '#include "vit_hip_kernels.h"', "int main(void) {",
             '    printf("pools %d %d %d\\n", VIT_HEAD_POOL_NONE, VIT_HEAD_POOL_AVG, VIT_HEAD_POOL_AVG_FCNORM);',
             '    printf("taps %d\\n", VIT_MAX_TAPS);',
             '    printf("spec %zu %zu %zu %zu %zu\\n", sizeof(vit_head_spec), offsetof(vit_head_spec, num_cls_layers), '
             "offsetof(vit_head_spec, cls_layers), offsetof(vit_head_spec, pool), offsetof(vit_head_spec, reserved));",
             '    printf("options %zu\\n", sizeof(vit_engine_options));', '    printf("config %zu\\n", sizeof(vit_config));',
             '    printf("intermediate %zu\\n", sizeof(vit_intermediate_spec));', '    printf("topk %zu\\n", sizeof(vit_topk_spec));',
             '    printf("feature %zu\\n", sizeof(vit_feature_spec));', "    return 0;", "}"]
    src, exe = tmp_path / "head.c", tmp_path / "head"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True,
                   text=True)
    out = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in
           subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()}
    assert out["pools"] == [0, 1, 2] and B.HEAD_POOLS == {"none": 0, "avg": 1, "avg_fcnorm": 2}
    assert out["taps"] == [32] == [B.VIT_MAX_TAPS]
    S = B.CHeadSpec
    assert out["spec"] == [C.sizeof(S), S.num_cls_layers.offset, S.cls_layers.offset, S.pool.offset, S.reserved.offset] == [140, 0, 4, 132, 136]
    # the head is engine state set by a call of its own: no other struct gained a field
    assert out["options"] == [C.sizeof(B.COptions)] == [12 * C.sizeof(C.c_int)]
    assert out["config"] == [C.sizeof(B.CConfig)] == [8 * C.sizeof(C.c_int)]
    assert out["intermediate"] == [C.sizeof(B.CIntermediateSpec)] == [(4 + 32) * 4]
    assert out["topk"] == [C.sizeof(B.CTopkSpec)] == [12]
    assert out["feature"] == [C.sizeof(B.CFeatureSpec)] == [8]


def test_binding_declares_the_calls():
    L = B.lib()
    spec = C.POINTER(B.CHeadSpec)
    v, i, z = C.c_void_p, C.c_int, C.c_size_t
    assert list(L.vit_engine_head_in_features.argtypes) == [v, spec] and L.vit_engine_head_in_features.restype == z
    assert list(L.vit_engine_set_head.argtypes) == [v, spec, B.f32p, B.f32p]
    assert list(L.vit_engine_read_head_operand.argtypes) == [v, B.f32p, i]
    assert list(L.vithip_pool_layernorm_f32.argtypes) == [v, v, z, v, z, v, v, i, i, i, i, v]
    assert list(L.vithip_pool_layernorm_f32_workspace_floats.argtypes) == [i] * 4
    assert L.vithip_pool_layernorm_f32_workspace_floats.restype == z
    op = inspect.signature(B.pool_layernorm).parameters
    assert list(op)[:6] == ["x", "gamma", "beta", "images", "tokens", "first_tok"]
    sh = inspect.signature(B.Engine.set_head).parameters
    assert list(sh)[:5] == ["self", "weight", "bias", "cls_layers", "pool"] and sh["cls_layers"].default == () and sh["pool"].default == "none"
    for name in ("set_head", "reset_head", "head_operand", "head_in_features"):
        assert callable(getattr(B.Engine, name)), name


def test_head_spec_helper_fills_the_struct():
    s = B.head_spec((8, 9, 10, 11), "avg")
    assert (s.num_cls_layers, list(s.cls_layers[:5]), s.pool, s.reserved) == (4, [8, 9, 10, 11, 0], 1, 0)
    s = B.head_spec((-4, -3, -2, -1), "avg", depth=12)
    assert list(s.cls_layers[:4]) == [8, 9, 10, 11]
    s = B.head_spec((), "avg_fcnorm", reserved=3)
    assert (s.num_cls_layers, s.pool, s.reserved) == (0, 2, 3)
    s = B.head_spec(range(40), 7)  # passed through for the C side to judge
    assert (s.num_cls_layers, s.pool) == (40, 7)


def test_workspace_floats_is_a_row_per_sixteen_tokens():
    f = B.lib().vithip_pool_layernorm_f32_workspace_floats
    g = B.lib().vithip_layernorm_pool_f32_workspace_floats
    for images, tokens, first, dim in [(1, 2, 1, 64), (3, 17, 1, 192), (3, 18, 1, 192), (2, 17, 0, 768), (256, 197, 1, 768), (4, 257, 1, 1024)]:
        want = images * -(-(tokens - first) // 16) * dim
        assert f(images, tokens, first, dim) == want == g(images, tokens, first, dim)
    for bad in [(0, 5, 1, 64), (1, 1, 1, 64), (1, 5, -1, 64), (1, 5, 1, 0)]:
        assert f(*bad) == 0


def test_calls_on_a_null_engine():
    L = B.lib()
    spec = B.head_spec((0,), "avg")
    w = np.zeros(4, np.float32)
    assert L.vit_engine_head_in_features(None, C.byref(spec)) == 0
    assert L.vit_engine_head_in_features(None, None) == 0
    assert L.vit_engine_set_head(None, C.byref(spec), w.ctypes.data_as(B.f32p), w.ctypes.data_as(B.f32p)) == 1  # VIT_ERR_ARG
    assert L.vit_engine_set_head(None, None, None, None) == 1
    assert L.vit_engine_read_head_operand(None, w.ctypes.data_as(B.f32p), 1) == 1


def test_the_launcher_refuses_bad_arguments_before_any_hip_call():
    """No device is needed (or touched): every refusal comes before the launch.  The pointers are host addresses that a launch would
    fault on -- they are only compared with NULL and checked for alignment."""
    f = B.lib().vithip_pool_layernorm_f32
    images, tokens, dim = 2, 5, 128

    def aligned(n):
        raw = np.zeros(n + 8, np.float32)
        off = (-raw.ctypes.data % 32) // 4
        return raw[off:off + n]

    x, out, g, b, ws = aligned(images * tokens * dim), aligned(images * dim), aligned(dim), aligned(dim), aligned(images * dim)
    good = dict(x=x.ctypes.data, ldx=dim, out=out.ctypes.data, ldo=dim, g=g.ctypes.data, b=b.ctypes.data, images=images, tokens=tokens,
                first=1, dim=dim, ws=ws.ctypes.data)

    def call(**kw):
        a = dict(good, **kw)
        return f(None, a["x"], a["ldx"], a["out"], a["ldo"], a["g"], a["b"], a["images"], a["tokens"], a["first"], a["dim"], a["ws"])

    for bad in [dict(x=None), dict(out=None), dict(g=None), dict(b=None), dict(ws=None), dict(images=0), dict(images=-2), dict(tokens=1),
                dict(first=-1), dict(first=tokens), dict(dim=0), dict(dim=126), dict(dim=2052), dict(ldx=dim - 4), dict(ldx=dim + 2),
                dict(ldo=dim - 4), dict(ldo=dim + 2), dict(x=good["x"] + 4), dict(out=good["out"] + 8), dict(g=good["g"] + 4),
                dict(b=good["b"] + 4), dict(ws=good["ws"] + 4)]:
        assert call(**bad) == HIP_INVALID_VALUE, bad
    assert not out.any() and not ws.any()
