"""Dense linear heads (vit_engine_set_dense_head, vit_engine_dense_*, vithip_dense_upsample_argmax_f32): what needs no GPU.

The exported symbols, the two specs against their ctypes mirrors, vit_engine_options and vit_config unchanged, the binding's argument
lists, and the refusals that come before any HIP call: the launchers' and the fold helper's.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from vit_amd import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["vit_engine_dense_" + place + inp for place in ("device", "host") for inp in ("", "_u8", "_images")]
INVALID = 1  # hipErrorInvalidValue


def test_library_exports_the_head_the_six_calls_the_row_size_the_launchers_and_the_fold():
    syms = subprocess.run(["nm", "-D", "--defined-only", B.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
    for want in CALLS + ["vit_engine_set_dense_head", "vit_engine_dense_row_bytes", "vithip_dense_upsample_argmax_f32",
                         "vithip_dense_grid_f32", "vit_dense_head_fold_batchnorm"]:
        assert want in names, want


def test_binding_declares_the_six_calls_like_the_intermediate_calls_with_the_spec_and_the_rows_exchanged():
    L = B.lib()
    for name in CALLS:
        got = list(getattr(L, name).argtypes)
        like = list(getattr(L, name.replace("dense", "intermediate")).argtypes)
        want = [C.POINTER(B.CDenseSpec) if t is C.POINTER(B.CIntermediateSpec) else t for t in like]
        if "_host" in name:  # rows of bytes: void *const * in place of float *const *
            assert want[-1] is C.POINTER(B.f32p)
            want[-1] = C.POINTER(C.c_void_p)
        assert got == want, name
    assert L.vit_engine_dense_row_bytes.restype is C.c_size_t
    assert list(L.vit_engine_dense_row_bytes.argtypes) == [C.c_void_p, C.POINTER(B.CDenseSpec)]
    assert list(L.vit_engine_set_dense_head.argtypes) == [C.c_void_p, C.POINTER(B.CDenseHeadSpec), B.f32p, B.f32p]
    assert list(L.vithip_dense_upsample_argmax_f32.argtypes) == [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t] + [C.c_int] * 5


def test_spec_mirrors_have_the_layout_of_the_header_and_options_and_config_are_unchanged(tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "vit_engine.h"', "int main(void) {",
             '    printf("head_size %zu\\n", sizeof(vit_dense_head_spec));', '    printf("spec_size %zu\\n", sizeof(vit_dense_spec));',
             '    printf("options %zu\\n", sizeof(vit_engine_options));', '    printf("config %zu\\n", sizeof(vit_config));',
             '    printf("stages %d\\n", VIT_STAGE_COUNT);', '    printf("max_taps %d\\n", VIT_MAX_TAPS);',
             '    printf("kinds %d %d\\n", VIT_DENSE_LABELS, VIT_DENSE_GRID);']
    for name, *_ in B.CDenseHeadSpec._fields_:
        lines.append(f'    printf("head.{name} %zu\\n", offsetof(vit_dense_head_spec, {name}));')
    for name, *_ in B.CDenseSpec._fields_:
        lines.append(f'    printf("spec.{name} %zu\\n", offsetof(vit_dense_spec, {name}));')
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "spec.c", tmp_path / "spec"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = {ln.split()[0]: ln.split()[1:] for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()}
    assert int(out["head_size"][0]) == C.sizeof(B.CDenseHeadSpec) == (4 + 32) * C.sizeof(C.c_int)
    assert int(out["spec_size"][0]) == C.sizeof(B.CDenseSpec) == 4 * C.sizeof(C.c_int)
    for name, *_ in B.CDenseHeadSpec._fields_:
        assert int(out["head." + name][0]) == getattr(B.CDenseHeadSpec, name).offset, name
    for name, *_ in B.CDenseSpec._fields_:
        assert int(out["spec." + name][0]) == getattr(B.CDenseSpec, name).offset, name
    assert [f[0] for f in B.CDenseHeadSpec._fields_] == ["num_layers", "layers", "norm", "num_classes", "reserved"]
    assert [f[0] for f in B.CDenseSpec._fields_] == ["kind", "out_h", "out_w", "reserved"]
    assert [int(v) for v in out["kinds"]] == [B.DENSE_KINDS["labels"], B.DENSE_KINDS["grid"]] == [0, 1]
    assert int(out["max_taps"][0]) == B.VIT_MAX_TAPS
    # the head is engine state and the output a per-call spec: no option, no configuration field and no stage was added
    assert int(out["options"][0]) == C.sizeof(B.COptions) == 12 * C.sizeof(C.c_int)
    assert int(out["config"][0]) == C.sizeof(B.CConfig) == 8 * C.sizeof(C.c_int)
    assert int(out["stages"][0]) == len(B.STAGES) == 9


def test_spec_builders_resolve_negative_layers_and_sizes_and_pass_the_rest_through():
    s = B.dense_head_spec((-4, -3, -2, -1), True, 150, depth=12)
    assert (s.num_layers, s.norm, s.num_classes, s.reserved) == (4, 1, 150, 0)
    assert list(s.layers)[:5] == [8, 9, 10, 11, 0] and not any(list(s.layers)[4:])
    assert B.dense_head_spec([3], False, 21).layers[0] == 3 and B.dense_head_spec((-1,), True, 21).layers[0] == -1
    assert B.dense_head_spec(range(40), True, 2).num_layers == 40      # more than the struct holds: refused on the C side
    d = B.dense_spec("labels")
    assert (d.kind, d.out_h, d.out_w, d.reserved) == (0, 0, 0, 0)
    d = B.dense_spec("labels", 64)
    assert (d.out_h, d.out_w) == (64, 64)
    d = B.dense_spec("grid", (37, 53), reserved=1)
    assert (d.kind, d.out_h, d.out_w, d.reserved) == (1, 37, 53, 1)
    assert B.dense_spec(7).kind == 7


def test_launchers_refuse_bad_arguments_before_any_hip_call():
    """No device is needed: every check comes before the first HIP call, and a refused call never reads its pointers."""
    ok = dict(logits_ptr=0x1000, ld_logits=21, image_stride=16 * 21, out_ptr=0x2000, out_image_stride=64 * 64, images=2, g=4, classes=21,
              out_h=64, out_w=64)
    bad = [dict(logits_ptr=None), dict(out_ptr=None), dict(images=0), dict(images=-1), dict(g=0), dict(g=-4), dict(g=46341), dict(classes=0),
           dict(classes=256), dict(out_h=0), dict(out_w=0), dict(out_h=4097), dict(out_w=4097), dict(out_h=-1), dict(ld_logits=20),
           dict(image_stride=15 * 21 + 20), dict(out_image_stride=64 * 64 - 1), dict(ld_logits=32, image_stride=15 * 32 + 20)]
    for b in bad:
        assert B.dense_upsample_argmax_raw(**{**ok, **b}) == INVALID, b
    L = B.lib()
    grid_ok = [None, 0x1000, 21, 16 * 21, 0x2000, 16 * 21, 2, 4, 21]
    for pos, val in [(1, None), (4, None), (2, 20), (3, 15 * 21 + 20), (5, 16 * 21 - 1), (6, 0), (7, 0), (8, 0), (8, 256)]:
        args = list(grid_ok)
        args[pos] = val
        assert L.vithip_dense_grid_f32(*args) == INVALID, (pos, val)


def test_fold_helper_refuses_bad_arguments_and_needs_no_device():
    W, b = np.ones((2, 4), np.float32), np.zeros(2, np.float32)
    ones, zeros = np.ones(4, np.float32), np.zeros(4, np.float32)
    assert B.fold_batchnorm_raw(W.copy(), b.copy(), 2, 4, ones, zeros, zeros, ones, 1e-5) == 0
    for bad in (dict(classes=0), dict(in_features=0), dict(eps=-1.0), dict(var=zeros, eps=0.0), dict(weight=None), dict(var=None)):
        a = dict(weight=W.copy(), bias=b.copy(), classes=2, in_features=4, gamma=ones, beta=zeros, mean=zeros, var=ones, eps=1e-5)
        a.update(bad)
        assert B.fold_batchnorm_raw(**a) != 0, bad
