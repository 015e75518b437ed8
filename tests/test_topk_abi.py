"""Top-k class records (vit_engine_topk_*, vithip_softmax_topk_f32): what can be checked of the interface without a GPU -- the
exported symbols, the enum values and the layout of vit_topk_spec against a C compile, that the other structs kept their sizes, the
argument lists of the binding, the row-width query on a NULL engine, and the launcher's refusals, which come before any HIP call.
"""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np

from vit_amd import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE_CALLS = ["vit_engine_topk_device", "vit_engine_topk_host", "vit_engine_topk_device_u8", "vit_engine_topk_host_u8",
                "vit_engine_topk_device_images", "vit_engine_topk_host_images"]
ENTRY_POINTS = ["vit_engine_topk_row_elems"] + ENGINE_CALLS + ["vithip_softmax_topk_f32"]
HIP_INVALID_VALUE = 1


def test_libraries_export_the_seven_engine_symbols_and_the_launcher():
    here = os.path.dirname(B.LIB_PATH)
    for path in {B.LIB_PATH, os.path.join(here, "libvit_mi355x.so"), os.path.join(here, "libvit_mi355x_probe.so")}:
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        names = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
        for want in ENTRY_POINTS + ["vithip_softmax_top1_f32", "vit_engine_forward_device"]:
            assert want in names, (path, want)


def test_enum_values_spec_layout_and_unchanged_struct_sizes(tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "vit_engine.h"', '#include "vit_hip_kernels.h"', "int main(void) {",
             '    printf("scores %d %d\\n", VIT_SCORE_PROB, VIT_SCORE_LOGIT);',
             '    printf("kernel_scores %d %d\\n", VITHIP_SCORE_PROB, VITHIP_SCORE_LOGIT);',
             '    printf("max %d %d\\n", VIT_MAX_TOPK, VITHIP_MAX_TOPK);',
             '    printf("spec %zu %zu %zu %zu\\n", sizeof(vit_topk_spec), offsetof(vit_topk_spec, k), offsetof(vit_topk_spec, score), '
             "offsetof(vit_topk_spec, reserved));",
             '    printf("options %zu\\n", sizeof(vit_engine_options));', '    printf("config %zu\\n", sizeof(vit_config));',
             '    printf("feature %zu\\n", sizeof(vit_feature_spec));', '    printf("preproc %zu\\n", sizeof(vit_preproc));',
             "    return 0;", "}"]
    src, exe = tmp_path / "topk.c", tmp_path / "topk"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True,
                   text=True)
    out = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in
           subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()}
    assert out["scores"] == out["kernel_scores"] == [0, 1]
    assert B.SCORES == {"prob": 0, "logit": 1}
    assert out["max"] == [64, 64] and B.VIT_MAX_TOPK == 64
    S = B.CTopkSpec
    assert out["spec"] == [C.sizeof(S), S.k.offset, S.score.offset, S.reserved.offset] == [12, 0, 4, 8]
    # the choice of output is per call: no other struct gained a field
    assert out["options"] == [C.sizeof(B.COptions)] == [12 * C.sizeof(C.c_int)]
    assert out["config"] == [C.sizeof(B.CConfig)] == [8 * C.sizeof(C.c_int)]
    assert out["feature"] == [C.sizeof(B.CFeatureSpec)] == [8]
    assert out["preproc"] == [C.sizeof(B.CPreproc)] == [36]


def test_binding_declares_the_calls():
    L = B.lib()
    spec, recs, pre = C.POINTER(B.CTopkSpec), C.POINTER(B.CImageU8), C.POINTER(B.CPreproc)
    rows = C.POINTER(B.i32p)
    v, i = C.c_void_p, C.c_int
    assert list(L.vit_engine_topk_device.argtypes) == [v, v, i, spec, v, v]
    assert list(L.vit_engine_topk_host.argtypes) == [v, C.POINTER(B.f32p), i, spec, rows]
    assert list(L.vit_engine_topk_device_u8.argtypes) == [v, v, i, B.f32p, B.f32p, spec, v, v]
    assert list(L.vit_engine_topk_host_u8.argtypes) == [v, C.POINTER(v), i, B.f32p, B.f32p, spec, rows]
    assert list(L.vit_engine_topk_device_images.argtypes) == [v, recs, i, pre, spec, v, v]
    assert list(L.vit_engine_topk_host_images.argtypes) == [v, recs, i, pre, spec, rows]
    assert list(L.vit_engine_topk_row_elems.argtypes) == [v, spec] and L.vit_engine_topk_row_elems.restype == C.c_size_t
    assert list(L.vithip_softmax_topk_f32.argtypes) == [v, v, i, v, i, i, i, i, i]
    op = inspect.signature(B.softmax_topk).parameters
    assert list(op)[:5] == ["logits", "k", "score", "ld_logits", "ld_out"] and op["score"].default == "prob"
    for name in ("topk_device", "topk_host", "topk_device_u8", "topk_host_u8", "topk_device_images", "topk_host_images", "topk_shape"):
        assert callable(getattr(B.Engine, name)), name
    s = B.topk_spec(5)
    assert (s.k, s.score, s.reserved) == (5, 0, 0)
    s = B.topk_spec(3, "logit")
    assert (s.k, s.score, s.reserved) == (3, 1, 0)


def test_split_topk_takes_a_record_array_apart():
    rec = np.array([[3, 1, 0x3F000000, 0x3E800000], [0x7FFFFFFF, 0x7FFFFFFF, -0x40800000, -0x40800000]], np.int32)
    labels, scores = B.split_topk(rec)
    assert labels.dtype == np.int32 and scores.dtype == np.float32
    assert labels.tolist() == [[3, 1], [B.TOPK_EMPTY_LABEL] * 2] and scores.tolist() == [[0.5, 0.25], [-1.0, -1.0]]


def test_row_elems_of_a_null_engine_is_zero():
    L = B.lib()
    assert L.vit_engine_topk_row_elems(None, C.byref(B.topk_spec(5))) == 0
    assert L.vit_engine_topk_row_elems(None, None) == 0


def test_engine_calls_refuse_a_null_engine():
    L = B.lib()
    spec = B.topk_spec(1)
    assert L.vit_engine_topk_device(None, None, 1, C.byref(spec), None, None) == 1  # VIT_ERR_ARG
    assert L.vit_engine_topk_host(None, None, 1, C.byref(spec), None) == 1


def test_the_launcher_refuses_bad_arguments_before_any_hip_call():
    """No device is needed (or touched): every refusal comes before the launch.  The pointers are host addresses that a launch would
    fault on -- they are only compared with NULL."""
    f = B.lib().vithip_softmax_topk_f32
    logits = np.zeros((2, 10), np.float32)
    out = np.zeros((2, 20), np.int32)
    lp, op = logits.ctypes.data, out.ctypes.data
    good = dict(logits=lp, ld_logits=10, out=op, ld_out=10, rows=2, classes=10, k=5, score=0)

    def call(**kw):
        a = dict(good, **kw)
        return f(None, a["logits"], a["ld_logits"], a["out"], a["ld_out"], a["rows"], a["classes"], a["k"], a["score"])

    for bad in (dict(logits=None), dict(out=None), dict(rows=0), dict(rows=-1), dict(k=0), dict(k=-3), dict(k=11), dict(classes=4),
                dict(k=65, classes=100, ld_logits=100, ld_out=130), dict(ld_logits=9), dict(ld_out=9), dict(score=2), dict(score=-1),
                dict(classes=0, k=1), dict(classes=-5, k=1)):
        assert call(**bad) == HIP_INVALID_VALUE, bad
    assert not out.any() and not logits.any()
