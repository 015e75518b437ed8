"""The gallery and neighbours interface (vit_engine_set_gallery, vit_engine_neighbours_*, vithip_knn_*): what can be checked without a
GPU -- the exported symbols, the layout of vit_neighbours_spec against a C compile, that vit_engine_options kept its size, the
binding's declarations, the row width of a NULL engine, the workspace's size and the launcher's refusals before any HIP call.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from vit_amd import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = [f"vit_engine_neighbours_{place}{inp}" for place in ("device", "host") for inp in ("", "_u8", "_images")]
HIP_INVALID_VALUE = 1


def test_libraries_export_the_interface():
    here = os.path.dirname(B.LIB_PATH)
    for path in {B.LIB_PATH, os.path.join(here, "libvit_mi355x.so"), os.path.join(here, "libvit_mi355x_probe.so")}:
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        names = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
        for want in CALLS + ["vit_engine_set_gallery", "vit_engine_gallery_rows", "vit_engine_neighbours_row_elems", "vithip_knn_topk_f32",
                             "vithip_knn_topk_bf16bank", "vithip_knn_workspace_bytes", "vithip_knn_slices"]:
            assert want in names, (path, want)


def test_spec_layout_and_unchanged_options(tmp_path):
    fields = ("kind", "l2_normalize", "k", "reserved")
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "vit_engine.h"', '#include "vit_hip_kernels.h"', "int main(void) {",
             '    printf("spec %zu ' + "%zu " * 4 + '\\n", sizeof(vit_neighbours_spec), ' + ", ".join(f"offsetof(vit_neighbours_spec, {f})" for f in fields) + ");",
             '    printf("max %d %d\\n", VIT_MAX_NEIGHBOURS, VITHIP_MAX_NEIGHBOURS);',
             '    printf("dtypes %d %d\\n", VIT_GALLERY_F32, VIT_GALLERY_BF16);',
             '    printf("options %zu\\n", sizeof(vit_engine_options));', '    printf("feature %zu\\n", sizeof(vit_feature_spec));',
             "    return 0;", "}"]
    src, exe = tmp_path / "nb.c", tmp_path / "nb"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in
           subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()}
    S = B.CNeighboursSpec
    assert out["spec"] == [C.sizeof(S)] + [getattr(S, f).offset for f in fields] == [16, 0, 4, 8, 12]
    assert out["max"] == [256, 256] and B.VIT_MAX_NEIGHBOURS == 256
    assert out["dtypes"] == [B.GALLERY_DTYPES["f32"], B.GALLERY_DTYPES["bf16"]] == [0, 1]
    assert out["options"] == [C.sizeof(B.COptions)] == [12 * C.sizeof(C.c_int)]
    assert out["feature"] == [C.sizeof(B.CFeatureSpec)] == [8]
    s = B.neighbours_spec(20, "mean")
    assert (s.kind, s.l2_normalize, s.k, s.reserved) == (B.FEATURE_KINDS["mean"], 1, 20, 0)


def test_binding_declares_the_calls():
    L = B.lib()
    spec, recs, pre, rows = C.POINTER(B.CNeighboursSpec), C.POINTER(B.CImageU8), C.POINTER(B.CPreproc), C.POINTER(B.i32p)
    v, i, l = C.c_void_p, C.c_int, C.c_long
    assert list(L.vit_engine_neighbours_device.argtypes) == [v, v, i, spec, v, v]
    assert list(L.vit_engine_neighbours_host.argtypes) == [v, C.POINTER(B.f32p), i, spec, rows]
    assert list(L.vit_engine_neighbours_device_u8.argtypes) == [v, v, i, B.f32p, B.f32p, spec, v, v]
    assert list(L.vit_engine_neighbours_host_u8.argtypes) == [v, C.POINTER(v), i, B.f32p, B.f32p, spec, rows]
    assert list(L.vit_engine_neighbours_device_images.argtypes) == [v, recs, i, pre, spec, v, v]
    assert list(L.vit_engine_neighbours_host_images.argtypes) == [v, recs, i, pre, spec, rows]
    assert list(L.vit_engine_set_gallery.argtypes) == [v, v, l, i, i, i]
    assert list(L.vithip_knn_topk_f32.argtypes) == list(L.vithip_knn_topk_bf16bank.argtypes) == [v, v, l, i, v, l, l, i, i, v, l, v, i]
    for name in ("set_gallery", "neighbours", "neighbours_u8", "neighbours_images", "neighbours_device", "neighbours_device_u8",
                 "neighbours_device_images"):
        assert callable(getattr(B.Engine, name)), name


def test_null_engine_and_the_workspace_size():
    L = B.lib()
    spec = B.neighbours_spec(5)
    assert L.vit_engine_neighbours_row_elems(None, C.byref(spec)) == 0 and L.vit_engine_gallery_rows(None) == 0
    assert L.vit_engine_neighbours_device(None, None, 1, C.byref(spec), None, None) == 1  # VIT_ERR_ARG
    assert L.vit_engine_set_gallery(None, None, 0, 0, 0, 0) == 1
    # O(n * slices * k) words, and the slices a launch uses: never more than asked for, than rows, or than 256
    for n, G, k, slices in ((256, 1281167, 200, 0), (1, 1000, 10, 0), (33, 129, 256, 3), (7, 2, 1, 3), (5, 10 ** 6, 4, 256)):
        S = L.vithip_knn_slices(n, G, slices)
        assert 1 <= S <= min(256, G) and (slices == 0 or S <= slices), (n, G, slices, S)
        assert L.vithip_knn_workspace_bytes(n, G, k, slices) == n * S * 2 * k * 4
    assert L.vithip_knn_slices(33, 129, 3) == 3 and L.vithip_knn_slices(256, 1281167, 0) > 8
    assert L.vithip_knn_workspace_bytes(1, 10, 257, 0) == 0 and L.vithip_knn_workspace_bytes(1, 2 ** 31 - 1, 1, 0) == 0


def test_the_launcher_refuses_bad_arguments_before_any_hip_call():
    """No device is needed (or touched): every refusal comes before the launch.  The pointers are host addresses, only compared with
    NULL and checked for alignment."""
    L = B.lib()
    q, bank, rec, ws = np.zeros((4, 16), np.float32), np.zeros((64, 16), np.float32), np.zeros((4, 12), np.int32), np.zeros(4096, np.int32)
    assert q.ctypes.data % 16 == 0 and bank.ctypes.data % 16 == 0
    good = dict(q=q.ctypes.data, ldq=16, n=4, bank=bank.ctypes.data, ldb=16, G=64, D=16, k=5, rec=rec.ctypes.data, ldr=12, ws=ws.ctypes.data, slices=2)
    for f in (L.vithip_knn_topk_f32, L.vithip_knn_topk_bf16bank):
        for bad in (dict(q=None), dict(bank=None), dict(rec=None), dict(ws=None), dict(n=0), dict(G=0), dict(G=2 ** 31 - 1), dict(D=12), dict(D=0),
                    dict(D=4104, ldq=4104, ldb=4104), dict(k=0), dict(k=257, ldr=600), dict(slices=-1), dict(slices=257), dict(ldq=12),
                    dict(ldq=18), dict(ldb=12), dict(ldb=20 if f is L.vithip_knn_topk_bf16bank else 18), dict(ldr=9), dict(q=q.ctypes.data + 4)):
            a = dict(good, **bad)
            assert f(None, a["q"], a["ldq"], a["n"], a["bank"], a["ldb"], a["G"], a["D"], a["k"], a["rec"], a["ldr"], a["ws"], a["slices"]) == HIP_INVALID_VALUE, bad
    assert not rec.any()
