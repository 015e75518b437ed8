"""The resize filter of the _images calls (vit_engine_set_resize_filter, vithip_images_u8_resize_crop_*_filter): what can be checked
of the interface without a GPU -- the exported symbols, the enum values, the setter and getter through ctypes as far as they go
without an engine (a NULL one; tests/test_gpu_preproc_bicubic.py sets real ones), the record check, the argument lists of the binding,
and that vit_preproc, vit_engine_options and vit_config kept their sizes.
"""
import ctypes as C
import inspect
import os
import subprocess

from vit_amd import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["vithip_images_u8_resize_crop_to_f32_filter", "vithip_images_u8_resize_crop_check_filter", "vit_engine_set_resize_filter",
                "vit_engine_get_resize_filter"]
VIT_ERR_ARG = 1


def test_libraries_export_the_new_entry_points_beside_the_old_ones():
    for path in (B.LIB_PATH, os.path.join(os.path.dirname(B.LIB_PATH), "libvit_mi355x.so")):
        syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        names = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
        for want in ENTRY_POINTS + ["vithip_images_u8_resize_crop_to_f32", "vithip_images_u8_resize_crop_check"]:
            assert want in names, (path, want)


def test_enum_values_and_unchanged_struct_sizes(tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "vit_engine.h"', '#include "vit_hip_kernels.h"', "int main(void) {",
             '    printf("filters %d %d\\n", VIT_RESIZE_BILINEAR, VIT_RESIZE_BICUBIC);',
             '    printf("kernel_filters %d %d\\n", VITHIP_RESIZE_BILINEAR, VITHIP_RESIZE_BICUBIC);',
             '    printf("preproc %zu %zu %zu %zu\\n", sizeof(vit_preproc), offsetof(vit_preproc, resize_shorter), offsetof(vit_preproc, mean), '
             "offsetof(vit_preproc, std));",
             '    printf("options %zu\\n", sizeof(vit_engine_options));', '    printf("config %zu\\n", sizeof(vit_config));',
             "    return 0;", "}"]
    src, exe = tmp_path / "flt.c", tmp_path / "flt"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True,
                   text=True)
    out = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in
           subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()}
    assert out["filters"] == out["kernel_filters"] == [0, 1]
    assert B.RESIZE_FILTERS == {"bilinear": 0, "bicubic": 1}
    # the filter is engine state: no struct gained a field (vit_preproc: an int and two float[4]; 12 and 8 ints)
    P = B.CPreproc
    assert out["preproc"] == [C.sizeof(P), P.resize_shorter.offset, P.mean.offset, P.std.offset] == [36, 0, 4, 20]
    assert out["options"] == [C.sizeof(B.COptions)] == [12 * C.sizeof(C.c_int)]
    assert out["config"] == [C.sizeof(B.CConfig)] == [8 * C.sizeof(C.c_int)]


def test_binding_declares_the_calls_and_keeps_the_old_ones_their_meaning():
    L = B.lib()
    recs = C.POINTER(B.CImageU8)
    assert list(L.vithip_images_u8_resize_crop_to_f32_filter.argtypes) == [C.c_void_p, recs, C.c_int, C.c_void_p] + [C.c_int] * 4 + [B.f32p] * 2
    assert list(L.vithip_images_u8_resize_crop_check_filter.argtypes) == [recs] + [C.c_int] * 5
    assert list(L.vithip_images_u8_resize_crop_to_f32.argtypes) == [C.c_void_p, recs, C.c_int, C.c_void_p] + [C.c_int] * 3 + [B.f32p] * 2
    assert list(L.vit_engine_set_resize_filter.argtypes) == [C.c_void_p, C.c_int]
    assert list(L.vit_engine_get_resize_filter.argtypes) == [C.c_void_p]
    op = inspect.signature(B.images_u8_resize_crop_to_f32).parameters
    assert list(op) == ["images", "img_size", "resize_shorter", "mean", "std", "filter"] and op["filter"].default == "bilinear"
    assert list(inspect.signature(B.Engine.set_resize_filter).parameters) == ["self", "filter"]


def test_the_record_check_knows_the_filters_without_a_gpu():
    """vithip_images_u8_resize_crop_check_filter reads the records only: the pixels are never touched."""
    L = B.lib()
    S, R = 32, 36
    recs = B.image_records([(4096, 40, 50), (4096, 64 * R, 64 * R + 9), (4096, 1, 7)])
    for flt in (0, 1):
        assert L.vithip_images_u8_resize_crop_check_filter(recs, 3, S, 3, R, flt) == 0
        assert L.vithip_images_u8_resize_crop_check_filter(B.image_records([(4096, 40, 50), (4096, 64 * R + 1, 64 * R + 1)]), 2, S, 3, R, flt) == 2
        assert L.vithip_images_u8_resize_crop_check_filter(recs, 3, S, 5, R, flt) == -1
    for flt in (-1, 2, 3):
        assert L.vithip_images_u8_resize_crop_check_filter(recs, 3, S, 3, R, flt) == -1
    assert L.vithip_images_u8_resize_crop_check(recs, 3, S, 3, R) == 0


def test_setter_and_getter_refuse_a_null_engine():
    """Without a GPU there is no engine to set a filter on (the GPU test does that); a NULL one is refused, not dereferenced."""
    L = B.lib()
    assert L.vit_engine_set_resize_filter(None, 1) == VIT_ERR_ARG
    assert L.vit_engine_get_resize_filter(None) == -1
