"""Position-embedding resampling (vit_engine_load_weights_resampled, vit_engine_copy_weights_resampled, vithip_pos_resample_*): what can
be checked of the interface without a GPU -- the exported symbols, vit_pos_resample against its ctypes mirror, vit_engine_options
unchanged, the enum values and the binding's argument lists.
"""
import ctypes as C
import inspect
import os
import subprocess

from vit_amd import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["vit_engine_load_weights_resampled", "vit_engine_copy_weights_resampled", "vithip_pos_resample_f32"]


def test_library_exports_the_new_entry_points_and_the_host_table():
    syms = subprocess.run(["nm", "-D", "--defined-only", B.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
    for want in ENTRY_POINTS + ["vithip_pos_resample_table"]:
        assert want in names, want


def test_pos_resample_mirror_has_the_layout_of_the_header_and_the_options_are_unchanged(tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "vit_engine.h"', '#include "vit_hip_kernels.h"', "int main(void) {",
             '    printf("size %zu\\n", sizeof(vit_pos_resample));', '    printf("options %zu\\n", sizeof(vit_engine_options));',
             '    printf("modes %d %d\\n", VIT_POS_BICUBIC, VIT_POS_BICUBIC_AA);',
             '    printf("kernel_modes %d %d\\n", VITHIP_POS_BICUBIC, VITHIP_POS_BICUBIC_AA);']
    for name, *_ in B.CPosResample._fields_:
        lines.append(f'    printf("{name} %zu\\n", offsetof(vit_pos_resample, {name}));')
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "pos.c", tmp_path / "pos"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True,
                   capture_output=True, text=True)
    out = {ln.split()[0]: ln.split()[1:] for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()}
    assert int(out["size"][0]) == C.sizeof(B.CPosResample) == 3 * C.sizeof(C.c_int)
    assert [name for name, *_ in B.CPosResample._fields_] == ["src_img_size", "mode", "reserved"]
    for name, *_ in B.CPosResample._fields_:
        assert int(out[name][0]) == getattr(B.CPosResample, name).offset, name
    assert [int(v) for v in out["modes"]] == [int(v) for v in out["kernel_modes"]] == [0, 1]
    assert B.POS_MODES == {"bicubic": 0, "bicubic_aa": 1}
    # how a checkpoint is loaded is per call: vit_engine_options gained no field (12 ints before and after)
    assert int(out["options"][0]) == C.sizeof(B.COptions) == 12 * C.sizeof(C.c_int)


def test_binding_declares_the_calls_and_keeps_the_old_ones_their_meaning():
    L = B.lib()
    assert list(L.vit_engine_load_weights_resampled.argtypes) == [C.c_void_p, C.POINTER(B.CNetwork), C.c_int, C.POINTER(B.CPosResample)]
    assert list(L.vit_engine_copy_weights_resampled.argtypes) == [C.c_void_p, C.c_void_p, C.c_int]
    assert list(L.vithip_pos_resample_f32.argtypes) == [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int]
    assert list(L.vithip_pos_resample_table.argtypes) == [C.c_int] * 3 + [C.POINTER(C.c_int)] * 2 + [C.POINTER(C.c_float), C.c_int]
    load = inspect.signature(B.Engine.load_weights).parameters
    assert list(load) == ["self", "weights", "pos_from", "pos_mode"]
    assert load["pos_from"].default is None and load["pos_mode"].default == "bicubic"
    copy = inspect.signature(B.Engine.copy_weights_from).parameters
    assert list(copy) == ["self", "other", "pos_mode"] and copy["pos_mode"].default is None
