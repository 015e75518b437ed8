"""Linear depth heads (vit_engine_set_depth_head, VIT_DENSE_DEPTH, vithip_dense_depth_f32): what needs no GPU.

The exported symbols, vit_depth_head_spec against its ctypes mirror, and the launcher's refusals, which come before any HIP call.
"""
import ctypes as C
import os
import subprocess

import pytest

from vit_amd import binding as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1  # hipErrorInvalidValue


def test_library_exports_the_head_and_the_launcher():
    syms = subprocess.run(["nm", "-D", "--defined-only", B.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
    assert {"vit_engine_set_depth_head", "vithip_dense_depth_f32"} <= names
    assert list(B.lib().vit_engine_set_depth_head.argtypes) == [C.c_void_p, C.POINTER(B.CDepthHeadSpec), B.f32p, B.f32p, B.f32p]


def test_spec_mirror_has_the_layout_of_the_header(tmp_path):
    fields = [f[0] for f in B.CDepthHeadSpec._fields_]
    assert fields == ["num_layers", "layers", "norm", "num_bins", "upsample", "class_token", "min_depth", "max_depth", "reserved"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "vit_engine.h"', "int main(void) {",
             '    printf("size %zu\\n", sizeof(vit_depth_head_spec));', '    printf("kind %d\\n", VIT_DENSE_DEPTH);']
    lines += [f'    printf("{name} %zu\\n", offsetof(vit_depth_head_spec, {name}));' for name in fields]
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "spec.c", tmp_path / "spec"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = dict(ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(out["size"]) == C.sizeof(B.CDepthHeadSpec) == (8 + B.VIT_MAX_TAPS) * 4
    assert int(out["kind"]) == B.DENSE_KINDS["depth"] == 3
    for name in fields:
        assert int(out[name]) == getattr(B.CDepthHeadSpec, name).offset, name


OK = dict(logits_ptr=0x1000, ld_logits=64, image_stride=16 * 64, cls_ptr=0x3000, ld_cls=64, centres_ptr=0x4000, out_ptr=0x2000,
          out_image_stride=37 * 53, scratch_ptr=0x5000, images=2, g=4, bins=64, upsample=4, min_depth=0.001, max_depth=10.0, out_h=37, out_w=53)


@pytest.mark.parametrize("bad", [
    dict(logits_ptr=None), dict(centres_ptr=None), dict(out_ptr=None), dict(scratch_ptr=None), dict(images=0), dict(g=0), dict(g=46341),
    dict(bins=1), dict(bins=257), dict(upsample=0), dict(upsample=9), dict(out_h=0), dict(out_w=4097), dict(ld_logits=63), dict(ld_cls=63),
    dict(image_stride=15 * 64 + 63), dict(out_image_stride=37 * 53 - 1), dict(min_depth=0.0), dict(min_depth=10.0), dict(max_depth=float("inf")),
    dict(min_depth=float("nan"))], ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_launcher_refuses_bad_arguments_before_any_hip_call(bad):
    """No device is needed: every check comes before the first HIP call, and a refused call never reads its pointers."""
    assert B.dense_depth_raw(**{**OK, **bad}) == INVALID
