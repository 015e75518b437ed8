"""The forward surface of the C-ABI as the binding declares it: 18 exported calls, output kind x input kind x place.

The argument lists are written out one by one, as the binding declared them before it built them from their parts: tests hand raw
integers, None and byref objects straight to these functions, so every element counts.
"""
import ctypes as C
import subprocess

import pytest

from vit_amd import binding as B

V, I, F = C.c_void_p, C.c_int, B.f32p
ROWS, U8_PTRS = C.POINTER(B.f32p), C.POINTER(C.c_void_p)
RECS, PP = C.POINTER(B.CImageU8), C.POINTER(B.CPreproc)
FSP, ASP = C.POINTER(B.CFeatureSpec), C.POINTER(B.CAttentionSpec)

ARGTYPES = {
    "vit_engine_forward_device": [V, V, I, V, V, V, V],
    "vit_engine_forward_host": [V, ROWS, I, ROWS],
    "vit_engine_forward_device_u8": [V, V, I, F, F, V, V, V, V],
    "vit_engine_forward_host_u8": [V, U8_PTRS, I, F, F, ROWS],
    "vit_engine_features_device": [V, V, I, FSP, V, V],
    "vit_engine_features_host": [V, ROWS, I, FSP, ROWS],
    "vit_engine_features_device_u8": [V, V, I, F, F, FSP, V, V],
    "vit_engine_features_host_u8": [V, U8_PTRS, I, F, F, FSP, ROWS],
    "vit_engine_forward_device_images": [V, RECS, I, PP, V, V, V, V],
    "vit_engine_forward_host_images": [V, RECS, I, PP, ROWS],
    "vit_engine_features_device_images": [V, RECS, I, PP, FSP, V, V],
    "vit_engine_features_host_images": [V, RECS, I, PP, FSP, ROWS],
    "vit_engine_cls_attention_device": [V, V, I, ASP, V, V],
    "vit_engine_cls_attention_host": [V, ROWS, I, ASP, ROWS],
    "vit_engine_cls_attention_device_u8": [V, V, I, F, F, ASP, V, V],
    "vit_engine_cls_attention_host_u8": [V, U8_PTRS, I, F, F, ASP, ROWS],
    "vit_engine_cls_attention_device_images": [V, RECS, I, PP, ASP, V, V],
    "vit_engine_cls_attention_host_images": [V, RECS, I, PP, ASP, ROWS],
}
ROW_ELEMS = ("vit_engine_feature_row_elems", "vit_engine_attention_row_elems")


def test_the_library_exports_the_18_calls_and_the_two_row_widths():
    assert len(ARGTYPES) == 18
    out = subprocess.run(["nm", "-D", "--defined-only", B.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split()}
    missing = [name for name in (*ARGTYPES, *ROW_ELEMS) if name not in exported]
    assert not missing, missing


@pytest.mark.parametrize("name", sorted(ARGTYPES))
def test_argtypes_are_element_for_element_what_they_were(name):
    got = getattr(B.lib(), name).argtypes
    assert got is not None and list(got) == ARGTYPES[name], (name, got)


def test_row_width_calls_keep_their_declarations():
    L = B.lib()
    assert L.vit_engine_feature_row_elems.restype is C.c_size_t and list(L.vit_engine_feature_row_elems.argtypes) == [V, FSP]
    assert L.vit_engine_attention_row_elems.restype is C.c_size_t and list(L.vit_engine_attention_row_elems.argtypes) == [V, ASP]
