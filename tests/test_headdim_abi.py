"""What head dims other than 64 add to the ABI, checked without a GPU: the exported symbols, vithip_qscale on the accepted set and
off it, the presets, and the MAC count of ViT-H/14 from the C side."""
import ctypes as C
import os
import subprocess

import numpy as np

from vit_amd import binding as B
from vit_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCEPTED = [64] + list(range(72, 129, 8))


def bits(x) -> int:
    return int(np.float32(x).view(np.uint32))


def test_library_exports_the_new_entry_points():
    syms = subprocess.run(["nm", "-D", "--defined-only", B.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
    want = {"vithip_attention_f32_hd", "vithip_attention_bf16io_hd", "vithip_cls_attention_f32_hd", "vithip_cls_attention_bf16_hd",
            "vithip_qscale"}
    assert want <= names, sorted(want - names)


def test_qscale_of_64_has_the_bits_of_the_constant(tmp_path):
    src, exe = tmp_path / "q.c", tmp_path / "q"
    src.write_text('#include <stdio.h>\n#include <string.h>\n#include "vit_hip_kernels.h"\n'
                   'int main(void) { float q = VITHIP_QSCALE; unsigned u; memcpy(&u, &q, 4); printf("%u\\n", u); return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    macro = int(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout)
    assert bits(B.qscale(64)) == macro == bits(B.QSCALE)


def test_qscale_on_the_accepted_set_and_off_it():
    for h in range(72, 129, 8):
        want = np.float32(1 / np.sqrt(np.float64(h)) * np.log2(np.e))
        assert bits(B.qscale(h)) == bits(want), h
    for h in (32, 60, 136, 0, -8):
        assert B.qscale(h) == 0.0, h
    # every other integer from -8 to 200 is refused as well: the accepted set is exactly 64 and 72, 80 .. 128
    assert [h for h in range(-8, 201) if B.qscale(h) != 0.0] == ACCEPTED


def test_the_presets_and_their_macs():
    h, c, g = synth.VIT_H14, synth.CLIP_H14, synth.CLIP_BIGG14
    assert (h.img_size, h.patch_size, h.embed_dim, h.depth, h.num_heads, h.hidden_dim, h.num_classes, h.mlp) == (224, 14, 1280, 32, 16, 5120, 1000, "gelu")
    assert (c.patch_size, c.embed_dim, c.depth, c.num_heads, c.hidden_dim, c.num_classes, c.mlp) == (14, 1280, 32, 16, 5120, 1024, "gelu")
    assert (g.patch_size, g.embed_dim, g.depth, g.num_heads, g.hidden_dim, g.num_classes, g.mlp) == (14, 1664, 48, 16, 8192, 1280, "gelu")
    assert h.tokens == c.tokens == g.tokens == 257
    assert (h.embed_dim // h.num_heads, g.embed_dim // g.num_heads) == (80, 104)
    L = B.lib()
    for cfg in (h, c, g):
        cc = B.CConfig.of(cfg)
        assert L.vit_config_macs_per_image(C.byref(cc)) == cfg.macs_per_image
        assert [L.vit_config_weight_size(C.byref(cc), i) for i in range(cfg.n_weights)] == [int(np.prod(s)) for s in cfg.weight_shapes()]
