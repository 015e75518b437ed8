"""Attention-pool heads (vit_engine_set_map_head, VIT_FEAT_MAP): what can be checked without a GPU -- the float64 model of the GPU
tests against PyTorch's own modules, and the ABI."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import map_head_model as M
from vit_amd import binding as B
from vit_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kind", ["gelu", "gelu_tanh"])
@pytest.mark.parametrize("D,H", [(64, 1), (192, 3), (1152, 16)])
def test_model_is_torch_multihead_attention_with_the_probe_as_query_then_the_mlp_block(D, H, kind):
    import torch
    import torch.nn.functional as F

    w = synth.make_map_head(D, H, 2 * D, seed=D + H)
    t = {k: torch.from_numpy(v.astype(np.float64)) for k, v in w.items()}
    y = np.random.default_rng(D).normal(0.0, 1.0, (2, 19, D))
    mha = torch.nn.MultiheadAttention(D, H, batch_first=True, dtype=torch.float64)
    with torch.no_grad():
        mha.in_proj_weight.copy_(t["in_proj_weight"]); mha.in_proj_bias.copy_(t["in_proj_bias"])
        mha.out_proj.weight.copy_(t["out_proj_weight"]); mha.out_proj.bias.copy_(t["out_proj_bias"])
        ty = torch.from_numpy(y)
        a = mha(t["probe"].reshape(1, 1, D).repeat(2, 1, 1), ty, ty)[0][:, 0]
        hid = F.gelu(F.linear(F.layer_norm(a, (D,), t["ln_weight"], t["ln_bias"], 1e-6), t["fc1_weight"], t["fc1_bias"]),
                     approximate="tanh" if kind == "gelu_tanh" else "none")
        ref = (a + F.linear(hid, t["fc2_weight"], t["fc2_bias"])).numpy()
    got = M.head(y, w, H, kind)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


def test_model_is_transformers_siglip_pooling_head():
    tr = pytest.importorskip("transformers")
    import torch

    D, H = 64, 4
    cfg = tr.SiglipVisionConfig(hidden_size=D, num_attention_heads=H, intermediate_size=128, layer_norm_eps=1e-6)
    mod = tr.models.siglip.modeling_siglip.SiglipMultiheadAttentionPoolingHead(cfg).double().eval()
    sd = mod.state_dict()
    w = {"probe": sd["probe"], "in_proj_weight": sd["attention.in_proj_weight"], "in_proj_bias": sd["attention.in_proj_bias"],
         "out_proj_weight": sd["attention.out_proj.weight"], "out_proj_bias": sd["attention.out_proj.bias"],
         "ln_weight": sd["layernorm.weight"], "ln_bias": sd["layernorm.bias"], "fc1_weight": sd["mlp.fc1.weight"],
         "fc1_bias": sd["mlp.fc1.bias"], "fc2_weight": sd["mlp.fc2.weight"], "fc2_bias": sd["mlp.fc2.bias"]}
    y = np.random.default_rng(3).normal(0.0, 1.0, (2, 10, D))
    with torch.no_grad():
        ref = mod(torch.from_numpy(y)).numpy()
    got = M.head(y, {k: v.numpy() for k, v in w.items()}, H, "gelu_tanh")
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


def test_abi_exports_the_head_and_leaves_the_existing_structs_alone(tmp_path):
    syms = subprocess.run(["nm", "-D", "--defined-only", B.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
    for want in ("vit_engine_set_map_head", "vithip_map_pool_f32", "vithip_map_pool_f32_workspace_floats", "vithip_gelu_tanh_rows_f32"):
        assert want in names, want
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "vit_engine.h"', "int main(void) {",
             '    printf("enums %d %d %d\\n", VIT_FEAT_MAP, VIT_MAP_ACT_GELU, VIT_MAP_ACT_GELU_TANH);',
             '    printf("sizes %zu %zu %zu %zu %zu\\n", sizeof(vit_map_head_spec), sizeof(vit_map_head_weights), sizeof(vit_feature_spec), '
             'sizeof(vit_engine_options), sizeof(vit_config));']
    for st, mirror in (("vit_map_head_spec", B.CMapHeadSpec), ("vit_map_head_weights", B.CMapHeadWeights)):
        for name, *_ in mirror._fields_:
            lines.append(f'    printf("{st}.{name} %zu\\n", offsetof({st}, {name}));')
    src, exe = tmp_path / "abi.c", tmp_path / "abi"
    src.write_text("\n".join(lines + ["    return 0;", "}"]))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True, capture_output=True)
    out = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()}
    assert out["enums"] == [B.FEATURE_KINDS["map"], B.MAP_ACTS["gelu"], B.MAP_ACTS["gelu_tanh"]] == [5, 0, 1]
    assert out["sizes"] == [C.sizeof(B.CMapHeadSpec), C.sizeof(B.CMapHeadWeights), C.sizeof(B.CFeatureSpec), C.sizeof(B.COptions), C.sizeof(B.CConfig)]
    assert out["sizes"][2:] == [8, 48, 32]  # vit_feature_spec, vit_engine_options, vit_config: as before the head
    for st, mirror in (("vit_map_head_spec", B.CMapHeadSpec), ("vit_map_head_weights", B.CMapHeadWeights)):
        for name, *_ in mirror._fields_:
            assert out[f"{st}.{name}"] == [getattr(mirror, name).offset], name
