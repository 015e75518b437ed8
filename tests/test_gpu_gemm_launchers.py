"""The host side of the GEMM family (csrc/vit_gemm*.hip, vit_patch_embed_*.hip): what the launchers refuse before any launch, and
the one class-row kernel behind the four patch embeddings.

Refusals: the codes are read off the argument checks of vithip_gemm_f32 / vithip_gemm_bf16 -- every case below fails one of
them with hipErrorInvalidValue before a kernel is chosen -- and the output buffer, preset to a sentinel, must come back untouched.

Class row: every embedding entry writes x[img][0][:] = cls + pos[0] through vitgemm::launch_cls_rows.  One and three images at
the smallest geometry the entry's own tests use, embedding width 192: 192 and 576 elements, neither a multiple of the kernel's
256-thread block, so the last (or only) block is partial.  Row 0 bit for bit, the patch rows at the bar of the entry's own oracle
test, the floats behind the last row untouched.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import oracle_config
from engine_helpers import same_bits
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

INVALID = 1  # hipErrorInvalidValue
SENTINEL = 0x7FC0DEAD
M, N, K = 64, 64, 128


def sentinel(count):
    return B.DeviceArray.from_numpy(np.full(count, SENTINEL, np.uint32).view(np.float32))


def untouched(d):
    return bool((d.numpy().view(np.uint32) == SENTINEL).all())


def test_refused_gemm_calls_return_invalid_value_and_launch_nothing():
    L = B.lib()
    L.vithip_gemm_bf16.argtypes = [C.c_void_p, C.POINTER(B.CGemmBf16Args)]
    zeros = lambda count, dtype=np.float32: B.DeviceArray.from_numpy(np.zeros(count, dtype))
    dA, dW, db, dR, dRows, dCs = zeros(M * K), zeros(N * K), zeros(N), zeros(M * N), zeros(2 * M), zeros(N)
    dA16, dW16 = zeros(M * K, np.uint16), zeros(N * K, np.uint16)
    dC, dX16, dPart = sentinel(M * N), sentinel(M * N), sentinel(B.ln_strips(N) * M * 2)

    def f32(epilogue=B.EPI_BIAS, tile=0, arith=B.ARITH_F32, residual=False, ln_rows=False):
        a = B.CGemmArgs(dA.ptr, K, dW.ptr, K, db.ptr, dR.ptr if residual else None, N, dC.ptr, N, M, N, K, epilogue, tile, 0, None, 0,
                        dRows.ptr if ln_rows else None, None, None, None, arith)
        return int(L.vithip_gemm_f32(None, C.byref(a)))

    def bf16(epilogue=B.BF16_EPI_BF16, variant=0, residual=False, consumer=False, producer=False):
        a = B.CGemmBf16Args(dA16.ptr, K, dW16.ptr, K, db.ptr, dR.ptr if residual else None, N, dC.ptr, N, M, N, K, epilogue, variant,
                            dRows.ptr if consumer else None, dCs.ptr if consumer else None, dX16.ptr if producer else None, N,
                            dPart.ptr if producer else None)
        return int(L.vithip_gemm_bf16(None, C.byref(a)))

    cases = {}
    for e in (3, 4, 5, 7, 8, -1):  # the fold forms and the stats form are the library's own; 8 and -1 are no code at all
        cases[f"f32 epilogue {e}"] = lambda e=e: f32(epilogue=e)
    for t in (1, 2, 3, 4, 5, 13):
        cases[f"f32 tile {t}"] = lambda t=t: f32(tile=t)
    for t in (6, 7, 8, 12):
        cases[f"f32 split with tile {t}"] = lambda t=t: f32(tile=t, arith=B.ARITH_SPLIT3)
    cases["f32 fold with the residual epilogue"] = lambda: f32(epilogue=B.EPI_BIAS_RESIDUAL, residual=True, ln_rows=True)
    cases["bf16 variant 3"] = lambda: bf16(variant=3)
    cases["bf16 variant -1"] = lambda: bf16(variant=-1)
    cases["bf16 F32_EMBED with variant 1"] = lambda: bf16(epilogue=3, variant=1)
    cases["bf16 fold consumer with the residual epilogue"] = lambda: bf16(epilogue=B.BF16_EPI_F32_RESIDUAL, residual=True, consumer=True)
    cases["bf16 fold producer with a bf16 epilogue"] = lambda: bf16(epilogue=B.BF16_EPI_BF16, producer=True)
    cases["bf16 epilogue past the last one"] = lambda: bf16(epilogue=5)
    for name, call in cases.items():
        assert call() == INVALID, name
        B.hip_check(L.vithip_device_sync(), "sync")
        assert untouched(dC) and untouched(dX16) and untouched(dPart), name
    # the table's base calls are valid: what was refused above is the one field each case changes
    assert f32() == 0 and bf16() == 0
    B.hip_check(L.vithip_device_sync(), "sync")
    assert not untouched(dC)


def small(img, patch, chans):
    return synth.ModelConfig(img_size=img, patch_size=patch, in_chans=chans, num_classes=10, embed_dim=192, depth=1, num_heads=3, hidden_dim=192)


def bf16_round(a):
    return B.from_bf16_bits(B.to_bf16_bits(a)).reshape(a.shape)


# entry -> (geometry, bf16 operands?): the smallest of test_patch_embed's, of test_gpu_patch_embed_general's, of test_patch_embed_bf16's
ENTRIES = {
    "vithip_patch_embed_f32": (small(32, 8, 2), False),
    "vithip_patch_embed_f32_general": (small(4, 2, 1), False),
    "vithip_patch_embed_bf16": (small(64, 16, 3), True),
    "vithip_patch_embed_bf16_implicit": (small(64, 16, 3), True),
}
GUARD = 64
_cache = {}


def operands(cfg):
    """(images [3][C][S][S], [cls, conv_w, conv_b, pos]) once per geometry."""
    if cfg not in _cache:
        _cache[cfg] = (synth.make_images(cfg, 3, 6), [synth.make_weight(cfg, i, 5) for i in range(4)])
    return _cache[cfg]


def reference(oracle, cfg, bf16):
    """The oracle's embedding of the three images (bf16 entries: of the bf16-rounded pixels and conv weight), once per geometry."""
    key = ("ref", cfg, bf16)
    if key not in _cache:
        imgs, W = operands(cfg)
        Wr = [W[0], bf16_round(W[1]), W[2], W[3]] if bf16 else W
        imgs_r = bf16_round(imgs) if bf16 else imgs
        ocfg = oracle_config(cfg)
        _cache[key] = np.stack([oracle.embed(ocfg, im, Wr) for im in imgs_r])
    return _cache[key]


def run_entry(entry, cfg, imgs, W):
    """x [n][T][D] and the GUARD floats behind it, as the entry left them."""
    L = B.lib()
    n, D = imgs.shape[0], cfg.embed_dim
    bf16 = ENTRIES[entry][1]
    d_img, d_b, d_cls, d_pos = (B.DeviceArray.from_numpy(np.ascontiguousarray(a, np.float32)) for a in (imgs, W[2], W[0], W[3]))
    conv_w = W[1].reshape(D, -1)
    d_w = B.DeviceArray.from_numpy(B.to_bf16_bits(conv_w) if bf16 else np.ascontiguousarray(conv_w, np.float32))
    d_x = sentinel(n * cfg.tokens * D + GUARD)
    geometry = (n, cfg.img_size, cfg.patch_size, cfg.in_chans, D)
    fn = getattr(L, entry)
    if entry == "vithip_patch_embed_bf16":
        fn.argtypes = [C.c_void_p] * 8 + [C.c_int] * 5
        d_patches = B.DeviceArray((n * cfg.patches, cfg.patch_dim), np.uint16)
        rc = fn(None, d_img.ptr, d_w.ptr, d_b.ptr, d_cls.ptr, d_pos.ptr, d_x.ptr, d_patches.ptr, *geometry)
    else:
        fn.argtypes = [C.c_void_p] * 7 + [C.c_int] * 5
        rc = fn(None, d_img.ptr, d_w.ptr, d_b.ptr, d_cls.ptr, d_pos.ptr, d_x.ptr, *geometry)
    B.hip_check(int(rc), entry)
    out = d_x.numpy()
    return out[:-GUARD].reshape(n, cfg.tokens, D), out[-GUARD:]


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_every_patch_embedding_writes_the_shared_class_row(oracle, entry, n):
    cfg, bf16 = ENTRIES[entry]
    imgs, W = operands(cfg)
    assert (n * cfg.embed_dim) % 256 != 0
    got, guard = run_entry(entry, cfg, imgs[:n], W)
    assert (guard.view(np.uint32) == SENTINEL).all()
    assert np.isfinite(got).all()  # every element written: the sentinel is a NaN
    cls_row = (W[0] + W[3].reshape(cfg.tokens, cfg.embed_dim)[0]).astype(np.float32)
    for i in range(n):
        assert same_bits(got[i, 0], cls_row), i
    ref = reference(oracle, cfg, bf16)[:n]
    for i in range(n):  # the bars of test_patch_embed / test_general_kernel_matches_the_oracle (fp32) and of test_patch_embed_bf16
        scale = max(1.0, float(np.abs(ref[i]).max())) if bf16 else float(np.abs(ref[i]).max()) + 1e-30
        err = float(np.abs(got[i].astype(np.float64) - ref[i].astype(np.float64)).max())
        print(f"{entry} n={n} image {i}: max |d| = {err:.3e}, bar {2e-5 * scale:.3e}")
        assert err <= 2e-5 * scale, (entry, n, i, err)
