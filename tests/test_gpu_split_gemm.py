"""The three-piece split of the fp32 GEMMs on the bf16 matrix pipe (vithip_gemm_args.arith = 1, vit_engine_options.fp32_split;
DESIGN.md 4.1.1): accuracy against float64 and against the fp32-MFMA arithmetic on the same operands, exactness where the
arithmetic promises it, the same bits on every tile code, the LayerNorm fold's hard cases, and the engine end to end.
The kernel these tests compare with (tile = 10, arith = ARITH_SPLIT3) is itself held to float64 and to a bit-exact host model in
tests/test_gpu_split_gemm_accuracy.py."""
import math
import os

import numpy as np
import pytest

from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

S = B.ARITH_SPLIT3
GOLD = os.path.join(os.path.dirname(__file__), "golden", "vit_b16_e2e.npz")


def u(k, shape, a, seed=777):
    n = int(np.prod(shape))
    return synth.uniform(seed, k, n, -a, a).reshape(shape)


def ref64(A, W, b, epi=B.EPI_BIAS, R=None):
    y = A.astype(np.float64) @ W.astype(np.float64).T + b
    if epi == B.EPI_BIAS_GELU:
        y = 0.5 * y * (1.0 + np.vectorize(math.erf)(y / math.sqrt(2.0)))
    if R is not None:
        y = y + R
    return y


def err_of(got, ref):
    return float(np.abs(got.astype(np.float64) - ref).max())


# the shapes of tests/test_gpu_ops.py::test_gemm_bias, _bias_gelu and _bias_residual, with their operand ranges
CASES = [(2, 3, 4, (M, N, K), 1.0, 0.05, B.EPI_BIAS) for M, N, K in
         [(197, 768, 768), (394, 2304, 768), (300, 1000, 768), (5, 10, 128), (129, 33, 64), (1, 1000, 768), (640, 256, 3072)]]
CASES += [(5, 6, 7, (394, 3072, 768), 1.0, 0.08, B.EPI_BIAS_GELU), (8, 9, 10, (394, 768, 3072), 1.0, 0.03, B.EPI_BIAS_RESIDUAL)]


@pytest.mark.parametrize("ka,kw,kb,shape,sa,sw,epi", CASES)
def test_split_against_float64_and_against_fp32_mfma(ka, kw, kb, shape, sa, sw, epi):
    M, N, K = shape
    A, W, b = u(ka, (M, K), sa), u(kw, (N, K), sw), u(kb, (N,), 0.1)
    R = u(11, (M, N), 2.0) if epi == B.EPI_BIAS_RESIDUAL else None
    ref = ref64(A, W, b, epi, R)
    scale = float(np.abs(ref).max())
    e1 = err_of(B.gemm(A, W, b, residual=R, epilogue=epi, arith=S), ref)
    e0 = err_of(B.gemm(A, W, b, residual=R, epilogue=epi), ref)
    print(f"{shape} epi {epi}: split {e1:.3g}, fp32 MFMA {e0:.3g} of {scale:.3g}")
    assert e1 <= 2e-5 * scale
    assert e1 <= 2 * e0 + 2.0 ** -24 * scale     # (the floor: one fp32 rounding of the output, for shapes where e0 is ~0)


@pytest.mark.parametrize("tile", [0, 9, 10, 11])
def test_split_identity_product_is_exact(tile):
    K = 256
    W = u(1, (160, K), 1.0)
    C = B.gemm(np.eye(K, dtype=np.float32), W, np.zeros(160, np.float32), tile=tile, arith=S)
    assert np.array_equal(C, W.T.copy())


def test_split_tile_codes_give_the_same_bits():
    M, N, K = 515, 200, 96
    A, W, b = u(12, (M, K), 1.0), u(13, (N, K), 0.1), u(14, (N,), 0.1)
    R = u(15, (M, N), 2.0)
    for epi, res in ((B.EPI_BIAS, None), (B.EPI_BIAS_GELU, None), (B.EPI_BIAS_RESIDUAL, R)):
        outs = [B.gemm(A, W, b, residual=res, epilogue=epi, tile=t, arith=S) for t in (0, 9, 10, 11)]
        for o in outs[1:]:
            assert np.array_equal(o, outs[0]), epi
        assert not np.array_equal(outs[0], B.gemm(A, W, b, residual=res, epilogue=epi))   # the split really ran
    for m in (7, 1):                                                # ragged M, one row: the same rows of the same products
        want = B.gemm(A, W, b, tile=10, arith=S)[:m]
        for t in (0, 9, 10, 11):
            assert np.array_equal(B.gemm(A[:m], W, b, tile=t, arith=S), want), (m, t)
    for t in (6, 7, 8, 12):
        with pytest.raises(B.VitError):
            B.gemm(A, W, b, tile=t, arith=S)
    with pytest.raises(B.VitError):
        B.gemm(A, W, b, arith=2)


def test_split_helper_pieces_are_bit_identical():
    """The persistent walk's hand-over (600 tiles on 512 workgroups) in split mode, helpers on time and late."""
    M, N, K = 128 * 100, 768, 768
    A, W, b, R = u(50, (M, K), 1.0), u(51, (N, K), 0.05), u(52, (N,), 0.1), u(53, (M, N), 2.0)
    for epi, res in ((B.EPI_BIAS_GELU, None), (B.EPI_BIAS_RESIDUAL, R)):
        ref = B.gemm(A, W, b, residual=res, epilogue=epi, tile=10, arith=S)
        for late in (0, 1):
            st = {}
            got = B.gemm(A, W, b, residual=res, epilogue=epi, tile=9, workspace=True, handover_test=late, stats=st, arith=S)
            assert np.array_equal(got, ref), (epi, late)
            assert st["taken"] + st["recomputed"] > 0, st


def test_mfma_bf16_gives_one_value_wherever_an_output_sits_in_the_block():
    """Probe: every row of A is the same vector and every row of W is the same vector, so all 64 x 64 outputs are the same dot
    product -- computed at every (row, column) position of the 32 x 32 accumulator blocks.  Operands over many binades, so that
    any position-dependent order or precision of the instruction's internal sum would show in the low bits."""
    K = 768
    rng = np.random.default_rng(5)
    a = (rng.standard_normal(K) * np.exp2(rng.integers(-12, 12, K))).astype(np.float32)
    w = (rng.standard_normal(K) * np.exp2(rng.integers(-12, 12, K))).astype(np.float32)
    A, W = np.tile(a, (64, 1)), np.tile(w, (64, 1))
    for t in (0, 10, 11):
        C = B.gemm(A, W, np.zeros(64, np.float32), tile=t, arith=S)
        assert (C.view(np.uint32) == C.view(np.uint32)[0, 0]).all(), t


def test_split_fold_on_near_constant_rows_stays_inside_its_stated_bound():
    """tests/test_gpu_lnfold.py::test_fp32_fold_on_near_constant_rows_stays_inside_its_stated_bound with arith = 1, same bar."""
    K, N = 768, 768
    spreads = [1.0, 1e-1, 1e-2]
    x = np.empty((128 * (len(spreads) + 1), K), np.float32)
    for i, sp in enumerate(spreads):
        x[128 * i:128 * (i + 1)] = u(40 + i, (128, 1), 2.0) + np.float32(sp) * u(50 + i, (128, K), 1.0)
    x[128 * len(spreads):] = np.repeat(np.array([2.0, -0.5, 0.0, 2.0], np.float32), 32)[:, None]
    gamma, beta = (1.0 + u(60, (K,), 0.5)).astype(np.float32), u(61, (K,), 0.5)
    W, b = u(62, (N, K), 0.05), u(63, (N,), 0.1)
    rows = B.rowstats_f32(x)
    x64, r64 = x.astype(np.float64), rows.astype(np.float64)
    ref = ((x64 - r64[:, 1:]) * r64[:, :1] * gamma + beta) @ W.astype(np.float64).T + b
    Wf, colsum, bias_f = B.ln_fold_weights_f32(W, b, gamma, beta)
    Wc, _, bias_c = B.ln_fold_weights_f32_centered(W, b, gamma, beta)
    for Wx, bx, cs in ((Wf, bias_f, colsum), (Wc, bias_c, None)):
        got = B.gemm(x, Wx, bx, epilogue=B.EPI_BIAS, ln=(rows, cs), arith=S).astype(np.float64)
        amp = r64[:, :1] * (np.abs(x64) @ np.abs(Wx.astype(np.float64)).T)
        err = np.abs(got - ref)
        assert np.isfinite(got).all()
        assert (err <= 8 * 2.0 ** -24 * amp + 2e-5).all(), float((err - 8 * 2.0 ** -24 * amp).max())
        assert float(err[:128].max()) <= 2e-5 * float(np.abs(ref[:128]).max())


def test_split_fold_on_real_gamma_beta_and_massive_channels():
    """tests/test_gpu_real_weights.py::test_fp32_layernorm_fold_on_real_gamma_beta_and_massive_channels with arith = 1 for the
    out_proj and the folded fc1-shaped GEMM, same bar (2e-5 x magnitude)."""
    from test_real_weights import activation_inputs, load_gold
    g = load_gold()
    seed, rows = int(g["seed"]), list(g["rows"])
    for l in g["outproj_layers"]:
        a, xres = activation_inputs(seed, int(l))
        st9 = {}
        r = B.gemm(a, g[f"outproj_w_{l}"], g[f"outproj_b_{l}"], residual=xres, epilogue=B.EPI_BIAS_RESIDUAL, tile=9, row_stats=st9,
                   arith=S)
        assert st9["in_epilogue"] == 1
        W1 = synth.uniform(seed, 900 + int(l), 512 * r.shape[1], -0.05, 0.05).reshape(512, r.shape[1])
        b1 = synth.uniform(seed, 950 + int(l), 512, -0.1, 0.1)
        ref = g[f"ln2_rows_{l}"].astype(np.float64) @ W1.astype(np.float64).T + b1
        Wc, _, bc = B.ln_fold_weights_f32_centered(W1, b1, g[f"ln2_w_{l}"], g[f"ln2_b_{l}"])
        for tile in (0, 9, 10):
            got = B.gemm(r, Wc, bc, epilogue=B.EPI_BIAS, tile=tile, ln=(st9["rows"], None), arith=S)[rows]
            err = float(np.abs(got - ref).max())
            print(f"layer {int(l)} tile {tile}: split out_proj + folded LN2 + fc1-shaped split GEMM: max |d| = {err:.3g}")
            assert err <= 2e-5 * float(np.abs(ref).max()), (int(l), tile)


def test_engine_split_golden_margin_and_switch():
    g = np.load(GOLD)
    n = int(g["n_images"])
    W = synth.make_weights(synth.VIT_B16, int(g["weight_seed"]))
    imgs = synth.make_images(synth.VIT_B16, n, int(g["image_seed"]))
    probs = {}
    for split in (0, -1):
        eng = B.Engine(synth.VIT_B16, max_batch=n, fp32_split=split)
        eng.load_weights(W)
        probs[split] = eng.forward(imgs)
        eng.close()
    err = {k: float(np.abs(p - g["probs"]).max()) for k, p in probs.items()}
    print(f"golden max |dprob|: split {err[0]:.3g}, fp32 MFMA {err[-1]:.3g}")
    assert err[0] <= 5e-6
    assert err[-1] <= 1e-4
    assert (probs[0].argmax(1) == g["probs"].argmax(1)).all()
    assert not np.array_equal(probs[0], probs[-1])          # auto is the split; -1 is the fp32-MFMA engine
