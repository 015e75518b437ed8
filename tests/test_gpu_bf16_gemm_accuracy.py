"""The bf16 GEMMs (vithip_gemm_bf16: the two-stage and the ping-pong kernel), the LayerNorm fold in their epilogues and the bf16 patch
embeddings, bit for bit on operands whose accumulator is exact, and against float64 at bars of the size of fp32 rounding.
tests/test_gpu_bf16.py and tests/test_gpu_lnfold.py hold them to 2^-8 |ref| + 1e-5 and 2e-5 |ref|max: a store that truncates, a bias of
the other tile parity on one tile or a row pair taken eight rows off passes those (tests/test_bf16_gemm_model.py shows which check
here rejects each).  bf16_gemm_model (G) holds the operand families, the epilogue models and the bars; its docstring states them.

  integer family   A in {-1, 0, 1}, W in {-2 .. 2}: the accumulator is the exact integer A . W^T in any order, every epilogue a short
                   chain of fp32 operations on it -- BF16 (fractional bias), F32_RESIDUAL (aliased and not), the fold consumer on given
                   (rstd, mean*rstd) pairs and column sums, the fold producer (C, x16, every strip partial; the finalised pairs against
                   float64) and both patch embeddings have the model's bits.
  sweeps           GELU and QuickGELU on fp32 pre-activations dense over [-8, 8], passed through a GEMM with one non-zero product:
                   GELU inside 5 % of half a bf16 ulp of the float64 value for y >= -4 sqrt 2 (include/vit_hip_kernels.h), in
                   [-4.5e-8, 0] below; QuickGELU inside d = 0.1006 % of half a bf16 ulp (twice what the five-step sequence shows on the
                   CPU with +-1 ulp on v_exp_f32 and v_rcp_f32); and the share of outputs that are not rne_bf16 of the float64 value
                   below twice the emulation's.
  random family    bf16-rounded uniform operands against float64: e <= 4 e_seq + 2^-23 |ref|max for fp32 outputs, bf16 outputs between
                   rne_bf16(ref - bar) and rne_bf16(ref + bar); the fold consumer with its own normaliser.

Shapes (G.SHAPES, G.PERSISTENT): 2 x 3 tiles with ragged M and N % 8 == 4 at K = 128, 192, 448; the model's K = 768 and 3072; less than
one tile; and 342 tiles on 256 workgroups.  Both kernels wherever they take the case (K >= 128 for the ping-pong kernel, no fold in the
two-stage one).  Measured on the MI355X: profiles/r33/bf16_gemm_accuracy.md.
"""
import functools
import time

import numpy as np
import pytest

import bf16_gemm_model as G
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

KERNELS = {1: "two-stage", 2: "ping-pong"}
PP = 2


@pytest.fixture(scope="module", autouse=True)
def wall_time():
    t0 = time.perf_counter()
    yield
    print(f"\ntest_gpu_bf16_gemm_accuracy.py: {time.perf_counter() - t0:.1f} s wall time")


def case_id(v):
    if isinstance(v, tuple):
        return "x".join(str(i) for i in v)
    if isinstance(v, bool):
        return "padded" if v else "dense"
    return KERNELS.get(v, str(v))


def cases(shapes, variants=(1, 2), padded=True):
    """(variant, shape, padded leading dimensions) wherever the kernel takes the shape; the padded form on the first shape only."""
    out = [(v, s, False) for v in variants for s in shapes if v == 1 or s[2] >= 128]
    return out + ([(v, shapes[0], True) for v in variants] if padded else [])


def pads(M, N, K, padded, *names):
    full = dict(lda=K + G.PADS["lda"], ldw=K + G.PADS["ldw"], ldc=N + G.PADS["ldc"], ldr=N + G.PADS["ldr"], ldx16=N + G.PADS["ldx16"])
    return {k: full[k] for k in names} if padded else {}


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def exact(got, want, what):
    n, first = G.mismatch(got, want)
    assert n == 0, f"{what}: {n} of {np.size(want)} differ, the first at {first}: got {np.asarray(got)[first]!r}, want {np.asarray(want)[first]!r}"


def need_more_tiles_than_workgroups(shape):
    if shape == G.PERSISTENT:
        cus = B.device_info()["compute_units"]
        tiles = -(-shape[0] // G.TILE) * -(-shape[1] // G.TILE)
        if tiles <= cus:
            pytest.skip(f"{tiles} tiles do not exceed the {cus} workgroups of this device: the persistent walk would not cross a tile boundary")


ALL = G.SHAPES + [G.PERSISTENT]
FOLD = [s for s in ALL if s[2] >= 128]


# ---- integer family --------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def integer_case(shape):
    M, N, K = shape
    A, W = G.integer_operands(M, N, K)
    bias, R = G.bias_residual(M, N, integer=False)
    return frozen(B.to_bf16_bits(A).reshape(M, K), B.to_bf16_bits(W).reshape(N, K), G.exact_acc(A, W), bias, R)


@pytest.mark.parametrize("variant,shape,padded", cases(ALL), ids=case_id)
def test_integer_bf16(variant, shape, padded):
    need_more_tiles_than_workgroups(shape)
    Ab, Wb, acc, bias, _ = integer_case(shape)
    got = B.gemm_bf16(Ab, Wb, bias, epilogue=B.BF16_EPI_BF16, variant=variant, **pads(*shape, padded, "lda", "ldw", "ldc"))
    y = G.f32(acc) + bias[None, :]
    assert float((G.rne_bf16(y) != y).mean()) > 0.9             # the bias is fractional: the store really rounds
    exact(got, G.bits16(y), "BF16")


@pytest.mark.parametrize("in_place", [False, True], ids=["separate", "in-place"])
@pytest.mark.parametrize("variant,shape,padded", cases(ALL), ids=case_id)
def test_integer_f32_residual(variant, shape, padded, in_place):
    need_more_tiles_than_workgroups(shape)
    Ab, Wb, acc, bias, R = integer_case(shape)
    got = B.gemm_bf16(Ab, Wb, bias, residual=R, epilogue=B.BF16_EPI_F32_RESIDUAL, variant=variant, in_place=in_place,
                      **pads(*shape, padded, "lda", "ldw", "ldc", *(() if in_place else ("ldr",))))
    exact(got, G.epi_f32_residual(acc, bias, R), "F32_RESIDUAL")


@pytest.mark.parametrize("variant,shape,padded", cases(FOLD, variants=(PP,)), ids=case_id)
def test_integer_fold_consumer(variant, shape, padded):
    """(rstd, mean*rstd) pairs and column sums given directly: rstd log-spaced over 0.05 .. 1e3, mean*rstd of both signs."""
    need_more_tiles_than_workgroups(shape)
    M, N, K = shape
    Ab, Wb, acc, bias, _ = integer_case(shape)
    rows, colsum = G.consumer_rows(M), G.u(16, (N,), -8.0, 8.0)
    assert rows[:, 0].min() < 0.06 and rows[:, 0].max() > 900 and rows[:, 1].min() < 0 < rows[:, 1].max()
    got = B.gemm_bf16(Ab, Wb, bias, epilogue=B.BF16_EPI_BF16, variant=variant, ln_rows=rows, ln_colsum=colsum,
                      **pads(*shape, padded, "lda", "ldw", "ldc"))
    exact(got, G.epi_consumer(acc, rows, colsum, bias), "fold consumer")


@functools.lru_cache(maxsize=None)
def producer_case(shape):
    return G.producer_case(*shape)


def ldx16_min(N):
    return -(-N // 8) * 8   # x16 rows take 16-byte stores: the entry point wants ldx16 % 8 == 0, so N % 8 == 4 has four columns of padding


@pytest.mark.parametrize("in_place", [False, True], ids=["separate", "in-place"])
@pytest.mark.parametrize("variant,shape,padded", cases(G.PRODUCER_SHAPES + [G.PERSISTENT], variants=(PP,)), ids=case_id)
def test_integer_fold_producer(variant, shape, padded, in_place):
    """C, x16 and every strip partial -- the strips behind N and the rows of the ragged last tile row among them -- are exact integers;
    the finalised pairs against float64 on the same exact sums at 4 e_seq + 2^-23 |ref|, with VITHIP_LN_EPS and with CLIP's 1e-5."""
    need_more_tiles_than_workgroups(shape)
    M, N, K = shape
    c = producer_case(shape)
    ld = {"ldx16": ldx16_min(N), **pads(*shape, padded, "lda", "ldw", "ldc", "ldx16", *(() if in_place else ("ldr",)))}
    C, x16, part = B.gemm_bf16(B.to_bf16_bits(c["A"]).reshape(M, K), B.to_bf16_bits(c["W"]).reshape(N, K), c["bias"], residual=c["R"],
                               epilogue=B.BF16_EPI_F32_RESIDUAL, variant=variant, ln_producer=True, in_place=in_place, **ld)
    exact(C, c["C"], "C")
    exact(x16, c["x16"], "x16")
    assert part.shape == (G.ln_strips(N), M, 2)
    exact(part, c["partials"], "strip partials")
    s, ss = c["partials"][:, :, 0].sum(axis=0, dtype=np.float64), c["partials"][:, :, 1].sum(axis=0, dtype=np.float64)
    for eps in (None, 1e-5):
        want = G.rows_f64(s, ss, N, eps)
        bar = G.rows_bar(G.rows_f32_seq(s, ss, N, eps), want)
        e = np.abs(B.rowstats_finalize(part, N, eps=eps).astype(np.float64) - want)
        print(f"finalised pairs {shape} eps={eps}: max e / bar = {float((e / bar).max()):.3f}")
        assert (e <= bar).all(), float((e / bar).max())


EMBED = {"vit-small x 5": (synth.VIT_SMALL, 5),
         "patch dim 128 x 7": (synth.ModelConfig(img_size=72, patch_size=8, in_chans=2, embed_dim=260, depth=1, num_heads=1, hidden_dim=64), 7)}


@pytest.mark.parametrize("implicit", [False, True], ids=["two-pass", "implicit-gemm"])
@pytest.mark.parametrize("name", list(EMBED))
def test_integer_patch_embed(name, implicit):
    """F32_EMBED and the implicit GEMM: (acc + conv_b) + pos, the class row cls + pos[0].  ViT-Small x 5: 80 GEMM rows of five images in
    one tile, the row cursor steps across four image boundaries; 2 x 8 x 8 patches: the shortest K (128), 81 patches per image (no
    multiple of the cursor's 8-row step), 567 rows in three tile rows, 260 columns in two tile columns."""
    cfg, n = EMBED[name]
    c = G.embed_case(cfg, n)
    got = B.patch_embed_bf16(cfg, c["images"], c["conv_w"], c["conv_b"], c["cls"], c["pos"], implicit=implicit)
    exact(got, c["x"], "patch embedding")


# ---- GELU and QuickGELU through the GEMM --------------------------------------------------------------------------------------------------

def run_sweep(variant, epilogue):
    a, bias, y = G.sweep_gemm()
    A, W = G.sweep_operands(a, bias.size, 128 if variant == PP else 64)
    got = B.gemm_bf16(B.to_bf16_bits(A).reshape(A.shape), B.to_bf16_bits(W).reshape(W.shape), bias, epilogue=epilogue, variant=variant)
    return y, got


@pytest.mark.parametrize("variant", [1, 2], ids=case_id)
def test_gelu_sweep(variant):
    """65,792 fp32 pre-activations over [-8, 8.06].  Above the clamp: inside 5 % of half a bf16 ulp of the float64 GELU (the header's
    promise; the emulation shows 1.65 %), and no more than twice the emulation's share of outputs (0.18 %) off rne_bf16 of it -- the
    cap that keeps a systematic half-ulp bias from hiding in the interval.  Below the clamp: in [-4.5e-8, 0]."""
    y, got = run_sweep(variant, B.BF16_EPI_BF16_GELU)
    keep = y.astype(np.float64) >= -G.CLAMP
    g = G.gelu_f64(y)
    ok = G.in_interval(got, g, G.GELU_HEADER_SHARE * G.half_ulp_bf16(g))
    assert ok[keep].all(), (int((~ok[keep]).sum()), y[keep][~ok[keep]][:8])
    low = B.from_bf16_bits(got).reshape(got.shape)[~keep]
    assert low.size > 1000 and ((low >= -G.GELU_FLOOR_GPU) & (low <= 0)).all(), (float(low.min()), float(low.max()))
    share, cap = G.differ_share(got[keep], g[keep]), 2.0 * G.emulated_differ_share(y[keep], "gelu")
    print(f"GELU sweep, {KERNELS[variant]}: {100 * share:.3f} % of the outputs are not rne_bf16(gelu), cap {100 * cap:.3f} %")
    assert share < cap


@pytest.mark.parametrize("variant", [1, 2], ids=case_id)
def test_quick_gelu_sweep(variant):
    """The same sweep: inside d = 0.1006 % of half a bf16 ulp of y / (1 + exp(-1.702 y)) in float64 (G.quick_gelu_d_share: twice the
    five-step sequence's 0.0503 % under +-1 ulp on v_exp_f32 and v_rcp_f32), and the differ-share cap."""
    y, got = run_sweep(variant, B.BF16_EPI_BF16_QGELU)
    g = G.quick_gelu_f64(y)
    ok = G.in_interval(got, g, G.quick_gelu_d_share() * G.half_ulp_bf16(g))
    assert ok.all(), (int((~ok).sum()), y[~ok][:8])
    share, cap = G.differ_share(got, g), 2.0 * G.emulated_differ_share(y, "quickgelu")
    print(f"QuickGELU sweep, {KERNELS[variant]}: {100 * share:.4f} % of the outputs are not rne_bf16(q), cap {100 * cap:.4f} %")
    assert share < cap


# ---- random family -------------------------------------------------------------------------------------------------------------------------

RANDOM = G.RANDOM_SHAPES + [G.PERSISTENT]


def seq_rows(M):
    return np.arange(M) if M <= 512 else G.sample_rows(M)


@functools.lru_cache(maxsize=None)
def random_case(shape):
    """Operands, float64 references and bars, once per shape.  e_seq of the large case is taken on a sample of rows (G.sample_rows)."""
    M, N, K = shape
    A, W = G.random_operands(M, N, K)
    bias, R = G.u(17, (N,), -0.1, 0.1), G.u(18, (M, N), -2.0, 2.0)
    rows = seq_rows(M)
    chain = G.fma_chain(A[rows], W)
    ref, refR = G.ref64(A, W, bias), G.ref64(A, W, bias, R)
    y = chain + bias[None, :]
    bar = 4.0 * float(np.abs(y - ref[rows]).max()) + 2.0 ** -23 * float(np.abs(ref).max())
    yR = y + R[rows]
    barR = 4.0 * float(np.abs(yR - refR[rows]).max()) + 2.0 ** -23 * float(np.abs(refR).max())
    # the producer's pairs: float64 statistics of the float64 rows; e_seq from the sequential C, its sequential sums and finish
    want = G.rows_f64(refR.sum(axis=1), (refR * refR).sum(axis=1), N)
    seq_pairs = G.rows_f32_seq(*G.seq_sums(yR), N)
    pairs_bar = 4.0 * np.abs(seq_pairs - want[rows]).max(axis=0)[None, :] + 2.0 ** -23 * np.abs(want)
    return dict(Ab=B.to_bf16_bits(A).reshape(M, K), Wb=B.to_bf16_bits(W).reshape(N, K), bias=bias, R=frozen(R), ref=frozen(ref),
                refR=frozen(refR), bar=bar, barR=barR, pairs=want, pairs_bar=pairs_bar)


@pytest.mark.parametrize("variant,shape,padded", cases(RANDOM, padded=False), ids=case_id)
def test_random_bf16(variant, shape, padded):
    need_more_tiles_than_workgroups(shape)
    c = random_case(shape)
    got = B.gemm_bf16(c["Ab"], c["Wb"], c["bias"], epilogue=B.BF16_EPI_BF16, variant=variant)
    ok = G.in_interval(got, c["ref"], c["bar"])
    print(f"BF16 {shape} {KERNELS[variant]}: bar {c['bar']:.3e} ({c['bar'] / float(np.abs(c['ref']).max()):.2e} |ref|max), "
          f"{100 * G.differ_share(got, c['ref']):.3f} % of the outputs are not rne_bf16(ref)")
    assert ok.all(), (int((~ok).sum()), tuple(np.argwhere(~ok)[0]))


@pytest.mark.parametrize("variant,shape,padded", cases(RANDOM, padded=False), ids=case_id)
def test_random_f32_residual(variant, shape, padded):
    need_more_tiles_than_workgroups(shape)
    c = random_case(shape)
    got = B.gemm_bf16(c["Ab"], c["Wb"], c["bias"], residual=c["R"], epilogue=B.BF16_EPI_F32_RESIDUAL, variant=variant)
    e = float(np.abs(got - c["refR"]).max())
    print(f"F32_RESIDUAL {shape} {KERNELS[variant]}: e {e:.3e}, bar {c['barR']:.3e} ({c['barR'] / float(np.abs(c['refR']).max()):.2e} |ref|max)")
    assert e <= c["barR"]


@pytest.mark.parametrize("shape", RANDOM, ids=case_id)
def test_random_fold_producer_pairs(shape):
    """C inside its bar, x16 = rne_bf16 of the stored C bit for bit, and the finalised pairs against the float64 statistics of the float64
    rows at 4 e_seq + 2^-23 |ref| (e_seq: the sequential C, its sequential sums, the fp32 finish)."""
    need_more_tiles_than_workgroups(shape)
    c = random_case(shape)
    C, x16, part = B.gemm_bf16(c["Ab"], c["Wb"], c["bias"], residual=c["R"], epilogue=B.BF16_EPI_F32_RESIDUAL, variant=PP, ln_producer=True,
                               ldx16=ldx16_min(shape[1]))
    assert float(np.abs(C - c["refR"]).max()) <= c["barR"]
    exact(x16, G.bits16(C), "x16 against the stored C")
    e = np.abs(B.rowstats_finalize(part, shape[1]).astype(np.float64) - c["pairs"])
    print(f"producer's pairs {shape}: max e / bar = {float((e / c['pairs_bar']).max()):.3f}")
    assert (e <= c["pairs_bar"]).all(), float((e / c["pairs_bar"]).max())


@pytest.mark.parametrize("shape", RANDOM, ids=case_id)
def test_random_fold_consumer(shape):
    """As the engine runs it: vithip_rowstats_bf16 and vithip_ln_fold_weights make the operands (rows whose mean is as large as their
    spread), the reference is float64 on exactly those operands, the bar (4 max e_seq / norm + 2^-23) norm per element."""
    need_more_tiles_than_workgroups(shape)
    M, N, K = shape
    x, W, b, g, beta = G.fold_inputs(M, N, K)
    x16, rows = B.rowstats_bf16(x)
    Wf, cs, bf = B.ln_fold_weights(W, b, g, beta)
    got = B.gemm_bf16(x16, Wf, bf, epilogue=B.BF16_EPI_BF16, variant=PP, ln_rows=rows, ln_colsum=cs)
    xa, wa = B.from_bf16_bits(x16).reshape(M, K), B.from_bf16_bits(Wf).reshape(N, K)
    ref, norm = G.consumer_ref64(xa, wa, rows, cs, bf), G.consumer_norm(xa, wa, rows, cs, bf)
    r = seq_rows(M)
    share = G.consumer_share(G.consumer_seq(xa[r], wa, rows[r], cs, bf), ref[r], norm[r])
    ok = G.in_interval(got, ref, share * norm)
    print(f"fold consumer {shape}: bar {share:.3e} of the normaliser, {100 * G.differ_share(got, ref):.3f} % of the outputs are not rne_bf16(ref)")
    assert ok.all(), (int((~ok).sum()), tuple(np.argwhere(~ok)[0]))


# ---- the row kernels that feed the fold ------------------------------------------------------------------------------------------------------

ROWS = [(197, 768), (5, 64), (77, 1024)]


@pytest.mark.parametrize("eps", [None, 1e-5], ids=["eps=1e-6", "eps=1e-5"])
@pytest.mark.parametrize("rows,dim", ROWS)
def test_rowstats_bf16_against_float64(rows, dim, eps):
    x = G.u(40, (rows, dim), -2.0, 2.0) + G.u(41, (rows, 1), -1.0, 1.0)
    x16, rs = B.rowstats_bf16(x, eps=eps)
    exact(x16, G.bits16(x), "x16")
    x64 = x.astype(np.float64)
    want = G.rows_f64(x64.sum(axis=1), (x64 * x64).sum(axis=1), dim, eps)
    bar = G.rows_bar(G.rows_f32_seq(*G.seq_sums(x), dim, eps), want)
    e = np.abs(rs.astype(np.float64) - want)
    print(f"rowstats_bf16 ({rows}, {dim}) eps={eps}: max e / bar = {float((e / bar).max()):.3f}")
    assert (e <= bar).all(), float((e / bar).max())


@pytest.mark.parametrize("eps", [None, 1e-5], ids=["eps=1e-6", "eps=1e-5"])
@pytest.mark.parametrize("rows,dim", ROWS)
def test_layernorm_bf16out_against_float64(rows, dim, eps):
    x = G.u(42, (rows, dim), -3.0, 3.0) + np.float32(0.5)
    g, b = G.u(43, (dim,), 0.5, 1.5), G.u(44, (dim,), -0.5, 0.5)
    got = B.layernorm_bf16out(x, g, b, eps=eps)
    ref = G.layernorm_f64(x, g, b, eps)
    bar = G.bar_f32(G.layernorm_f32_seq(x, g, b, eps), ref)
    ok = G.in_interval(got, ref, bar)
    print(f"layernorm_bf16out ({rows}, {dim}) eps={eps}: bar {bar:.3e}, {100 * G.differ_share(got, ref):.3f} % of the outputs are not rne_bf16(ref)")
    assert ok.all(), (int((~ok).sum()), tuple(np.argwhere(~ok)[0]))
