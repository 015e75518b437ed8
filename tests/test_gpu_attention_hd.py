"""The attention kernels for head dims other than 64 (csrc/vit_attention_hd.hip) against the oracle's attention_core, which is general
in head_dim, and the class-token kernels against a float64 restatement.  Bars: the ones of tests/test_gpu_ops.py::test_attention*
(fp32) and tests/test_gpu_bf16.py::test_attention_bf16_io (bf16), which do not depend on head_dim.

The kernel streams K / V in chunks of 64 (bf16) or 32 (fp32) keys and works on 32-key tiles and 128-row query blocks: the token
counts sit below, at and above 32, 64, 128 and 256.
"""
import numpy as np
import pytest

import strided as S
from headdim_model import cls_attention_ref
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

INVALID = 1  # hipErrorInvalidValue
HEAD_DIMS = [72, 80, 88, 96, 104, 112, 120, 128]
TOKENS_F32 = [1, 5, 31, 32, 33, 64, 65, 129, 197, 257, 577]
TOKENS_BF16 = [1, 33, 65, 197, 257, 577]


def u(k, shape, a, seed=2020):
    n = int(np.prod(shape))
    return synth.uniform(seed, k, n, -a, a).reshape(shape)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(S.as_bits(a), S.as_bits(b))


def oracle_attention(oracle, qkv, n, T, heads):
    """[n][T][D] fp32: attention_core image by image on the columns [Q | K | V] of qkv [n * T][3D]."""
    D = qkv.shape[1] // 3
    out = []
    for i in range(n):
        blk = qkv[i * T:(i + 1) * T]
        q, k, v = (np.ascontiguousarray(blk[:, j * D:(j + 1) * D], np.float32) for j in range(3))
        out.append(oracle.attention_core(q, k, v, heads))
    return np.stack(out)


def bf16_case(vals, hd, heads, q_scaled):
    """(bits the kernel reads, the values the reference reads): vals rounded to bf16; q_scaled: the Q columns hold qscale(hd) * q and
    the reference divides the ROUNDED columns by it again."""
    D = heads * hd
    vals = np.array(vals, np.float32)
    qs = np.float32(B.qscale(hd))
    if q_scaled:
        vals[:, :D] *= qs
    bits = B.to_bf16_bits(vals)
    ref_in = B.from_bf16_bits(bits)
    if q_scaled:
        ref_in[:, :D] /= qs
    return bits, ref_in


def run(kind, qkv, n, T, heads, hd, **kw):
    """One launch of kind "f32" | "bf16" | "qscaled" on qkv (fp32 values, or bf16 bits); the output in the input's type."""
    if kind == "f32":
        return B.attention_hd(qkv, n, T, heads, hd, **kw)
    return B.attention_bf16io_hd(qkv, n, T, heads, hd, q_scaled=kind == "qscaled", **kw)


# ---- 1: fp32 against the oracle ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_fp32_matches_the_oracle(oracle, hd):
    """The reference's order of operations; the accuracy test, against float64 at fp32-level bars: tests/test_gpu_attention_accuracy.py."""
    heads, n = 2, 2
    D = heads * hd
    for T in TOKENS_F32:
        qkv = u(30 + T, (n * T, 3 * D), 1.5)
        got = B.attention_hd(qkv, n, T, heads, hd).reshape(n, T, D)
        ref = oracle_attention(oracle, qkv, n, T, heads)
        for i in range(n):
            err, top = float(np.abs(got[i] - ref[i]).max()), max(1.0, float(np.abs(ref[i]).max()))
            print(f"fp32 head_dim {hd} T {T} image {i}: {err:.3e} (bar {(1e-5 if T <= 224 else 2e-5) * top:.3e})")
            assert err <= (1e-5 if T <= 224 else 2e-5) * top, (hd, T, i, err)


# ---- 2, 3: peaked rows; the running maximum moves ----------------------------------------------------------------------------------

@pytest.mark.parametrize("hd", [80, 128])
def test_fp32_peaked_rows(oracle, hd):
    """Large scores: the max subtraction must keep the exponential in range."""
    n, T, heads = 1, 197, 2
    qkv = u(31, (T, 3 * heads * hd), 8.0)
    got = B.attention_hd(qkv, n, T, heads, hd)
    ref = oracle_attention(oracle, qkv, n, T, heads)[0]
    assert np.isfinite(got).all()
    err = float(np.abs(got - ref).max())
    print(f"peaked rows head_dim {hd}: {err:.3e} (bar {2e-4 * float(np.abs(ref).max()):.3e})")
    assert err <= 2e-4 * float(np.abs(ref).max())


@pytest.mark.parametrize("hd", [80, 104])
def test_fp32_running_maximum_moves(oracle, hd):
    """The construction of test_attention_chunked_running_max_moves: the row maximum sits in the last tenth of the sequence."""
    T, heads = 500, 1
    qkv = u(33, (T, 3 * hd), 1.0)
    qkv[450:, hd:2 * hd] *= 6.0  # large keys at the end of the sequence
    got = B.attention_hd(qkv, 1, T, heads, hd)
    ref = oracle_attention(oracle, qkv, 1, T, heads)[0]
    err = float(np.abs(got - ref).max())
    print(f"running maximum head_dim {hd}: {err:.3e} (bar {2e-5 * float(np.abs(ref).max()):.3e})")
    assert err <= 2e-5 * float(np.abs(ref).max())


# ---- 4: bf16 -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("q_scaled", [False, True], ids=["plain-q", "qscaled"])
@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_bf16_matches_the_oracle(oracle, hd, q_scaled):
    """The bar of test_attention_bf16_io: 2^-8 |ref| for the one rounding of the output + 1e-3, sized there for a P rounded to bf16
    once (sum_j |dp_j v_j| <~ 2^-9 |v| sqrt(sum p^2), a statistical allowance: the worst case is 2^-9 max |v| = 2.9e-3).  This test
    draws about 1.2 million outputs, the short sequences (33 and 65 keys, where sum p^2 is largest) among them, and a P rounded once
    does not stay inside: a float64 model of that arithmetic is outside by 1 - 2 elements for 36 of 38 seeds, and the kernel's first
    version was on the same elements (head_dim 96, T 33: 3.55e-5 over).  So the kernel multiplies V with P in two bf16 pieces,
    bf16(p) and bf16(p - bf16(p)); measured: worst |d| 1.95e-3, every element at least 9.99e-4 inside the bar (the output's rounding
    is all that is left)."""
    heads, n = 2, 2
    D = heads * hd
    missed = []
    for T in TOKENS_BF16:
        bits, ref_in = bf16_case(u(13 + T, (n * T, 3 * D), 1.5), hd, heads, q_scaled)
        got = B.from_bf16_bits(B.attention_bf16io_hd(bits, n, T, heads, hd, q_scaled=q_scaled)).reshape(n, T, D)
        ref = oracle_attention(oracle, ref_in, n, T, heads)
        over = np.abs(got - ref) - (2.0 ** -8 * np.abs(ref) + 1e-3)
        print(f"bf16 head_dim {hd} T {T} q_scaled {q_scaled}: max |d| {float(np.abs(got - ref).max()):.3e}, worst margin {float(over.max()):.3e}")
        if not (over <= 0).all():
            missed.append((T, int((over > 0).sum()), float(over.max())))
    assert not missed, f"head_dim {hd}: (T, elements over the bar, worst excess) = {missed}"


@pytest.mark.parametrize("q_scaled", [False, True], ids=["plain-q", "qscaled"])
def test_bf16_rising_scores_move_the_maximum(oracle, q_scaled):
    """The input of test_attention_bf16_streamed_reference_maximum_moves at head_dim 80: every row's score rises along the keys (the
    second head's fall), so the running maximum moves in every tile and O and the row sum are rescaled every time."""
    heads, n, T, hd = 2, 1, 300, 80
    D = heads * hd
    rng = np.random.default_rng(5)
    j = np.arange(T, dtype=np.float32)[:, None] / T
    rate = np.linspace(0.3, 1.0, T, dtype=np.float32)[:, None]
    q = np.concatenate([rate * 2.0 * np.ones((T, hd), np.float32), -rate * 2.0 * np.ones((T, hd), np.float32)], axis=1)
    k = np.concatenate([j * 6.0 * np.ones((T, hd), np.float32), j * 6.0 * np.ones((T, hd), np.float32)], axis=1)
    q += rng.uniform(-0.05, 0.05, q.shape).astype(np.float32)
    k += rng.uniform(-0.05, 0.05, k.shape).astype(np.float32)
    v = rng.uniform(-1.5, 1.5, (T, D)).astype(np.float32)
    bits, ref_in = bf16_case(np.concatenate([q, k, v], axis=1), hd, heads, q_scaled)
    got = B.from_bf16_bits(B.attention_bf16io_hd(bits, n, T, heads, hd, q_scaled=q_scaled)).reshape(T, D)
    ref = oracle_attention(oracle, ref_in, n, T, heads)[0]
    s0 = (ref_in[:, :hd] @ ref_in[:, D:D + hd].T) * B.qscale(hd)
    assert float((s0[:, -1] - s0[:, 63]).min()) > 24.0  # the exponent really rises by far more than 2^8 along the sequence
    print(f"rising scores q_scaled {q_scaled}: max |d| {float(np.abs(got - ref).max()):.3e}")
    assert (np.abs(got - ref) <= 2.0 ** -8 * np.abs(ref) + 4e-3).all(), float(np.abs(got - ref).max())


# ---- 5: the padded tail of the contraction is really zero, and a head reads its own columns only -----------------------------------

@pytest.mark.parametrize("kind", ["f32", "bf16", "qscaled"])
@pytest.mark.parametrize("hd", [72, 104])
def test_a_head_reads_its_own_columns_only(hd, kind):
    """Head 1 of 3: whatever the neighbouring heads' columns hold (1e30: an Inf or a NaN as soon as it is multiplied into a score or
    an output; or 0), head 1's output has the same bits, and they are the bits of a single-head launch on head 1's columns."""
    heads, n, T = 3, 2, 70
    D = heads * hd
    vals = u(50, (n * T, 3 * D), 1.5)
    own = np.zeros(3 * D, bool)
    for j in range(3):
        own[j * D + hd:j * D + 2 * hd] = True
    outs = []
    for fill in (1e30, 0.0):
        x = vals.copy()
        x[:, ~own] = fill
        qkv = x if kind == "f32" else B.to_bf16_bits(x)
        outs.append(run(kind, qkv, n, T, heads, hd).reshape(n * T, D)[:, hd:2 * hd])
    packed = np.ascontiguousarray(vals[:, own])
    alone = run(kind, packed if kind == "f32" else B.to_bf16_bits(packed), n, T, 1, hd)
    assert not S.has_nan(outs[0]) and same_bits(outs[0], outs[1])
    assert same_bits(outs[0], alone)


# ---- 6: q_rows ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["f32", "bf16", "qscaled"])
@pytest.mark.parametrize("T", [33, 257])
def test_only_the_first_q_rows_are_written(T, kind):
    heads, n, hd = 2, 2, 80
    D = heads * hd
    vals = u(60, (n * T, 3 * D), 1.5)
    qkv = vals if kind == "f32" else B.to_bf16_bits(vals)
    full = run(kind, qkv, n, T, heads, hd).reshape(n, T, D)
    for q_rows in (1, 7, T):
        out = {}
        got = run(kind, qkv, n, T, heads, hd, q_rows=q_rows, frames=S, out=out).reshape(n, T, D)
        out["out"].assert_untouched()
        assert same_bits(got[:, :q_rows], full[:, :q_rows]), q_rows
        assert not S.has_nan(got[:, :q_rows])
        assert (S.as_bits(got[:, q_rows:]) == S.SENTINEL[got.dtype]).all(), f"q_rows {q_rows}: rows behind it were written"


# ---- 7, 8: position independence, isolation ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["f32", "bf16", "qscaled"])
@pytest.mark.parametrize("hd", [80, 128])
def test_an_image_has_the_same_bits_wherever_it_sits(hd, kind):
    heads, T = 2, 70
    D = heads * hd
    img = u(70, (T, 3 * D), 1.5)
    others = u(71, (5 * T, 3 * D), 1.5)
    batch = others.copy()
    for place in (0, 2, 4):
        batch[place * T:(place + 1) * T] = img
    cast = (lambda x: x) if kind == "f32" else B.to_bf16_bits
    alone = run(kind, cast(img), 1, T, heads, hd)
    got = run(kind, cast(batch), 5, T, heads, hd).reshape(5, T, D)
    for place in (0, 2, 4):
        assert same_bits(got[place], alone), place
    assert not same_bits(got[1], alone)


@pytest.mark.parametrize("kind", ["f32", "bf16", "qscaled"])
def test_non_finite_values_stay_in_their_image(kind):
    heads, T, n, hd = 2, 70, 4, 80
    D = heads * hd
    vals = u(80, (n * T, 3 * D), 1.5)
    cast = (lambda x: x) if kind == "f32" else B.to_bf16_bits
    clean = run(kind, cast(vals), n, T, heads, hd).reshape(n, T, D)
    bad = vals.copy()
    bad[1 * T + 3, 5] = np.nan            # a Q element of image 1
    bad[1 * T + 40, D + hd + 7] = np.inf  # a K element of image 1, head 1
    bad[2 * T + 69, 2 * D + 9] = -np.inf  # a V element of image 2's last row
    got = run(kind, cast(bad), n, T, heads, hd).reshape(n, T, D)
    for i in (0, 3):
        assert same_bits(got[i], clean[i]), i
    assert not np.isfinite(B.from_bf16_bits(got[1]) if kind != "f32" else got[1]).all()


# ---- 9: head_dim 64 through the _hd entries is the existing entry -------------------------------------------------------------------

@pytest.mark.parametrize("T", [197, 577])
def test_head_dim_64_is_the_existing_entry(T):
    heads, n = 3, 2
    D = heads * 64
    vals = u(90, (n * T, 3 * D), 1.5)
    bits = B.to_bf16_bits(vals)
    assert same_bits(B.attention_hd(vals, n, T, heads, 64), B.attention(vals, n, T, heads))
    assert same_bits(B.attention_bf16io_hd(bits, n, T, heads, 64), B.attention_bf16io(bits, n, T, heads))
    assert same_bits(B.attention_bf16io_hd(bits, n, T, heads, 64, q_scaled=True), B.attention_bf16io(bits, n, T, heads, q_scaled=True))
    if T <= 224:
        assert same_bits(B.attention_hd(vals, n, T, heads, 64, q_rows=1, fill=7.0), B.attention_rows(vals, n, T, heads, 1, fill=7.0))
        want = B.attention_bf16io_rows(bits, n, T, heads, 1)
        assert same_bits(B.attention_bf16io_hd(bits, n, T, heads, 64, q_rows=1), want)
        want = B.attention_bf16io_rows(bits, n, T, heads, 1, q_scaled=True)
        assert same_bits(B.attention_bf16io_hd(bits, n, T, heads, 64, q_rows=1, q_scaled=True), want)
    else:  # the limit of the _rows entries is the limit of head_dim 64 here as well
        with pytest.raises(B.VitError) as e:
            B.attention_hd(vals, n, T, heads, 64, q_rows=1)
        assert e.value.code == INVALID


# ---- 10: refusals ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["f32", "bf16"])
def test_refusals_leave_the_output_alone(kind):
    n, T, heads = 1, 5, 2
    dtype = np.float32 if kind == "f32" else np.uint16

    def refused(call, out):
        with pytest.raises(B.VitError) as e:
            call()
        assert e.value.code == INVALID, e.value
        f = out["out"]
        arr = f.download()
        f.assert_untouched(arr)
        assert (S.as_bits(f.window(arr)) == S.SENTINEL[f.dtype]).all(), "a refused call wrote its output"

    for hd in (32, 56, 68, 136):
        out = {}
        qkv = np.zeros((n * T, 3 * heads * hd), dtype)
        refused(lambda: run(kind, qkv, n, T, heads, hd, frames=S, out=out), out)
    hd = 80
    qkv = np.zeros((n * T, 3 * heads * hd), dtype)
    for q_rows in (0, -1, T + 1):
        out = {}
        refused(lambda: run(kind, qkv, n, T, heads, hd, q_rows=q_rows, frames=S, out=out), out)
    # NULL pointers, through the entry itself
    fn = B.lib().vithip_attention_f32_hd if kind == "f32" else B.lib().vithip_attention_bf16io_hd
    extra = () if kind == "f32" else (0,)
    dq, do = S.framed(qkv), S.out_frame(n * T, heads * hd, dtype=dtype)
    assert fn(None, None, do.ptr, n, T, heads, hd, T, *extra) == INVALID
    assert fn(None, dq.ptr, None, n, T, heads, hd, T, *extra) == INVALID
    assert fn(None, dq.ptr, do.ptr, 0, T, heads, hd, T, *extra) == INVALID
    assert fn(None, dq.ptr, do.ptr, n, T, heads, 0, T, *extra) == INVALID  # head_dim 0: no frame of that width exists, the entry itself
    if kind == "bf16":
        assert fn(None, dq.ptr, do.ptr, n, T, heads, hd, T, 2) == INVALID
    arr = do.download()
    do.assert_untouched(arr)
    assert (S.as_bits(do.window(arr)) == S.SENTINEL[do.dtype]).all()
    assert fn(None, dq.ptr, do.ptr, n, T, heads, hd, T, *extra) == 0  # and the same frames are fine otherwise
    B.hip_check(B.lib().vithip_device_sync(), "sync")
    do.check()


# ---- 11: the class-token kernels ---------------------------------------------------------------------------------------------------

CAP = {"f32": 1e-4, "bf16": 2e-2}  # the project's probability bars: caps, never loosened
CLS_HEAD_DIMS = [72, 80, 104, 128]
CLS_TOKENS = [1, 2, 17, 65, 197, 257, 577]


def cls_run(dtype, vals, n, T, heads, hd, **kw):
    """(probabilities, the float64 restatement on the values the kernel read)."""
    if dtype == "f32":
        return B.cls_attention_hd(vals, n, T, heads, hd, **kw), cls_attention_ref(vals, n, T, heads, hd)
    bits = B.to_bf16_bits(vals)
    return B.cls_attention_bf16_hd(bits, n, T, heads, hd, **kw), cls_attention_ref(B.from_bf16_bits(bits), n, T, heads, hd)


def cls_run_64(dtype, vals, n, T, heads):
    if dtype == "f32":
        return B.cls_attention(vals, n, T, heads), cls_attention_ref(vals, n, T, heads, 64)
    bits = B.to_bf16_bits(vals)
    return B.cls_attention_bf16(bits, n, T, heads), cls_attention_ref(B.from_bf16_bits(bits), n, T, heads, 64)


def rows_sum_to_one(p, T):
    assert np.isfinite(p).all()
    off = float(np.abs(p.astype(np.float64).sum(-1) - 1.0).max())
    assert off <= T * 2.0 ** -23, (T, off)


@pytest.fixture(scope="module")
def cls_worst():
    return {}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("hd", CLS_HEAD_DIMS)
def test_cls_kernel_matches_the_restatement(hd, dtype, cls_worst):
    """Against float64 under the cap, and against the existing 64 kernel's own error on inputs drawn the same way at the same T and
    heads: at most 2 * (head_dim / 64) times it (head_dim / 64: the longer dot product; 2: draw-to-draw spread)."""
    n = 2
    worst, worst64 = 0.0, 0.0
    for T in CLS_TOKENS:
        for heads in (1, 3):
            vals = u(100 + T + heads, (n * T, 3 * heads * hd), 1.5)
            got, ref = cls_run(dtype, vals, n, T, heads, hd)
            assert got.shape == (n, heads, T)
            rows_sum_to_one(got, T)
            err = float(np.abs(got - ref).max())
            assert err <= CAP[dtype], (hd, T, heads, err)
            worst = max(worst, err)
            mean = (B.cls_attention_hd if dtype == "f32" else B.cls_attention_bf16_hd)(
                vals if dtype == "f32" else B.to_bf16_bits(vals), n, T, heads, hd, head_mean=True)
            want = got[:, 0].copy()
            for h in range(1, heads):
                want = want + got[:, h]
            assert same_bits(mean, want / np.float32(heads)), (hd, T, heads)
            vals64 = u(100 + T + heads, (n * T, 3 * heads * 64), 1.5)
            got64, ref64 = cls_run_64(dtype, vals64, n, T, heads)
            worst64 = max(worst64, float(np.abs(got64 - ref64).max()))
    cls_worst[(dtype, hd)] = (worst, worst64)
    print(f"cls attention {dtype} head_dim {hd}: worst error {worst:.3e}; the 64 kernel on inputs drawn the same way: {worst64:.3e}")
    assert worst <= 2 * (hd / 64) * worst64, (worst, worst64)


@pytest.mark.parametrize("hd", [72, 128])
def test_cls_kernel_q_scaled_reads_prescaled_queries(hd):
    n, T, heads = 2, 65, 3
    D = heads * hd
    vals = u(120, (n * T, 3 * D), 1.5)
    bits, ref_in = bf16_case(vals, hd, heads, True)
    ref = cls_attention_ref(ref_in, n, T, heads, hd)
    got = B.cls_attention_bf16_hd(bits, n, T, heads, hd, q_scaled=True)
    rows_sum_to_one(got, T)
    assert float(np.abs(got - ref).max()) <= CAP["bf16"]
    plain = B.cls_attention_bf16_hd(bits, n, T, heads, hd, q_scaled=False)  # the flag matters: the same bits read as plain q
    assert float(np.abs(plain - ref).max()) > CAP["bf16"]


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_cls_kernel_isolation_and_footprint(dtype):
    n, T, heads, hd = 4, 70, 3, 104
    D = heads * hd
    vals = u(130, (n * T, 3 * D), 1.5)
    cast = (lambda x: x) if dtype == "f32" else B.to_bf16_bits
    fn = B.cls_attention_hd if dtype == "f32" else B.cls_attention_bf16_hd
    clean = fn(cast(vals), n, T, heads, hd)
    bad = vals.copy()
    bad[1 * T, 3] = np.nan                 # the class row's Q of image 1
    bad[2 * T + 9, D + hd + 4] = np.inf    # a K element of image 2
    got = fn(cast(bad), n, T, heads, hd)
    for i in (0, 3):
        assert same_bits(got[i], clean[i]), i
    assert not np.isfinite(got[1]).all() and not np.isfinite(got[2]).all()
    # the row alone is written: ld_out wider than the row keeps the fill behind it
    for mean in (False, True):
        row = T if mean else heads * T
        raw = fn(cast(vals), n, T, heads, hd, head_mean=mean, ld_out=row + 5, fill=7.0)
        assert (raw[:, row:] == 7.0).all() and np.isfinite(raw[:, :row]).all()
    # refusals: head dims off the set, a row stride below the row
    L = B.lib()
    entry = L.vithip_cls_attention_f32_hd if dtype == "f32" else L.vithip_cls_attention_bf16_hd
    extra = () if dtype == "f32" else (0,)
    dq = B.DeviceArray.from_numpy(cast(vals))
    do = B.DeviceArray.from_numpy(np.full((n, heads * T), 7.0, np.float32))
    for bad_hd in (32, 56, 68, 136, 0):
        assert entry(None, dq.ptr, 3 * D, do.ptr, heads * T, n, T, heads, bad_hd, 0, *extra) == INVALID
    assert entry(None, dq.ptr, 3 * D - 8, do.ptr, heads * T, n, T, heads, hd, 0, *extra) == INVALID
    assert entry(None, None, 3 * D, do.ptr, heads * T, n, T, heads, hd, 0, *extra) == INVALID
    assert (do.numpy() == 7.0).all()


@pytest.mark.parametrize("head_mean", [False, True], ids=["heads", "head-mean"])
@pytest.mark.parametrize("T", [17, 197])
def test_cls_head_dim_64_is_the_existing_entry(T, head_mean):
    """The class-row _hd entries with head_dim 64 give the bits of vithip_cls_attention_f32 / _bf16."""
    heads, n = 3, 2
    vals = u(140 + T, (n * T, 3 * heads * 64), 1.5)
    bits = B.to_bf16_bits(vals)
    assert same_bits(B.cls_attention_hd(vals, n, T, heads, 64, head_mean=head_mean), B.cls_attention(vals, n, T, heads, head_mean=head_mean))
    for q_scaled in (False, True):
        got = B.cls_attention_bf16_hd(bits, n, T, heads, 64, head_mean=head_mean, q_scaled=q_scaled)
        assert same_bits(got, B.cls_attention_bf16(bits, n, T, heads, head_mean=head_mean, q_scaled=q_scaled)), q_scaled
