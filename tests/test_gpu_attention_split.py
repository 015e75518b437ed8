"""vithip_attention_f32_split (csrc/vit_attention_hd.hip: attention_split_kernel): fp32 attention at head_dim 64 with both products
on the bf16 matrix pipe, every operand in three bf16 pieces.  Against the oracle's attention_core with the bars of the fp32 kernels
(tests/test_gpu_ops.py::test_attention, ::test_attention_peaked_rows, ::test_attention_chunked_running_max_moves), and the guarantees
the other P.V entries give: bits that depend on neither the batch nor q_rows, isolation of a non-finite image, refusals that launch
nothing.  Then the engine, which takes this entry whenever fp32_split is on and head_dim is 64.

The kernel works on tiles of 32 keys, skips a group of 16 keys behind the last token, streams K and V in chunks of 64 keys and gives
a workgroup 128 query rows: the token counts sit either side of 16, 32, 48, 64, 128 and at the workload's 197, 224 and beyond.
"""
import numpy as np
import pytest

import strided as S
from engine_helpers import engines, same_bits, weights  # noqa: F401  (fixtures)
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

INVALID = 1  # hipErrorInvalidValue
SHAPES = [(1, 1, 1), (3, 5, 2), (1, 32, 1), (1, 33, 1), (1, 64, 1), (2, 65, 2), (2, 129, 2), (1, 197, 3), (1, 224, 2), (1, 257, 1),
          (1, 300, 1)]
EDGES = [(1, 16, 1), (1, 17, 1), (1, 48, 1), (1, 49, 1), (1, 128, 1)]  # the 16-key group, the 128-row workgroup


def u(k, shape, a, seed=777):  # the inputs of tests/test_gpu_ops.py
    n = int(np.prod(shape))
    return synth.uniform(seed, k, n, -a, a).reshape(shape)


def oracle_attention(oracle, qkv, n, T, heads):
    D = qkv.shape[1] // 3
    out = []
    for i in range(n):
        blk = qkv[i * T:(i + 1) * T]
        q, k, v = (np.ascontiguousarray(blk[:, j * D:(j + 1) * D], np.float32) for j in range(3))
        out.append(oracle.attention_core(q, k, v, heads))
    return np.stack(out)


@pytest.mark.parametrize("n,T,heads", SHAPES + EDGES)
def test_matches_the_oracle(oracle, n, T, heads):
    """The reference's order of operations; the accuracy test, against float64 at fp32-level bars: tests/test_gpu_attention_accuracy.py."""
    D = heads * 64
    qkv = u(30, (n * T, 3 * D), 1.5)
    got = B.attention_split(qkv, n, T, heads).reshape(n, T, D)
    ref = oracle_attention(oracle, qkv, n, T, heads)
    for i in range(n):
        err, bar = float(np.abs(got[i] - ref[i]).max()), 1e-5 * max(1.0, float(np.abs(ref[i]).max()))
        print(f"split attention n {n} T {T} heads {heads} image {i}: {err:.3e} (bar {bar:.3e})")
        assert err <= bar, (n, T, heads, i, err)


def test_peaked_rows(oracle):
    n, T, heads = 1, 197, 2
    qkv = u(31, (T, 3 * heads * 64), 8.0)
    got = B.attention_split(qkv, n, T, heads)
    ref = oracle_attention(oracle, qkv, n, T, heads)[0]
    assert np.isfinite(got).all()
    err = float(np.abs(got - ref).max())
    print(f"split attention, peaked rows: {err:.3e} (bar {2e-4 * float(np.abs(ref).max()):.3e})")
    assert err <= 2e-4 * float(np.abs(ref).max())


def test_running_maximum_moves(oracle):
    """Keys 100.. six times larger: the rows' maximum moves in the fourth and fifth tile, the rescale branch runs."""
    T = 130
    qkv = u(33, (T, 192), 1.0)
    qkv[100:, 64:128] *= 6.0
    got = B.attention_split(qkv, 1, T, 1)
    ref = oracle_attention(oracle, qkv, 1, T, 1)[0]
    err = float(np.abs(got - ref).max())
    print(f"split attention, running maximum: {err:.3e} (bar {2e-5 * float(np.abs(ref).max()):.3e})")
    assert err <= 2e-5 * float(np.abs(ref).max())


@pytest.fixture(scope="module")
def batch26():
    heads, n, T = 12, 26, 197
    qkv = u(70, (n * T, 3 * heads * 64), 1.5)
    return qkv, B.attention_split(qkv, n, T, heads).reshape(n, T, heads * 64)


def test_an_image_alone_has_its_bits_in_the_batch(batch26):
    qkv, big = batch26
    T, heads = 197, 12
    for i in (0, 7, 25):
        one = B.attention_split(qkv[i * T:(i + 1) * T].copy(), 1, T, heads)
        assert np.array_equal(S.as_bits(one).view(np.uint32), S.as_bits(big[i]).view(np.uint32)), i
    assert not np.array_equal(big[0], big[1])


@pytest.mark.parametrize("q_rows", [1, 40])
def test_q_rows_writes_those_rows_with_the_full_calls_bits(batch26, q_rows):
    qkv, big = batch26
    T, heads, n = 197, 12, 2
    out = {}
    got = B.attention_split(qkv[:n * T], n, T, heads, q_rows=q_rows, frames=S, out=out).reshape(n, T, heads * 64)
    out["out"].assert_untouched()
    assert same_bits(got[:, :q_rows], big[:n, :q_rows])
    assert (S.as_bits(got[:, q_rows:]) == S.SENTINEL[got.dtype]).all(), "rows behind q_rows were written"


def test_an_image_of_nans_stays_in_its_image(batch26):
    qkv, big = batch26
    T, heads, n = 197, 12, 4
    bad = qkv[:n * T].copy()
    bad[2 * T:3 * T] = np.nan
    got = B.attention_split(bad, n, T, heads).reshape(n, T, heads * 64)
    assert np.isnan(got[2]).all()
    for i in (0, 1, 3):
        assert same_bits(got[i], big[i]), i


def test_refusals_launch_nothing():
    n, T, heads = 1, 5, 2
    fn = B.lib().vithip_attention_f32_split
    dq = S.framed(np.zeros((n * T, 3 * heads * 64), np.float32))
    do = S.out_frame(n * T, heads * 64)
    wide_q = S.framed(np.zeros((n * T, 3 * heads * 128), np.float32))     # frames large enough for the head dims it refuses
    wide_o = S.out_frame(n * T, heads * 128)
    assert fn(None, wide_q.ptr, wide_o.ptr, n, T, heads, 72, T) == INVALID   # head_dim 72: vithip_attention_f32_hd has it
    assert fn(None, wide_q.ptr, wide_o.ptr, n, T, heads, 128, T) == INVALID
    B.hip_check(B.lib().vithip_device_sync(), "sync")
    arr = wide_o.download()
    wide_o.assert_untouched(arr)
    assert (S.as_bits(wide_o.window(arr)) == S.SENTINEL[wide_o.dtype]).all(), "a refused call wrote its output"
    assert fn(None, dq.ptr, do.ptr, n, 0, heads, 64, 0) == INVALID        # tokens 0
    assert fn(None, dq.ptr, do.ptr, n, T, heads, 64, 0) == INVALID        # q_rows 0
    assert fn(None, dq.ptr, do.ptr, n, T, heads, 64, T + 1) == INVALID    # q_rows > tokens
    assert fn(None, dq.ptr + 4, do.ptr, n, T, heads, 64, T) == INVALID    # misaligned qkv
    assert fn(None, dq.ptr, do.ptr + 8, n, T, heads, 64, T) == INVALID    # misaligned out
    assert fn(None, None, do.ptr, n, T, heads, 64, T) == INVALID
    B.hip_check(B.lib().vithip_device_sync(), "sync")
    arr = do.download()
    do.assert_untouched(arr)
    assert (S.as_bits(do.window(arr)) == S.SENTINEL[do.dtype]).all(), "a refused call wrote its output"
    assert fn(None, dq.ptr, do.ptr, n, T, heads, 64, T) == 0              # the same frames are fine otherwise
    B.hip_check(B.lib().vithip_device_sync(), "sync")
    do.check()


def test_engine_default_agrees_with_the_fp32_matrix_engine(engines):
    """VIT_TINY (2 layers, 2 heads of 64), batch 3.  The default engine runs its GEMMs and now its attention on the split; with
    fp32_split = -1 everything is on the fp32 matrix instruction.  tests/test_gpu_split_gemm.py holds the two to 5e-6 and 1e-4 of
    one golden: the wider of the two between them, and the same top-1."""
    imgs = synth.make_images(synth.VIT_TINY, 3, 7)
    split = engines("tiny", max_batch=3).forward(imgs)
    fp32 = engines("tiny", max_batch=3, fp32_split=-1).forward(imgs)
    err = float(np.abs(split - fp32).max())
    print(f"engine, split against fp32 MFMA: max |dprob| = {err:.3e}")
    assert err <= 1e-4
    assert (split.argmax(1) == fp32.argmax(1)).all()
    assert not np.array_equal(split, fp32)


def test_engine_prune_last_layer_changes_no_bit(engines):
    imgs = synth.make_images(synth.VIT_TINY, 3, 7)
    plain = engines("tiny", max_batch=3).forward(imgs)
    pruned = engines("tiny", max_batch=3, prune_last_layer=True).forward(imgs)
    assert same_bits(plain, pruned)
