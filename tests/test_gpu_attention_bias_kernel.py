"""vithip_attention_f32_bias / _bf16io_bias (csrc/vit_attention_bias.hip) against a float64 softmax(q.k / sqrt(hd) + b) . V.  One image,
two heads with biases of their own, U(-4, 4); Q, K, V: the "iid" family of attention_split_model.  Tokens: 33 (one key past a 32-key
tile), 129 (a second 128-row query block, a third 64-key chunk in bf16), 197 with ld_bias = 200; head dims 64 and 72.
  fp32   max |got - ref| <= 4 e_seq + 2^-23 |ref|max, e_seq from a sequential fp32 evaluation (bar (a) of test_gpu_attention_accuracy.py)
  bf16   every output in [rne_bf16(ref - bar), rne_bf16(ref + bar)], bar = 2^-8 A + 4 e_seq + 2^-23 |ref|max, A = sum p |v| / sum p
         (tier II (a) of test_gpu_attention_bf16_accuracy.py); plain and q_scaled
  masked every third key column -inf, the pad columns [T, ld_bias) NaN patterns: the same bars against the sequence without those keys
  one-hot  a single 0 per bias row, -inf elsewhere: the output row is that V row, bit for bit (p is 1 and 0, the row sum 1)
Measured on the MI355X: profiles/r37/attention_bias.md."""
import functools

import numpy as np
import pytest

import attention_bf16_model as A
import attention_split_model as M
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu
HEADS, SEED, LOG2E = 2, 2037, np.float32(1.4426950408889634)
SHAPES = [(33, 36), (129, 132), (197, 200)]   # (tokens, ld_bias)
HEAD_DIMS = [64, 72]


def reference(q, k, v, b, head_dim, q_scaled):
    """(softmax(q.k / sqrt(hd) + b) . v, the same with |v|) in float64; q_scaled: q holds scale_f32(hd) * q, p = 2^(q.k + b log2 e)"""
    q, k, v, b = (np.asarray(a, np.float64) for a in (q, k, v, b))
    x = q @ k.T + b * float(LOG2E) if q_scaled else (q @ k.T / np.sqrt(float(head_dim)) + b) * np.log2(np.e)
    p = np.exp2(x - x.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    return p @ v, p @ np.abs(v)


def sequential_f32(q, k, v, b, head_dim, q_scaled):
    """attention_split_model.attention_f32_sequential with the bias: x = fma(s, c, b log2 e), p = exp2(x - max x), every step rounded to fp32."""
    q, k, v = (np.asarray(a, np.float32) for a in (q, k, v))
    c = np.float64(1.0 if q_scaled else M.scale_f32(head_dim))
    s = np.zeros((q.shape[0], k.shape[0]), np.float32)
    for d in range(head_dim):
        s = M.f32(s.astype(np.float64) + np.outer(q[:, d].astype(np.float64), k[:, d].astype(np.float64)))
    x = M.f32(s.astype(np.float64) * c + M.f32(b.astype(np.float64) * np.float64(LOG2E)).astype(np.float64))
    p = M.f32(np.exp2((x - x.max(1, keepdims=True)).astype(np.float64)))
    total, o = np.zeros(q.shape[0], np.float32), np.zeros((q.shape[0], v.shape[1]), np.float32)
    for key in range(k.shape[0]):
        total = total + p[:, key]
        o = M.f32(o.astype(np.float64) + np.outer(p[:, key].astype(np.float64), v[key].astype(np.float64)))
    return o * (np.float32(1.0) / total)[:, None]


@functools.lru_cache(maxsize=None)
def case(T, ld, head_dim, masked, bf16=False, q_scaled=False):
    """Once: qkv as the entry reads it (bf16: rounded), the bias [heads][T][ld], the float64 reference, A, e_seq (masked: without those keys)"""
    qkv = M.family_inputs("iid", T, head_dim, HEADS, SEED)[0].copy()
    if q_scaled:
        qkv[:, :HEADS * head_dim] *= M.scale_f32(head_dim)
    if bf16:
        qkv = B.from_bf16_bits(B.to_bf16_bits(qkv)).reshape(qkv.shape)
    bias = synth.uniform(SEED, 7, HEADS * T * ld, -4.0, 4.0).reshape(HEADS, T, ld)
    keep = np.ones(T, bool)
    if masked:
        keep[1::3] = False
        bias[:, :, :T][:, :, ~keep] = -np.inf
        bias[:, :, T:] = np.array([0x7FC00001, 0xFFFFFFFF, 0x7F800001], np.uint32).view(np.float32)[:ld - T]
    ref, Aa, seq = [], [], []
    for h in range(HEADS):
        q, k, v = M.head_operands(qkv, HEADS, head_dim, h)
        b = bias[h][:, :T][:, keep]
        r, a = reference(q, k[keep], v[keep], b, head_dim, q_scaled)
        ref.append(r), Aa.append(a), seq.append(sequential_f32(q, k[keep], v[keep], b, head_dim, q_scaled))
    ref, Aa = np.concatenate(ref, 1), np.concatenate(Aa, 1)
    return dict(qkv=qkv, bias=bias, ref=ref, A=Aa, top=float(np.abs(ref).max()), e_seq=float(np.abs(np.concatenate(seq, 1) - ref).max()))


@pytest.mark.parametrize("masked", [False, True], ids=["dense", "masked"])
@pytest.mark.parametrize("head_dim", HEAD_DIMS)
@pytest.mark.parametrize("T,ld", SHAPES)
def test_fp32_against_float64(T, ld, head_dim, masked):
    c = case(T, ld, head_dim, masked)
    got = B.attention_bias(c["qkv"], c["bias"], 1, T, HEADS, head_dim)
    e, bar = float(np.abs(got - c["ref"]).max()), 4 * c["e_seq"] + 2.0 ** -23 * c["top"]
    print(f"fp32 T {T} hd {head_dim} masked {masked}: e_kernel {e:.3e}  e_seq {c['e_seq']:.3e}  bar {bar:.3e}  |ref|max {c['top']:.3g}")
    assert np.isfinite(got).all() and e <= bar, (e, bar)


@pytest.mark.parametrize("masked", [False, True], ids=["dense", "masked"])
@pytest.mark.parametrize("q_scaled", [False, True], ids=["plain", "qscaled"])
@pytest.mark.parametrize("head_dim", HEAD_DIMS)
@pytest.mark.parametrize("T,ld", SHAPES)
def test_bf16_against_float64(T, ld, head_dim, q_scaled, masked):
    c = case(T, ld, head_dim, masked, True, q_scaled)
    got = B.attention_bf16io_bias(B.to_bf16_bits(c["qkv"]).reshape(c["qkv"].shape), c["bias"], 1, T, HEADS, head_dim, q_scaled=q_scaled)
    bar = 2.0 ** -8 * c["A"] + 4 * c["e_seq"] + 2.0 ** -23 * c["top"]
    outside = int(A.outside_bracket(got, c["ref"], bar).sum())
    print(f"bf16 T {T} hd {head_dim} q_scaled {q_scaled} masked {masked}: {outside} outside, max e / bar {float((np.abs(A.values(got) - c['ref']) / bar).max()):.2f}")
    assert outside == 0


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("head_dim", HEAD_DIMS)
@pytest.mark.parametrize("T,ld", SHAPES)
def test_a_one_hot_bias_selects_the_value_row_bit_for_bit(T, ld, head_dim, dtype):
    D = HEADS * head_dim
    qkv = case(T, ld, head_dim, False, dtype == "bf16")["qkv"]
    pick = (7 * np.arange(T)[None, :] + 3 * np.arange(HEADS)[:, None] + 1) % T
    bias = np.full((HEADS, T, ld), -np.inf, np.float32)
    for h in range(HEADS):
        bias[h, np.arange(T), pick[h]] = 0.0
    if dtype == "bf16":
        bits = B.to_bf16_bits(qkv).reshape(qkv.shape)
        got, v = B.attention_bf16io_bias(bits, bias, 1, T, HEADS, head_dim), bits[:, 2 * D:]
    else:
        got, v = B.attention_bias(qkv, bias, 1, T, HEADS, head_dim).view(np.uint32), qkv[:, 2 * D:].view(np.uint32)
    for h in range(HEADS):
        cols = slice(h * head_dim, (h + 1) * head_dim)
        assert np.array_equal(got[:, cols], v[pick[h]][:, cols]), (h, np.argwhere(got[:, cols] != v[pick[h]][:, cols])[0])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_single_rows_batch_position_and_refused_arguments(dtype):
    T, ld, hd = 129, 132, 72
    c = case(T, ld, hd, False, dtype == "bf16")
    other = case(T, ld, hd, False, dtype == "bf16", True)["qkv"]   # another image: this one with scaled Q columns
    if dtype == "bf16":
        run, conv, fill = B.attention_bf16io_bias, lambda a: B.to_bf16_bits(a).reshape(a.shape), 0x1234
    else:
        run, conv, fill = B.attention_bias, lambda a: a, 7.0
    full = run(conv(c["qkv"]), c["bias"], 1, T, HEADS, hd)
    row = run(conv(c["qkv"]), c["bias"], 1, T, HEADS, hd, q_rows=1, fill=fill)
    assert np.array_equal(row[0].view(np.uint8), full[0].view(np.uint8)) and (row[1:] == fill).all()
    three = run(conv(np.concatenate([c["qkv"], other, c["qkv"]])), c["bias"], 3, T, HEADS, hd)
    assert all(np.array_equal(three[i * T:(i + 1) * T].view(np.uint8), full.view(np.uint8)) for i in (0, 2))
    zeros68 = np.zeros((T, 3 * HEADS * 68), c["qkv"].dtype)
    for qkv, head_dim, kw in [(c["qkv"], hd, dict(null_bias=True)), (c["qkv"], hd, dict(ld_bias=T - 1)), (c["qkv"], hd, dict(ld_bias=ld - 2)), (zeros68, 68, {})]:
        frames = {}
        with pytest.raises(B.VitError) as err:
            run(conv(qkv), c["bias"], 1, T, HEADS, head_dim, fill=fill, out=frames, **kw)
        assert err.value.code == 1 and (frames["out"].window() == fill).all(), kw   # hipErrorInvalidValue, nothing launched
