"""vithip_rope_f32 / vithip_rope_bf16 (csrc/vit_rope.hip) against float64 on the exact input values: 5 images (an image slice has a
tail), 3 heads, a 3 x 3 grid behind a prefix of 5 rows (and of 1), ld = 3D + 8, qkv uniform in [-4, 4]; tables uniform in [-1, 1], not
true cos / sin, so that a swapped table, sign or half shows.  Bars, derived and not measured, with x1, x2, c, s of the element's pair:
  fp32: |got - ref| <= 2^-23 (|x1 c| + |x2 s|): one rounding of the product and one of the fma, 2^-24 relative each;
  bf16: the same plus 2^-8 |ref|: one nearest-even rounding to 8 significant bits, a factor 2 for results next to a binade edge.
Every element that must not change (prefix rows, V, pad columns, guard rows, Q under "k") is compared bitwise."""
import numpy as np
import pytest

import strided
from vit_amd import binding as B

pytestmark = pytest.mark.gpu
N, HEADS, P = 5, 3, 9


def model64(qkv, cos, sin, hd, prefix, which):
    """(ref, bar, rotated): the float64 rotation, the fp32 bar per element, the mask of the elements the launch may write."""
    half = hd // 2
    v = qkv.astype(np.float64).reshape(N, prefix + P, 3, HEADS, hd)
    ref, bar, rotated = v.copy(), np.zeros_like(v), np.zeros(v.shape, bool)
    c, s = cos.astype(np.float64)[None, :, None, :], sin.astype(np.float64)[None, :, None, :]   # [1][P][1][half]
    for seg in ((0, 1) if which == "qk" else (1,)):
        x1, x2 = v[:, prefix:, seg, :, :half], v[:, prefix:, seg, :, half:]
        ref[:, prefix:, seg, :, :half], ref[:, prefix:, seg, :, half:] = x1 * c - x2 * s, x2 * c + x1 * s
        bar[:, prefix:, seg, :, :half] = 2.0 ** -23 * (np.abs(x1 * c) + np.abs(x2 * s))
        bar[:, prefix:, seg, :, half:] = 2.0 ** -23 * (np.abs(x2 * c) + np.abs(x1 * s))
        rotated[:, prefix:, seg] = True
    return (a.reshape(qkv.shape) for a in (ref, bar, rotated))


@pytest.mark.parametrize("prefix", [5, 1])
@pytest.mark.parametrize("which", ["qk", "k"])
@pytest.mark.parametrize("hd", [64, 80, 128])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_rotation_is_within_the_bar_of_float64_and_writes_the_rotated_elements_only(bf16, hd, which, prefix):
    rng = np.random.default_rng(1000 * hd + 10 * prefix + bf16)
    D, T = HEADS * hd, prefix + P
    qkv = rng.uniform(-4, 4, (N * T, 3 * D)).astype(np.float32)
    cos, sin = (rng.uniform(-1, 1, (P, hd // 2)).astype(np.float32) for _ in range(2))
    data = B.to_bf16_bits(qkv).reshape(qkv.shape) if bf16 else qkv
    qkv = B.from_bf16_bits(data).reshape(qkv.shape) if bf16 else qkv   # the values the kernel sees
    sink = {}
    got_bits = B.rope(data, cos, sin, N, T, prefix, HEADS, hd, which, ld=3 * D + 8, frames=strided, out=sink)
    sink["qkv"].assert_untouched()   # the pad columns and the guard rows
    got = B.from_bf16_bits(got_bits).reshape(qkv.shape) if bf16 else got_bits
    ref, bar, rotated = model64(qkv, cos, sin, hd, prefix, which)
    if bf16:
        bar = bar + 2.0 ** -8 * np.abs(ref)
    assert np.array_equal(strided.as_bits(got_bits)[~rotated], strided.as_bits(data)[~rotated]), "an element outside the rotation changed"
    err = np.abs(got.astype(np.float64) - ref)
    print(f"{'bf16' if bf16 else 'f32'} hd={hd} {which} prefix={prefix}: worst error {float((err[rotated] / bar[rotated]).max()):.3f} of the bar")
    assert not (err > bar).any(), (int((err > bar).sum()), np.argwhere(err > bar)[0])
    again = B.rope(data, cos, sin, N, T, prefix, HEADS, hd, which, ld=3 * D + 8, frames=strided)
    assert np.array_equal(strided.as_bits(again), strided.as_bits(got_bits)), "two launches differ"


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_refused_arguments_return_invalid_value_and_leave_the_buffer_untouched(bf16):
    hd, prefix = 64, 5
    D, T, dt = HEADS * hd, prefix + P, np.dtype(np.uint16 if bf16 else np.float32)
    Q = strided.out_frame(N * T, 3 * D, 3 * D + 8, dt)
    Cs, Sn = (strided.framed(np.zeros((P, hd // 2), np.float32)) for _ in range(2))
    ok = [Q.ptr, Q.ld, Cs.ptr, Sn.ptr, N, T, prefix, HEADS, hd, 0]   # rope_raw's arguments; below, per position, the values it refuses
    refused = {0: [None, Q.ptr + dt.itemsize], 1: [3 * D - 4, 3 * D + 2], 2: [None, Cs.ptr + 4], 3: [None, Sn.ptr + 8], 4: [0, -1],
               5: [0, prefix], 6: [-1, T], 7: [0], 8: [0, 68, 136], 9: [2, -1]}
    for i, values in refused.items():
        for v in values:
            assert B.rope_raw(*ok[:i], v, *ok[i + 1:], bf16) == 1, (i, v)   # hipErrorInvalidValue
    B.hip_check(B.lib().vithip_device_sync(), "sync")
    assert (Q.download() == strided.SENTINEL[dt]).all(), "a refused call wrote"   # the frame's image is kept as bit patterns
