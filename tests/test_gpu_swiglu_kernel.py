"""vithip_swiglu_f32 / vithip_swiglu_bf16 (csrc/vit_swiglu.hip) against the float64 model of tests/swiglu_model.py.

Shapes: rows in {1, 3, 67}; H in {4, 36, 256} (fp32) / {8, 72, 256} (bf16): the single-vector row, a width that is no multiple of a
workgroup's column coverage, a full one.  Layouts: dense, padded leading dimensions (ldu = 2H + 8, ldh = H + 16), in place.
Inputs: gate and value uniform in [-20, 20]; the last row also holds 0, -0, +-1e-30, +-87, +-89, +-104, +-3e38, +-Inf, NaN in both
roles (at H = 256 every (gate, value) pair of them).

fp32 bar, derived and not measured: |got - ref| <= 4 ulp_f32(|ref|) + 2^-126 on every finite reference.  expf is within 1 ulp (OCML's
stated bound) and its error reaches s = 1 + e attenuated by e / (1 + e) <= 1; the add, the divide and the multiply add half an ulp
each: under 2.5 ulp plus second-order terms.  (The form for g < -87, ((g t) v) t with t = expf(g / 2): 2 ulp of t twice over plus
three half-ulp products = 3.5 ulp.)  Measured on an MI355X: see profiles/r18/swiglu.md.
bf16 bar: got == bf16_rne(ref) wherever no bf16 rounding boundary lies within that fp32 bound of ref, else either neighbour.
"""
import numpy as np
import pytest

import strided
import swiglu_model
from vit_amd import binding as B

gpu = pytest.mark.gpu

HIP_INVALID = 1  # hipErrorInvalidValue
SPECIALS = np.array([0.0, -0.0, 1e-30, -1e-30, 87, -87, 89, -89, 104, -104, 3e38, -3e38, np.inf, -np.inf, np.nan], np.float32)
ROWS = [1, 3, 67]
LAYOUTS = ["dense", "padded", "in_place"]
_cases = {}


def inputs(rows, H, bf16):
    """u [rows][2H] = gate | value (float32; bf16: values a bf16 holds exactly), the last row with the special values; and the mask
    [rows][H] of the elements that hold drawn values only."""
    key = (rows, H, bf16)
    if key not in _cases:
        rng = np.random.default_rng(1000 * rows + H + (7 if bf16 else 0))
        u = rng.uniform(-20, 20, (rows, 2 * H)).astype(np.float32)
        drawn = np.ones((rows, H), bool)
        g, v = u[-1, :H], u[-1, H:]
        S = len(SPECIALS)
        if H >= S * S:      # every pair
            j = np.arange(S * S)
            g[j], v[j] = SPECIALS[j % S], SPECIALS[j // S]
            drawn[-1, :S * S] = False
        else:               # even columns: a special gate and a drawn value; odd columns: the other way round
            j = np.arange(H)
            g[0::2] = SPECIALS[(j[0::2] // 2) % S]
            v[1::2] = SPECIALS[(j[1::2] // 2 + H // 4) % S]
            drawn[-1] = False
        if bf16:
            u = B.from_bf16_bits(B.to_bf16_bits(u)).reshape(rows, 2 * H)
        _cases[key] = (u, drawn)
    return _cases[key]


def model64(u, H):
    """The float64 model (before its one rounding) and its fp32 rounding."""
    g, v = u[:, :H].astype(np.float64), u[:, H:].astype(np.float64)
    with np.errstate(all="ignore"):
        ref = (g / (1.0 + np.exp(-g))) * v
        return ref, ref.astype(np.float32)


def f32_bound(ref64, ref32):
    with np.errstate(all="ignore"):
        return 4.0 * np.spacing(np.abs(ref32)).astype(np.float64) + 2.0 ** -126


def run(u, H, layout, bf16, sink):
    data = B.to_bf16_bits(u).reshape(u.shape) if bf16 else u
    if bf16:   # to_bf16_bits is exact here except for the NaN's bit pattern
        data[np.isnan(u)] = 0x7FC0
    pad = layout == "padded"
    got = B.swiglu(data, H, in_place=layout == "in_place", ldu=2 * H + 8 if pad else None, ldh=H + 16 if pad else None, frames=strided,
                   out=sink)
    sink["h"].assert_untouched()
    return data, got


def check_f32(got, u, H, tag):
    ref64, ref32 = model64(u, H)
    finite = np.isfinite(ref32)
    assert np.array_equal(np.isfinite(got), finite), f"{tag}: non-finite outputs are not where the model has them"
    assert np.array_equal(np.isnan(got), np.isnan(ref32)), f"{tag}: NaNs are not where the model has them"
    assert np.array_equal(got[~finite & ~np.isnan(ref32)], ref32[~finite & ~np.isnan(ref32)]), f"{tag}: an infinity of the wrong sign"
    with np.errstate(all="ignore"):
        err = np.abs(got.astype(np.float64) - ref64)
        bound = f32_bound(ref64, ref32)
        ulps = np.where(finite, err / np.spacing(np.abs(ref32)).astype(np.float64), 0.0)
    normal = finite & (np.abs(ref32) >= 2.0 ** -126)
    worst = float(ulps[normal].max()) if normal.any() else 0.0
    print(f"{tag}: max error {worst:.3f} ulp over {int(normal.sum())} normal references, "
          f"max |d| {float(err[finite & ~normal].max()) if (finite & ~normal).any() else 0.0:.3e} over the {int((finite & ~normal).sum())} below 2^-126")
    bad = finite & (err > bound)
    assert not bad.any(), (tag, int(bad.sum()), np.argwhere(bad)[0], got[bad][0], ref64[bad][0])
    return worst


def bf16_window(u, H):
    """Per element the lowest and the highest bf16 value (as float32) the bar accepts, and the model's fp32 rounding."""
    ref64, ref32 = model64(u, H)
    with np.errstate(all="ignore"):
        tol = f32_bound(ref64, ref32)
        tol = np.where(np.abs(ref32) >= 2.0 ** -120, tol - 2.0 ** -126, tol)   # the absolute term is for results below the normal range
        lo = B.from_bf16_bits(B.to_bf16_bits((ref64 - tol).astype(np.float32))).reshape(ref32.shape)
        hi = B.from_bf16_bits(B.to_bf16_bits((ref64 + tol).astype(np.float32))).reshape(ref32.shape)
    return lo, hi, ref32


def check_bf16(got_bits, u, H, tag):
    got = B.from_bf16_bits(got_bits).reshape(got_bits.shape)
    lo, hi, ref32 = bf16_window(u, H)
    finite = np.isfinite(ref32) & np.isfinite(lo) & np.isfinite(hi)   # a reference within the bound of the largest bf16 may round either way
    sure = np.isfinite(ref32) == (np.isfinite(lo) & np.isfinite(hi))
    assert np.array_equal(np.isfinite(got)[sure], np.isfinite(ref32)[sure]), f"{tag}: non-finite outputs are not where the model has them"
    assert np.array_equal(np.isnan(got), np.isnan(ref32)), f"{tag}: NaNs are not where the model has them"
    inf = np.isinf(ref32) & sure
    assert np.array_equal(got[inf], ref32[inf]), f"{tag}: an infinity of the wrong sign"
    bad = finite & ~((got >= lo) & (got <= hi))
    assert not bad.any(), (tag, int(bad.sum()), np.argwhere(bad)[0], got[bad][0], ref32[bad][0])
    exact = finite & (lo == hi)
    print(f"{tag}: {int(exact.sum())} of {int(finite.sum())} finite references leave one bf16 value")
    assert np.array_equal(got[exact], lo[exact])


@gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("H", [4, 36, 256])
@pytest.mark.parametrize("rows", ROWS)
def test_fp32_gate_is_within_four_ulp_of_the_model_and_writes_its_window_only(rows, H, layout):
    u, _ = inputs(rows, H, False)
    sink = {}
    _, got = run(u, H, layout, False, sink)
    if layout == "in_place":
        assert got.shape == (rows, 2 * H)
        assert np.array_equal(got[:, H:].view(np.uint32), u[:, H:].view(np.uint32)), "in place: the value half changed"
        got = got[:, :H]
    assert got.shape == (rows, H)
    check_f32(got, u, H, f"fp32 rows={rows} H={H} {layout}")


@gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("H", [8, 72, 256])
@pytest.mark.parametrize("rows", ROWS)
def test_bf16_gate_is_the_rounded_model_and_writes_its_window_only(rows, H, layout):
    u, _ = inputs(rows, H, True)
    sink = {}
    data, got = run(u, H, layout, True, sink)
    if layout == "in_place":
        assert got.shape == (rows, 2 * H)
        assert np.array_equal(got[:, H:], data[:, H:]), "in place: the value half changed"
        got = got[:, :H]
    assert got.shape == (rows, H) and got.dtype == np.uint16
    check_bf16(got, u, H, f"bf16 rows={rows} H={H} {layout}")


def test_few_drawn_elements_sit_near_a_bf16_rounding_boundary():
    """On the CPU: the share of drawn elements for which the bf16 bar accepts two values is about 2 * 4 / 65536, under 0.1 % -- where
    the results are spread evenly over the low bits, which is so for gates below 14.5.  Above, silu(g) is g to within 4 fp32 ulp
    (exp(-14.5) = 5e-7, and nothing at all from 17.4 on) and h is the product of two bf16 values: 16 bits at most, so one result in
    fifty or so IS a rounding boundary, whatever the kernel does.  Those elements (14 % of the draws) are counted apart; over all
    draws the share is 0.27 %.  Every one of them is still held to "either neighbour"."""
    near = total = near_big = total_big = 0
    for rows in ROWS:
        for H in (8, 72, 256):
            u, drawn = inputs(rows, H, True)
            lo, hi, _ = bf16_window(u, H)
            big = u[:, :H] >= 14.5
            near += int((lo != hi)[drawn & ~big].sum())
            total += int((drawn & ~big).sum())
            near_big += int((lo != hi)[drawn & big].sum())
            total_big += int((drawn & big).sum())
    print(f"gates below 14.5: {near} of {total} drawn elements within 4 fp32 ulp of a bf16 rounding boundary ({near / total:.2e}); "
          f"from 14.5 on: {near_big} of {total_big} ({near_big / total_big:.2e}); all: {(near + near_big) / (total + total_big):.2e}")
    assert total > 15000 and near / total < 1e-3
    assert total_big > 1000 and near_big / total_big < 0.05


@gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_two_launches_give_the_same_bits(bf16):
    u, _ = inputs(67, 256, bf16)
    a = run(u, 256, "padded", bf16, {})[1]
    b = run(u, 256, "padded", bf16, {})[1]
    bits = np.uint16 if bf16 else np.uint32
    assert np.array_equal(a.view(bits), b.view(bits))


@gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_a_non_finite_element_reaches_its_own_output_only(bf16):
    rows, H = 67, 72
    rng = np.random.default_rng(9)
    u = rng.uniform(-20, 20, (rows, 2 * H)).astype(np.float32)
    if bf16:
        u = B.from_bf16_bits(B.to_bf16_bits(u)).reshape(rows, 2 * H)
    dirty = u.copy()
    where = [(0, 0), (5, 71), (33, 72 + 3), (66, 143), (40, 17)]
    for k, (r, c) in enumerate(where):
        dirty[r, c] = (np.nan, np.inf, -np.inf)[k % 3]
    clean = run(u, H, "dense", bf16, {})[1]
    got = run(dirty, H, "dense", bf16, {})[1]
    bits = np.uint16 if bf16 else np.uint32
    same = clean.view(bits) == got.view(bits)
    hit = np.zeros((rows, H), bool)
    for r, c in where:
        hit[r, c % H] = True
    assert same[~hit].all() and not same[hit].any()


@gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_refused_arguments_return_invalid_value_and_leave_the_output_untouched(bf16):
    v = 8 if bf16 else 4
    dt = np.uint16 if bf16 else np.float32
    rows, H = 3, 4 * v
    U = strided.framed(np.zeros((rows, 2 * H), dt))
    Hf = strided.out_frame(rows, H, H + 2 * v, dt)
    esz = np.dtype(dt).itemsize
    refused = {
        "rows = 0": (U.ptr, U.ld, Hf.ptr, Hf.ld, 0, H),
        "H % vec": (U.ptr, U.ld, Hf.ptr, Hf.ld, rows, H - v // 2),
        "H = 0": (U.ptr, U.ld, Hf.ptr, Hf.ld, rows, 0),
        "ldu < 2H": (U.ptr, 2 * H - v, Hf.ptr, Hf.ld, rows, H),
        "ldh < H": (U.ptr, U.ld, Hf.ptr, H - v, rows, H),
        "ldu % vec": (U.ptr, U.ld + v // 2, Hf.ptr, Hf.ld, rows, H),
        "ldh % vec": (U.ptr, U.ld, Hf.ptr, Hf.ld + v // 2, rows, H),
        "u misaligned": (U.ptr + esz, U.ld, Hf.ptr, Hf.ld, rows, H),
        "h misaligned": (U.ptr, U.ld, Hf.ptr + esz, Hf.ld, rows, H),
        "partial overlap": (Hf.ptr, 2 * H, Hf.ptr + 16, 2 * H, rows, H),
        "same base, other ld": (Hf.ptr, 2 * H, Hf.ptr, 4 * H, rows, H),
        "h inside u": (Hf.ptr, 2 * H, Hf.ptr + H * esz, 2 * H, rows, H),
    }
    for what, args in refused.items():
        assert B.swiglu_raw(*args, bf16=bf16) == HIP_INVALID, what
    B.hip_check(B.lib().vithip_device_sync(), "sync")
    bits = Hf.download().view(np.uint16 if bf16 else np.uint32)
    assert (bits == strided.SENTINEL[np.dtype(dt)]).all(), "a refused call wrote"
    U.assert_untouched()


@gpu
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_row_offsets_past_two_to_the_31_elements_are_64_bit(bf16):
    """Three rows a little over 2^30 elements apart, in place: row 2 starts past element 2^31 (and past byte 2^32).  Only the three
    windows are ever written or read; the allocation's other bytes are never touched."""
    v, dt = (8, np.uint16) if bf16 else (4, np.float32)
    H, rows = 2 * v, 3
    ld = (1 << 30) + v
    esz = np.dtype(dt).itemsize
    u = np.random.default_rng(3).uniform(-20, 20, (rows, 2 * H)).astype(np.float32)
    if bf16:
        u = B.from_bf16_bits(B.to_bf16_bits(u)).reshape(rows, 2 * H)
    data = B.to_bf16_bits(u).reshape(u.shape) if bf16 else u
    L = B.lib()
    dev = B.DeviceArray(((rows - 1) * ld + 2 * H + 64,), dt)
    guard = np.full(64, strided.SENTINEL[np.dtype(dt)], np.uint16 if bf16 else np.uint32)
    for r in range(rows):
        row = np.ascontiguousarray(data[r])
        B.hip_check(L.vithip_memcpy_h2d(dev.ptr + r * ld * esz, row.ctypes.data, row.nbytes, None), "h2d")
        B.hip_check(L.vithip_memcpy_h2d(dev.ptr + (r * ld + 2 * H) * esz, guard.ctypes.data, guard.nbytes, None), "h2d")
    B.hip_check(L.vithip_device_sync(), "sync")
    assert B.swiglu_raw(dev.ptr, ld, dev.ptr, ld, rows, H, bf16) == 0
    B.hip_check(L.vithip_device_sync(), "sync")
    got = np.empty((rows, 2 * H + 64), dt)
    for r in range(rows):
        B.hip_check(L.vithip_memcpy_d2h(got[r].ctypes.data, dev.ptr + r * ld * esz, got[r].nbytes, None), "d2h")
    B.hip_check(L.vithip_device_sync(), "sync")
    dev.free()
    bits = np.uint16 if bf16 else np.uint32
    assert (got[:, 2 * H:].view(bits) == guard).all(), "written behind a row's 2H columns"
    assert np.array_equal(got[:, H:2 * H].view(bits), np.ascontiguousarray(data[:, H:]).view(bits)), "the value half changed"
    if bf16:
        check_bf16(np.ascontiguousarray(got[:, :H]), u, H, "bf16 far rows")
    else:
        check_f32(np.ascontiguousarray(got[:, :H]), u, H, "fp32 far rows")
