"""The 18 forward entry points as one surface: output kind x place x input kind, every call made raw through the C-ABI.

Same pixels, same bits: six random 32 x 32 images are handed over as 8-bit pixels, as the fp32 images the host restatement of the
normalisation makes of them (tests/test_input_u8_model.py) and as decoded images with resize_shorter = 32 (at equal sizes the resize
is skipped and the crop is the whole image); every output then has the same bytes whichever of the six calls returned it.  Refusals
name their call and come in one order.  Both tests run over CALLS, which must be the surface test_call_surface_abi.py writes out.
"""
import ctypes as C

import numpy as np
import pytest

from engine_helpers import CONSTS, cfloats, read_back, same_bits
from test_call_surface_abi import ARGTYPES
from test_gpu_preproc import DeviceImages
from test_input_u8_model import normalise_u8
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

VIT_ERR_ARG, VIT_ERR_STATE = 1, 5
CFG, MAX_BATCH, N = synth.VIT_TINY, 4, 6  # both places run N as pieces of 4 + 2
SPECS = {"forward": (None,), "features": ("cls", "mean", "tokens"), "cls_attention": ("heads", "head_mean")}
CALLS = [(out, place, inp) for out in SPECS for place in ("device", "host") for inp in ("", "_u8", "_images")]


def who(call) -> str:
    return "{}_{}{}".format(*call)


def test_calls_are_the_whole_surface():
    assert len(CALLS) == 18 and {"vit_engine_" + who(c) for c in CALLS} == set(ARGTYPES)


class Data:
    """The six images in every form a call takes, and what keeps them alive."""

    def __init__(self):
        self.u8 = np.random.default_rng(1201).integers(0, 256, size=(N, CFG.img_size, CFG.img_size, CFG.in_chans), dtype=np.uint8)
        self.f32 = normalise_u8(self.u8, *CONSTS)
        self.d_f32, self.d_u8 = B.DeviceArray.from_numpy(self.f32), B.DeviceArray.from_numpy(self.u8)
        self.dev = DeviceImages(list(self.u8), lead=0)
        self.keep, host_recs = B.host_image_records(list(self.u8), CFG.in_chans)
        self.images = {("device", ""): self.d_f32.ptr, ("device", "_u8"): self.d_u8.ptr, ("device", "_images"): self.dev.records,
                       ("host", ""): (B.f32p * N)(*[im.ctypes.data_as(B.f32p) for im in self.f32]),
                       ("host", "_u8"): (C.c_void_p * N)(*[im.ctypes.data for im in self.u8]), ("host", "_images"): host_recs}
        self.mean, self.std = cfloats(CONSTS[0]), cfloats(CONSTS[1])
        self.pp = B.preproc_params(CFG.img_size, *CONSTS, CFG.in_chans)

    def norm(self, inp, mean="given"):
        """The arguments between n and the spec."""
        mean = self.mean if mean == "given" else mean
        return {"": [], "_u8": [mean, self.std], "_images": [C.byref(self.pp)]}[inp]


@pytest.fixture(scope="module")
def data():
    return Data()


@pytest.fixture(scope="module")
def engines():
    """One fp32 and one bf16 engine with weights, and one without."""
    W = synth.make_weights(CFG, 1234)
    engs = {dtype: B.Engine(CFG, max_batch=MAX_BATCH, dtype=dtype) for dtype in ("f32", "bf16")}
    for eng in engs.values():
        eng.load_weights(W)
    engs["empty"] = B.Engine(CFG, max_batch=MAX_BATCH)
    yield engs
    for eng in engs.values():
        eng.close()


def spec_arg(out, kind):
    if out == "forward":
        return []
    return [C.byref(B.feature_spec(kind) if out == "features" else B.attention_spec(kind))]


def shape_of(eng, out, kind, n=N):
    if out == "forward":
        return (n, CFG.num_classes)
    return eng.feature_shape(n, kind) if out == "features" else eng.attention_shape(n, kind)


def tail(call):
    """What follows the destination: a device forward's top-1 pointers, a device call's stream."""
    out, place, _ = call
    return [] if place == "host" else ([None, None] if out == "forward" else []) + [None]


def raw(handle, call, images, n, norm, spec, dst):
    return getattr(B.lib(), "vit_engine_" + who(call))(handle, images, n, *norm, *spec, dst, *tail(call))


def run(eng, call, data, kind):
    """The rows `call` returns for the six images."""
    out, place, inp = call
    blank = np.full(shape_of(eng, out, kind), np.nan, np.float32)
    if place == "device":
        d_out = B.DeviceArray.from_numpy(blank)
        dst = d_out.ptr
    else:
        dst = (B.f32p * N)(*[row.ctypes.data_as(B.f32p) for row in blank])
    rc = raw(eng._h, call, data.images[place, inp], N, data.norm(inp), spec_arg(out, kind), dst)
    assert rc == 0, (who(call), rc, B.lib().vit_engine_last_error(eng._h))
    return read_back(eng, d_out, blank.shape) if place == "device" else blank


# ---- same pixels, same bits ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def first_rows(engines, data):
    """(dtype, lanes, out, kind) -> the rows of the fp32 device call, computed once: what the other five calls must equal."""
    cache = {}

    def get(dtype, lanes, out, kind):
        if (dtype, lanes, out, kind) not in cache:
            engines[dtype].set_lanes(lanes)
            rows = run(engines[dtype], (out, "device", ""), data, kind)
            assert np.isfinite(rows).all()
            cache[dtype, lanes, out, kind] = rows
        return cache[dtype, lanes, out, kind]

    return get


@pytest.mark.parametrize("lanes", [1, 2])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("call", CALLS, ids=who)
def test_same_pixels_give_the_same_bits_through_every_call(engines, data, first_rows, call, dtype, lanes):
    eng = engines[dtype]
    for kind in SPECS[call[0]]:
        ref = first_rows(dtype, lanes, call[0], kind)
        eng.set_lanes(lanes)
        assert same_bits(run(eng, call, data, kind), ref), (who(call), kind)


# ---- refusals name their call ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def earlier(engines, data):
    eng = engines["f32"]
    eng.set_lanes(1)
    return eng.forward(data.f32), eng.features(data.f32, "cls"), eng.cls_attention(data.f32, "heads")


@pytest.mark.parametrize("call", CALLS, ids=who)
def test_refusals_name_their_call_and_leave_the_engine_usable(engines, data, earlier, call):
    L = B.lib()
    eng, empty = engines["f32"], engines["empty"]
    eng.set_lanes(1)
    out, place, inp = call
    kind = SPECS[out][0]
    images, norm, spec = data.images[place, inp], data.norm(inp), spec_arg(out, kind)
    rows = np.empty(shape_of(eng, out, kind), np.float32)
    d_out = B.DeviceArray(rows.shape)
    dst = d_out.ptr if place == "device" else (B.f32p * N)(*[row.ctypes.data_as(B.f32p) for row in rows])

    def refused(handle, *args):
        assert raw(handle, call, *args) == VIT_ERR_ARG
        return L.vit_engine_last_error(handle).decode() if handle else None

    for args in [(None, N, norm, spec, dst), (images, N, norm, spec, None), (images, 0, norm, spec, dst)]:
        assert refused(eng._h, *args).startswith(f"{who(call)}: bad arguments (n=")
    if inp == "_u8":
        assert refused(eng._h, images, N, data.norm(inp, mean=None), spec, dst) == f"{who(call)}: mean and std are required"
        if out == "features":  # the input is judged before the output spec
            unknown = [C.byref(B.feature_spec(7))]
            assert refused(eng._h, images, N, data.norm(inp, mean=None), unknown, dst) == f"{who(call)}: mean and std are required"
        if place == "device":
            assert refused(eng._h, images + 1, N, norm, spec, dst) == f"{who(call)}: d_images must be 4-byte aligned"
    refused(None, images, N, norm, spec, dst)  # a NULL engine: the code, no message to read, no crash
    # without weights the arguments are still judged first; only a call that passes them learns about the weights
    assert refused(empty._h, images, 0, norm, spec, dst).startswith(f"{who(call)}: bad arguments (n=")
    assert raw(empty._h, call, images, N, norm, spec, dst) == VIT_ERR_STATE
    for got, ref in zip((eng.forward(data.f32), eng.features(data.f32, "cls"), eng.cls_attention(data.f32, "heads")), earlier):
        assert same_bits(got, ref)
