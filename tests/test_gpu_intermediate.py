"""Intermediate-layer outputs (vit_engine_intermediate_*, vithip_tap_f32): tokens or channel-major maps of chosen layers.

References: for the kernel, the LayerNorm kernel's own rows (or the source bits) rearranged by tests/tap_model.py, bit for bit; for
the engine, the live oracle's residual stream behind every layer (pyoracle.forward_image(..., want_stages=True): stages[l + 1] is
behind encoder layer l), optionally through its own LayerNorm with the final LayerNorm's weights.  Bars: 1e-3 x max |ref| per tap
(LOGIT_REL, the project's bar for rows the logits are a linear map of) and ten times the measured figure for fp32 engines, the
measured-and-doubled figures below for bf16 engines, and bitwise for everything the engine promises to keep bit-identical.
"""
import ctypes as C

import numpy as np
import pytest

import tap_model
from conftest import oracle_config
from engine_helpers import CONFIGS, CONSTS, device_features, engines, read_back, same_bits, weights  # noqa: F401 (fixtures)
from strided import SENTINEL
from test_gpu_preproc import DeviceImages
from test_input_u8_model import normalise_u8
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

LOGIT_REL = 1e-3
VIT_ERR_ARG = 1
HIP_INVALID = 1  # hipErrorInvalidValue
KINDS = tap_model.LAYOUTS


def rel_err(got, ref) -> float:
    return float(np.abs(got - ref).max()) / float(np.abs(ref).max())


def device_intermediate(eng, d_images, n, layers, kind, norm=True, u8=False, stream=0, d_out=None):
    shape = eng.intermediate_shape(n, layers, kind, norm)
    d_out = d_out or B.DeviceArray(shape)
    if u8:
        eng.intermediate_device_u8(d_images.ptr, n, d_out.ptr, layers, kind, norm, *CONSTS, stream=stream)
    else:
        eng.intermediate_device(d_images.ptr, n, d_out.ptr, layers, kind, norm, stream=stream)
    return read_back(eng, d_out, shape)


# ---- 1: the kernel, bit for bit ------------------------------------------------------------------------------------------

GUARD = 1024  # floats of sentinel in front of and behind the output buffer
SENT = SENTINEL[np.dtype(np.float32)]


class TapBuffer:
    """[GUARD | images x 3 blocks | GUARD] floats of sentinel on the device; a launch writes block 1 of every image."""

    def __init__(self, images, block):
        self.images, self.block = images, block
        self.dev = B.DeviceArray.from_numpy(np.full(2 * GUARD + images * 3 * block, SENT, np.uint32))
        self.ptr, self.stride = self.dev.ptr + (GUARD + block) * 4, 3 * block

    def check(self):
        """The written blocks [images][block] as float32, after asserting that every other word still holds the sentinel."""
        bits = self.dev.numpy()
        body = bits[GUARD:-GUARD].reshape(self.images, 3, self.block)
        assert (bits[:GUARD] == SENT).all() and (bits[-GUARD:] == SENT).all(), "guard frame touched"
        assert (body[:, 0] == SENT).all() and (body[:, 2] == SENT).all(), "written outside an image's block"
        return body[:, 1].copy().view(np.float32)

    def untouched(self):
        return bool((self.dev.numpy() == SENT).all())


@pytest.mark.parametrize("tokens", [2, 5, 10, 17, 197])  # P = 1, 4, 9 (unaligned channel runs), 16, 196 (no multiple of the tile)
@pytest.mark.parametrize("dim", [128, 192, 768, 1024])   # one vector with idle lanes, a partial first vector, 3 vectors, 4 vectors
def test_tap_kernel_gives_the_layernorm_bits_in_every_layout_and_writes_its_block_only(dim, tokens):
    rng = np.random.default_rng(1000 * dim + tokens)
    gamma = (1.0 + 0.1 * rng.standard_normal(dim)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(dim)).astype(np.float32)
    for images in (1, 3):
        x = (rng.standard_normal((images * tokens, dim)) * 2.0 + 0.5).astype(np.float32)
        rows = {True: B.layernorm(x, gamma, beta), False: x}
        assert not same_bits(rows[True], rows[False])
        for ldx in (dim, dim + 4):
            for norm in (True, False):
                for layout in KINDS:
                    want = tap_model.arrange(rows[norm], images, tokens, layout).reshape(images, -1)
                    buf = TapBuffer(images, tap_model.block_elems(tokens, dim, layout))
                    B.tap(x, gamma if norm else None, beta if norm else None, images, tokens, layout, ldx=ldx,
                          out_image_stride=buf.stride, d_out=buf.ptr)
                    got = buf.check()
                    assert same_bits(got, want), (images, ldx, norm, layout, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
        # and through the binding's own frames: one block per image, back to back
        got = B.tap(x, gamma, beta, images, tokens, "map")
        assert got.shape == (images, dim, tokens - 1) and same_bits(got, tap_model.arrange(rows[True], images, tokens, "map"))


@pytest.mark.parametrize("dim,tokens", [(512, 17), (512, 10), (2048, 17), (2048, 10), (2048, 37)])
def test_tap_kernel_gives_the_layernorm_bits_at_the_other_vector_counts(dim, tokens):
    """2 and 8 vectors per lane, the instances the shapes above leave out; above dim 1024 the map's tile is 16 tokens (37: three tiles)."""
    rng = np.random.default_rng(1000 * dim + tokens)
    gamma = (1.0 + 0.1 * rng.standard_normal(dim)).astype(np.float32)
    beta = (0.1 * rng.standard_normal(dim)).astype(np.float32)
    images = 3
    x = (rng.standard_normal((images * tokens, dim)) * 2.0 + 0.5).astype(np.float32)
    rows = {True: B.layernorm(x, gamma, beta), False: x}
    for norm in (True, False):
        for layout in KINDS:
            want = tap_model.arrange(rows[norm], images, tokens, layout).reshape(images, -1)
            buf = TapBuffer(images, tap_model.block_elems(tokens, dim, layout))
            B.tap(x, gamma if norm else None, beta if norm else None, images, tokens, layout, ldx=dim + 4,
                  out_image_stride=buf.stride, d_out=buf.ptr)
            assert same_bits(buf.check(), want), (norm, layout)


def test_tap_kernel_refuses_bad_arguments_and_leaves_the_buffer_untouched():
    L = B.lib()
    images, tokens, dim = 2, 5, 128
    d_x = B.DeviceArray.from_numpy(np.ones((images * tokens, dim + 4), np.float32))
    d_g, d_b = B.DeviceArray.from_numpy(np.ones(dim, np.float32)), B.DeviceArray.from_numpy(np.zeros(dim, np.float32))
    block = tokens * dim
    buf = TapBuffer(images, block)
    ok = dict(x=d_x.ptr, ldx=dim + 4, out=buf.ptr, stride=buf.stride, g=d_g.ptr, b=d_b.ptr, images=images, tokens=tokens, dim=dim, layout=1)
    bad = [dict(x=None), dict(out=None), dict(g=None), dict(b=None), dict(images=0), dict(images=-1), dict(tokens=0), dict(dim=0),
           dict(layout=4), dict(layout=-1), dict(layout=2, tokens=1), dict(layout=3, tokens=1), dict(dim=126), dict(dim=2052, ldx=2052),
           dict(ldx=dim - 4), dict(ldx=dim + 2), dict(stride=buf.stride + 2), dict(stride=block - 4), dict(layout=3, stride=(tokens - 1) * dim - 4),
           dict(layout=0, stride=dim - 4), dict(x=d_x.ptr + 4), dict(out=buf.ptr + 4), dict(g=d_g.ptr + 4), dict(b=d_b.ptr + 8),
           dict(images=1 << 30, tokens=4)]
    for change in bad:
        a = dict(ok, **change)
        rc = L.vithip_tap_f32(None, a["x"], a["ldx"], a["out"], a["stride"], a["g"], a["b"], a["images"], a["tokens"], a["dim"], a["layout"])
        assert rc == HIP_INVALID, (change, rc)
    B.hip_check(L.vithip_device_sync(), "sync")
    assert buf.untouched()
    with pytest.raises(B.VitError) as err:
        B.tap(np.ones((4, 8), np.float32), np.ones(8, np.float32), None, 2, 2, "cls")
    assert err.value.code == HIP_INVALID
    # the accepted call still works
    a = ok
    assert L.vithip_tap_f32(None, a["x"], a["ldx"], a["out"], a["stride"], a["g"], a["b"], images, tokens, dim, 1) == 0
    B.hip_check(L.vithip_device_sync(), "sync")
    assert (buf.check() == 0.0).all()  # LayerNorm of constant rows with beta = 0


# ---- 2, 3: engines against the live oracle -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def oracle_stages(oracle, weights):
    """(model, n) -> (images, per image the oracle's residual streams), computed once and shared."""
    cache = {}

    def get(name, n):
        if (name, n) not in cache:
            cfg, W = CONFIGS[name], weights(name, 21)
            imgs = synth.make_images(cfg, n, 100 + n)
            ocfg = oracle_config(cfg)
            cache[(name, n)] = (imgs, [oracle.forward_image(ocfg, im, W, want_stages=True)[2] for im in imgs])
        return cache[(name, n)]

    return get


def worst_tap_error(got, ref) -> float:
    """The largest max |d| / max |ref| over the taps (blocks) of the rows."""
    return max(rel_err(got[:, j], ref[:, j]) for j in range(ref.shape[1]))


# Measured on an MI355X (profiles/r13/README.md): the largest max |d| / max |ref| per tap over both models, all n, the four kinds
# and norm = 0 / 1 (VIT_SMALL; VIT_TINY shows 5.6e-7).  It sits far below the logits bar, so ten times it is asserted as well: a
# regression of two orders of magnitude cannot hide under 1e-3.
FP32_MEASURED = 1.103e-6


@pytest.mark.parametrize("name", ["tiny", "small"])
def test_fp32_intermediate_rows_match_the_live_oracle(oracle, engines, weights, oracle_stages, name):
    cfg, W = CONFIGS[name], weights(name, 21)
    eng = engines(name, 21, max_batch=4)  # chunk loop and ragged tails
    layers = list(range(cfg.depth))
    g = cfg.img_size // cfg.patch_size
    worst = 0.0
    for n in (1, 5, 11):
        imgs, stages = oracle_stages(name, n)
        for kind in KINDS:
            for norm in (0, 1):
                ref = tap_model.intermediate_reference(oracle, stages, layers, W[-4], W[-3], kind, norm, grid=g)
                got = eng.intermediate(imgs, layers, kind, norm)
                assert got.shape == ref.shape == eng.intermediate_shape(n, layers, kind, norm)
                err = worst_tap_error(got, ref)
                print(f"fp32 {name} n={n} {kind} norm={norm}: worst tap max |d| / max |ref| = {err:.3e}")
                worst = max(worst, err)
                assert err <= LOGIT_REL, (n, kind, norm, err)
    print(f"fp32 {name}: worst = {worst:.3e}")
    assert worst <= 10 * FP32_MEASURED, worst  # measured: tiny 5.562e-7, small 1.103e-6


# No project bar exists for bf16 activations.  Measured on an MI355X (profiles/r13/README.md): the largest max |d| / max |ref| per
# tap against the oracle over n = 1, 3, 8, per (kind, norm); the assertion is twice the measured value rounded up to one significant
# digit (the rule of BF16_BAR in tests/test_gpu_features.py), and more than 1e-5: really the bf16 path.
BF16_MEASURED = {("cls", 0): 4.933e-3, ("cls", 1): 4.215e-3, ("tokens", 0): 2.917e-3, ("tokens", 1): 3.354e-3,
                 ("patches", 0): 2.917e-3, ("patches", 1): 3.391e-3, ("map", 0): 2.917e-3, ("map", 1): 3.391e-3}
BF16_BAR = {("cls", 0): 1e-2, ("cls", 1): 9e-3, ("tokens", 0): 6e-3, ("tokens", 1): 7e-3,
            ("patches", 0): 6e-3, ("patches", 1): 7e-3, ("map", 0): 6e-3, ("map", 1): 7e-3}


def test_bf16_intermediate_rows_against_the_live_oracle(oracle, engines, weights, oracle_stages):
    cfg, W = synth.VIT_SMALL, weights("small", 21)
    eng = engines("small", 21, max_batch=4, dtype="bf16")
    layers = list(range(cfg.depth))
    g = cfg.img_size // cfg.patch_size
    worst = {(k, norm): 0.0 for k in KINDS for norm in (0, 1)}
    for n in (1, 3, 8):
        imgs, stages = oracle_stages("small", n)
        for kind, norm in worst:
            ref = tap_model.intermediate_reference(oracle, stages, layers, W[-4], W[-3], kind, norm, grid=g)
            err = worst_tap_error(eng.intermediate(imgs, layers, kind, norm), ref)
            print(f"bf16 small n={n} {kind} norm={norm}: worst tap max |d| / max |ref| = {err:.3e}")
            worst[kind, norm] = max(worst[kind, norm], err)
    print("bf16 small: worst =", {k: f"{v:.3e}" for k, v in worst.items()})
    for key, err in worst.items():
        assert err > 1e-5, (key, err)  # really the bf16 path: fp32 engines sit near 1e-6
        assert err <= BF16_BAR[key], (key, err, BF16_MEASURED[key])  # 2 x measured, rounded up to one significant digit


# ---- 4: bitwise identities -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name,mb,n", [("tiny", 16, 19), ("b16", 16, 19)])
def test_last_layer_taps_are_the_feature_rows_blocks_stand_alone_and_pruning_changes_no_bit(engines, name, mb, n, dtype):
    cfg = CONFIGS[name]
    imgs = synth.make_images(cfg, n, 401)
    plain, pruned = engines(name, max_batch=mb, dtype=dtype), engines(name, max_batch=mb, dtype=dtype, prune_last_layer=True)
    last, g = cfg.depth - 1, cfg.img_size // cfg.patch_size
    before = plain.forward(imgs)
    tok = plain.intermediate(imgs, [-1], "tokens", True)
    assert same_bits(tok[:, 0], plain.features(imgs, "tokens"))
    cls = plain.intermediate(imgs, [last], "cls", True)
    assert same_bits(cls[:, 0], plain.features(imgs, "cls")) and same_bits(cls[:, 0], tok[:, 0, 0])
    with pytest.raises(B.VitError):  # nothing wrote logits
        plain.logits(1)
    # the layouts of one layer are one set of rows
    pat = plain.intermediate(imgs, [last], "patches", True)
    assert same_bits(pat[:, 0], tok[:, 0, 1:])
    assert same_bits(plain.intermediate(imgs, [last], "map", True)[:, 0].reshape(n, cfg.embed_dim, g * g), pat[:, 0].transpose(0, 2, 1))
    # block j of a call does not depend on the other layers tapped; norm = 0 differs from norm = 1
    for kind in (KINDS if name == "tiny" else ("cls", "map")):  # b16: the wide kinds would be 140 MB of rows per call
        every = plain.intermediate(imgs, range(cfg.depth), kind, True)
        two = plain.intermediate(imgs, (0, last), kind, True)
        assert same_bits(two[:, 0], every[:, 0]) and same_bits(two[:, 1], every[:, last]), kind
        assert same_bits(plain.intermediate(imgs, [0], kind, True)[:, 0], every[:, 0]), kind
        raw = plain.intermediate(imgs, (0, last), kind, False)
        assert not same_bits(raw, two)
        # prune_last_layer: CLS through the pruned layer, the other kinds make the call run it unpruned; untapped, it does not run
        assert same_bits(pruned.intermediate(imgs, (0, last), kind, True), two), kind
        assert same_bits(pruned.intermediate(imgs, (0, last), kind, False), raw), kind
        assert same_bits(pruned.intermediate(imgs, [0], kind, True)[:, 0], every[:, 0]), kind
    assert same_bits(plain.forward(imgs), before) and same_bits(pruned.forward(imgs), before)
    assert plain.logits(1).shape == (1, cfg.num_classes)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["tiny", "b16"])
def test_lanes_change_no_bit(engines, name, dtype):
    cfg = CONFIGS[name]
    imgs = synth.make_images(cfg, 37, 402)  # chunks of 16, 16, 5: four lanes, four lanes, two lanes
    eng = engines(name, max_batch=16, dtype=dtype)
    layers = (cfg.depth // 2 - 1, cfg.depth - 1)
    calls = [(k, norm) for k in (KINDS if name == "tiny" else ("cls", "map")) for norm in (0, 1)]
    want = {c: eng.intermediate(imgs, layers, *c) for c in calls}
    try:
        for lanes in (2, 4):
            eng.set_lanes(lanes)
            for c, w in want.items():
                assert same_bits(eng.intermediate(imgs, layers, *c), w), (lanes, c)
    finally:
        eng.set_lanes(1)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_an_images_row_is_the_same_wherever_it_sits(engines, dtype):
    eng = engines("small", max_batch=4, dtype=dtype)
    base = synth.make_images(eng.cfg, 3, 403)
    idx = np.array([0, 1, 2, 2, 0, 1, 1, 0, 2, 0, 1])  # chunks of 4, 4, 3
    for kind in KINDS:
        got = eng.intermediate(base[idx], (0, 2), kind, True)
        alone = [eng.intermediate(base[k:k + 1], (0, 2), kind, True)[0] for k in range(3)]
        for pos, k in enumerate(idx):
            assert same_bits(got[pos], alone[k]), (kind, pos, k)
        assert not same_bits(alone[0], alone[1])


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_host_device_u8_and_images_calls_agree_bit_for_bit(engines, dtype):
    eng = engines("small", max_batch=4, dtype=dtype)
    cfg, n = eng.cfg, 11
    u8 = np.random.default_rng(404).integers(0, 256, size=(n, cfg.img_size, cfg.img_size, cfg.in_chans), dtype=np.uint8)
    x = normalise_u8(u8, *CONSTS)
    d_x, d_u8, dev = B.DeviceArray.from_numpy(x), B.DeviceArray.from_numpy(u8), DeviceImages(list(u8), lead=0)
    before = eng.forward(x)
    for kind, layers, norm in (("tokens", (0, 1, 2), 1), ("cls", (1,), 0), ("map", (0, 2), 1), ("patches", (2,), 0)):  # widest row first
        host = eng.intermediate(x, layers, kind, norm)
        shape = host.shape
        assert same_bits(device_intermediate(eng, d_x, n, layers, kind, norm), host), kind
        assert same_bits(eng.intermediate_u8(u8, layers, kind, norm, *CONSTS), host), kind
        assert same_bits(device_intermediate(eng, d_u8, n, layers, kind, norm, u8=True), host), kind
        # decoded images of the model's own size: the resize is skipped and the crop is the whole image
        assert same_bits(eng.intermediate_images(list(u8), cfg.img_size, layers, kind, norm, *CONSTS), host), kind
        d_out = B.DeviceArray(shape)
        eng.intermediate_device_images(dev.triples, d_out.ptr, cfg.img_size, layers, kind, norm, *CONSTS)
        assert same_bits(read_back(eng, d_out, shape), host), kind
    # the probabilities still come through the (regrown) staging unharmed
    assert same_bits(eng.forward_u8(u8, *CONSTS), before)


# ---- 5: graph --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_graph_cache_keys_on_the_whole_spec(engines, dtype):
    """One input buffer and ONE output buffer for every call: only the output descriptor tells the calls apart."""
    plain = engines("small", max_batch=8, dtype=dtype)
    graph = engines("small", max_batch=8, dtype=dtype, use_graph=True)
    cfg, n = plain.cfg, 6
    d_images = B.DeviceArray.from_numpy(synth.make_images(cfg, n, 405))
    d_out = B.DeviceArray((n, max(cfg.depth * cfg.tokens * cfg.embed_dim, cfg.num_classes)))

    def run(eng, what):
        if what == "probs":
            eng.forward_device(d_images.ptr, n, d_out.ptr)
            eng.sync()
            return d_out.numpy().reshape(-1)[:n * cfg.num_classes].copy()
        if what[0] == "features":
            return device_features(eng, d_images, n, what[1], d_out=d_out)
        return device_intermediate(eng, d_images, n, *what, d_out=d_out)

    a, b, c = ((0,), "cls", 1), ((1,), "cls", 1), ((2,), "cls", 1)  # the same row width: they differ in `layers` alone
    calls = [a, b, a, a, "probs", c, ("features", "cls"), c, ((0, 1), "cls", 1), ((0, 2), "cls", 1), ((0, 2), "cls", 0), "probs",
             ((0, 2), "map", 0), ((0, 2), "patches", 0), ((0, 1, 2), "tokens", 1), ("features", "tokens"), ((2,), "tokens", 1), b, "probs"]
    want = {w: run(plain, w) for w in set(calls)}
    for w in calls:
        assert same_bits(run(graph, w), want[w]), w
    assert not same_bits(want[a], want[b]) and not same_bits(want[b], want[c])
    assert not same_bits(want[((0, 1), "cls", 1)], want[((0, 2), "cls", 1)])
    assert same_bits(want[c][:, 0], want[("features", "cls")])


# ---- 6: early stop ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lanes", [1, 2])
def test_layers_behind_the_deepest_tap_are_not_launched(engines, lanes):
    eng = engines("small", max_batch=4, lanes=lanes, profile=True, ln_fold=-1)
    n, depth = 4, eng.cfg.depth
    imgs = synth.make_images(eng.cfg, n, 406)

    def launches(fn):
        eng.reset_stage_times()
        fn()
        t = eng.stage_times()
        assert t["images"] == n
        return {s: v["launches"] for s, v in t["stages"].items()}

    probs = launches(lambda: eng.forward(imgs))
    gemms = ("qkv", "attn", "outproj", "fc1", "fc2")
    assert all(probs[s] == depth * lanes for s in gemms) and probs["head"] == lanes and probs["softmax"] == lanes
    assert probs["ln"] == (2 * depth + 1) * lanes  # two per layer and the head's
    for kind in KINDS:
        got = launches(lambda: eng.intermediate(imgs, [0], kind, 1))
        assert all(got[s] == lanes for s in gemms), (kind, got)       # exactly one layer
        assert got["head"] == 0 and got["softmax"] == 0, (kind, got)
        assert got["ln"] == (2 + 1) * lanes and got["embed"] == probs["embed"], (kind, got)
    got = launches(lambda: eng.intermediate(imgs, (0, 1), "map", 0))
    assert all(got[s] == 2 * lanes for s in gemms) and got["ln"] == (4 + 2) * lanes and got["head"] == 0
    got = launches(lambda: eng.intermediate(imgs, range(depth), "cls", 1))
    assert all(got[s] == depth * lanes for s in gemms) and got["ln"] == (2 * depth + depth) * lanes and got["softmax"] == 0


# ---- 7: errors -------------------------------------------------------------------------------------------------------------

def test_invalid_arguments_return_vit_err_arg_and_leave_the_engine_usable(engines):
    L = B.lib()
    eng = engines("small", max_batch=4)
    cfg, n = eng.cfg, 3
    imgs = synth.make_images(cfg, n, 407)
    u8 = np.random.default_rng(408).integers(0, 256, size=(n, cfg.img_size, cfg.img_size, cfg.in_chans), dtype=np.uint8)
    ref, ref_tap = eng.forward(imgs), eng.intermediate(imgs, (0, 2), "map", 1)
    d_x, d_u8 = B.DeviceArray.from_numpy(imgs), B.DeviceArray.from_numpy(u8)
    d_out = B.DeviceArray((n, cfg.depth, cfg.tokens, cfg.embed_dim))
    mean, std = (C.c_float * 3)(*B.IMAGENET_MEAN), (C.c_float * 3)(*B.IMAGENET_STD)
    zero_std = (C.c_float * 3)(0.229, 0.0, 0.225)

    def spec(layers=(0, 2), kind=0, norm=1, reserved=0, num=None):
        s = B.intermediate_spec(layers, kind, norm, reserved=reserved)
        if num is not None:
            s.num_layers = num
        return s

    def still_fine():
        assert L.vit_engine_last_error(eng._h)
        assert same_bits(eng.forward(imgs), ref)
        assert same_bits(eng.intermediate(imgs, (0, 2), "map", 1), ref_tap)

    bad_specs = {"kind": spec(kind=4), "kind<0": spec(kind=-1), "norm": spec(norm=2), "norm<0": spec(norm=-1), "none": spec(num=0),
                 "negative count": spec(num=-1), "too many": spec(range(33)), "reserved": spec(reserved=1), "deep": spec((0, 3)),
                 "negative layer": spec((-1,)), "equal": spec((1, 1)), "falling": spec((2, 1)), "late": spec((0, 1, 2, 2), num=4)}
    for why, s in bad_specs.items():
        assert L.vit_engine_intermediate_device(eng._h, d_x.ptr, n, C.byref(s), d_out.ptr, None) == VIT_ERR_ARG, why
        assert L.vit_engine_intermediate_row_elems(eng._h, C.byref(s)) == 0, why
        msg = L.vit_engine_last_error(eng._h).decode()
        assert msg.startswith("intermediate_device:"), msg
        if why in ("deep", "negative layer"):
            assert "layers[%d]" % (1 if why == "deep" else 0) in msg, msg
        if why in ("equal", "falling"):
            assert "layers[1]" in msg, msg
        if why == "late":
            assert "layers[3]" in msg, msg
        still_fine()
    good = C.byref(spec())
    for d_images, nn, sp, out in [(None, n, good, d_out.ptr), (d_x.ptr, n, good, None), (d_x.ptr, n, None, d_out.ptr),
                                  (d_x.ptr, 0, good, d_out.ptr), (d_x.ptr, -1, good, d_out.ptr)]:
        assert L.vit_engine_intermediate_device(eng._h, d_images, nn, sp, out, None) == VIT_ERR_ARG
        still_fine()
    for d_images, nn, m, s, sp in [(d_u8.ptr, n, None, std, good), (d_u8.ptr, n, mean, zero_std, good), (d_u8.ptr + 1, n, mean, std, good),
                                   (d_u8.ptr, n, mean, std, C.byref(bad_specs["deep"])), (d_u8.ptr, 0, mean, std, good)]:
        assert L.vit_engine_intermediate_device_u8(eng._h, d_images, nn, m, s, sp, d_out.ptr, None) == VIT_ERR_ARG
        still_fine()
    out = np.empty((n, cfg.depth, cfg.tokens, cfg.embed_dim), np.float32)
    rows = (B.f32p * n)(*[out[i].ctypes.data_as(B.f32p) for i in range(n)])
    holes = (B.f32p * n)(*[out[i].ctypes.data_as(B.f32p) if i != 1 else None for i in range(n)])
    in_f32 = (B.f32p * n)(*[imgs[i].ctypes.data_as(B.f32p) for i in range(n)])
    in_u8 = (C.c_void_p * n)(*[u8[i].ctypes.data for i in range(n)])
    for ptrs, nn, sp, r in [(None, n, good, rows), (in_f32, n, good, None), (in_f32, 0, good, rows), (in_f32, n, None, rows),
                            (in_f32, n, C.byref(bad_specs["falling"]), rows), (in_f32, n, good, holes)]:
        assert L.vit_engine_intermediate_host(eng._h, ptrs, nn, sp, r) == VIT_ERR_ARG
        still_fine()
    for ptrs, nn, m, s, sp, r in [(in_u8, n, mean, None, good, rows), (in_u8, n, mean, zero_std, good, rows),
                                  (in_u8, n, mean, std, C.byref(bad_specs["kind"]), rows), (None, n, mean, std, good, rows)]:
        assert L.vit_engine_intermediate_host_u8(eng._h, ptrs, nn, m, s, sp, r) == VIT_ERR_ARG
        still_fine()
    keep, recs = B.host_image_records(list(u8), cfg.in_chans)
    small_pp, pp = B.preproc_params(cfg.img_size - 4, *CONSTS, cfg.in_chans), B.preproc_params(cfg.img_size, *CONSTS, cfg.in_chans)
    for p, sp in [(None, good), (C.byref(small_pp), good), (C.byref(pp), C.byref(bad_specs["norm"]))]:
        assert L.vit_engine_intermediate_host_images(eng._h, recs, n, p, sp, rows) == VIT_ERR_ARG
        still_fine()
    D, T = cfg.embed_dim, cfg.tokens
    widths = {0: 2 * D, 1: 2 * T * D, 2: 2 * (T - 1) * D, 3: 2 * D * (T - 1)}
    for k, w in widths.items():
        assert L.vit_engine_intermediate_row_elems(eng._h, C.byref(spec(kind=k))) == w
    assert L.vit_engine_intermediate_row_elems(eng._h, None) == 0 and L.vit_engine_intermediate_row_elems(None, good) == 0
    with pytest.raises(B.VitError):
        eng.intermediate(imgs, (0, 5), "cls")
    with pytest.raises(B.VitError):
        eng.intermediate_shape(n, (), "cls")
    assert eng.intermediate_shape(n, (-1,), "map") == (n, 1, D, 4, 4)
    still_fine()
