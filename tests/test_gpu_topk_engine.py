"""vit_engine_topk_*: the k best classes of every image as records, on the GPU.

The expectation is tests/topk_model.py applied to what the SAME engine's forward returns (probabilities) or to its logits
(vit_engine_read_logits); every comparison is bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import topk_model as M
from engine_helpers import CONSTS, device_forward, engines, same_bits, weights  # noqa: F401  (fixtures)
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

VIT_ERR_ARG = 1
DTYPES = ["f32", "bf16"]


def read_records(d_out, n, k):
    B.hip_check(B.lib().vithip_device_sync(), "sync")
    got = np.empty((n, 2 * k), np.int32)
    B.hip_check(B.lib().vithip_memcpy_d2h(got.ctypes.data, d_out.ptr, got.nbytes, None), "d2h")
    B.hip_check(B.lib().vithip_device_sync(), "sync")
    return got


def device_topk(eng, d_images, n, k, score="prob", u8=False, stream=0, d_out=None):
    d_out = d_out or B.DeviceArray(eng.topk_shape(n, k), np.int32)
    if u8:
        eng.topk_device_u8(d_images.ptr, n, d_out.ptr, k, score, *CONSTS, stream=stream)
    else:
        eng.topk_device(d_images.ptr, n, d_out.ptr, k, score, stream=stream)
    return read_records(d_out, n, k)


def prob_records(probs, k):
    return M.topk_records(probs, k, M.EMPTY_SCORE["prob"])


def logit_records(logits, k):
    return M.topk_records(logits, k, M.EMPTY_SCORE["logit"])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["tiny", "small"])
def test_records_are_the_model_on_the_engines_own_forward(engines, name, dtype):
    eng = engines(name, max_batch=2, dtype=dtype)
    cfg, n, k = eng.cfg, 5, 3  # three chunks: 2, 2, 1
    imgs = synth.make_images(cfg, n, 701)
    d_x = B.DeviceArray.from_numpy(imgs)
    probs, label, prob = device_forward(eng, d_x, n)
    logits_fwd = eng.logits(1)
    assert eng.topk_shape(n, k) == (n, 2 * k)
    got = device_topk(eng, d_x, n, k)
    assert same_bits(got, prob_records(probs, k))
    labels, scores = B.split_topk(got)
    assert same_bits(labels[:, 0], label) and same_bits(scores[:, 0], prob)
    got = device_topk(eng, d_x, n, k, "logit")
    logits = eng.logits(1)  # the last chunk: image 4
    assert same_bits(logits, logits_fwd)
    assert same_bits(got[4:5], logit_records(logits, k))
    with pytest.raises(B.VitError):
        eng.logits(2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_all_six_calls_give_the_same_bits(engines, dtype):
    eng = engines("small", max_batch=4, dtype=dtype)
    cfg, n, k = eng.cfg, 5, 4
    S, Cc = cfg.img_size, cfg.in_chans
    u8 = np.random.default_rng(702).integers(0, 256, size=(n, S, S, Cc), dtype=np.uint8)
    x = B.images_u8_to_f32(u8, *CONSTS)
    d_x, d_u8 = B.DeviceArray.from_numpy(x), B.DeviceArray.from_numpy(u8)
    triples = [(d_u8.ptr + i * S * S * Cc, S, S) for i in range(n)]  # height = width = resize_shorter = img_size: no resize
    for score in ("prob", "logit"):
        host = eng.topk_host(x, k, score)
        assert host.dtype == np.int32 and host.shape == (n, 2 * k)
        assert same_bits(device_topk(eng, d_x, n, k, score), host), score
        assert same_bits(eng.topk_host_u8(u8, k, score, *CONSTS), host), score
        assert same_bits(device_topk(eng, d_u8, n, k, score, u8=True), host), score
        assert same_bits(eng.topk_host_images(list(u8), S, k, score, *CONSTS), host), score
        d_out = B.DeviceArray((n, 2 * k), np.int32)
        eng.topk_device_images(triples, d_out.ptr, S, k, score, *CONSTS)
        assert same_bits(read_records(d_out, n, k), host), score
    assert same_bits(eng.topk_host(x, k), prob_records(eng.forward(x), k))


@pytest.mark.parametrize("dtype", DTYPES)
def test_lanes_and_pruning_change_no_bit(engines, dtype):
    n, k = 7, 5
    imgs = synth.make_images(synth.VIT_SMALL, n, 703)
    want = None
    for lanes in (1, 2):
        for prune in (False, True):
            eng = engines("small", max_batch=4, dtype=dtype, lanes=lanes, prune_last_layer=prune)
            got = [eng.topk_host(imgs, k, score) for score in ("prob", "logit")]
            want = want or got
            assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), (lanes, prune)
    assert same_bits(want[0], prob_records(engines("small", max_batch=4, dtype=dtype).forward(imgs), k))


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_image_has_the_same_row_wherever_it_sits(engines, dtype):
    eng = engines("small", max_batch=4, dtype=dtype)
    n, k = 7, 5
    imgs = synth.make_images(eng.cfg, n, 704)
    for pos in (0, 3, 6):
        imgs[pos] = imgs[0]
    for score in ("prob", "logit"):
        got = eng.topk_host(imgs, k, score)
        assert same_bits(got[3], got[0]) and same_bits(got[6], got[0]), score
        assert not same_bits(got[1], got[0])


def test_host_rows_wider_than_the_classes_grow_the_staging_and_leave_the_other_calls_working(engines, weights):
    cfg = synth.VIT_TINY
    eng = B.Engine(cfg, max_batch=4)  # a fresh one: its output staging is at the classes-sized start
    try:
        eng.load_weights(weights("tiny", 1234))
        n, k = 6, 8  # 2k = 16 words > 10 classes
        imgs = synth.make_images(cfg, n, 705)
        probs = eng.forward(imgs)
        got = eng.topk_host(imgs, k)
        assert same_bits(got, prob_records(probs, k))
        assert same_bits(eng.forward(imgs), probs)
        tokens = eng.features(imgs, "tokens")
        assert same_bits(tokens, engines("tiny", max_batch=4).features(imgs, "tokens"))
        assert same_bits(eng.topk_host(imgs, k), got)
        by_logit = eng.topk_host(imgs, 10, "logit")  # k = classes; the call's pieces are 4 + 2 images
        assert same_bits(by_logit[4:], logit_records(eng.logits(2), 10))
        assert same_bits(eng.forward(imgs), probs)
    finally:
        eng.close()


@pytest.mark.parametrize("dtype", DTYPES)
def test_graph_cache_keeps_forwards_and_topk_calls_apart(engines, dtype):
    """One input buffer, ONE output buffer and one explicit stream for every call: only the output descriptor tells them apart."""
    plain = engines("tiny", max_batch=8, dtype=dtype)
    graph = engines("tiny", max_batch=8, dtype=dtype, use_graph=True)
    cfg, n = plain.cfg, 6
    L = B.lib()
    stream = C.c_void_p()
    L.vithip_stream_create.argtypes = [C.POINTER(C.c_void_p)]
    L.vithip_stream_destroy.argtypes = [C.c_void_p]
    B.hip_check(L.vithip_stream_create(C.byref(stream)), "stream")
    try:
        d_images = B.DeviceArray.from_numpy(synth.make_images(cfg, n, 706))
        d_out = B.DeviceArray((n, cfg.num_classes))  # 10 words a row: holds k = 3 and k = 5 records too

        def run(eng, what):
            if what == "probs":
                eng.forward_device(d_images.ptr, n, d_out.ptr, stream=stream.value)
                B.hip_check(L.vithip_device_sync(), "sync")
                return d_out.numpy().copy()
            k, score = what
            eng.topk_device(d_images.ptr, n, d_out.ptr, k, score, stream=stream.value)
            return read_records(d_out, n, k)

        calls = ["probs", (3, "prob"), (5, "prob"), (3, "logit"), "probs", (3, "logit"), (3, "prob"), (3, "prob"), "probs"]
        want = {w: run(plain, w) for w in set(calls)}
        assert same_bits(want[(3, "prob")], prob_records(want["probs"], 3))
        assert not same_bits(want[(3, "prob")], want[(3, "logit")])
        for w in calls:
            assert same_bits(run(graph, w), want[w]), w
    finally:
        B.hip_check(L.vithip_device_sync(), "sync")
        L.vithip_stream_destroy(stream)


@pytest.mark.parametrize("lanes", [1, 2])
def test_profile_accounts_the_launch_to_the_softmax_stage(engines, lanes):
    eng = engines("tiny", max_batch=4, lanes=lanes, profile=True)
    n = 8  # two chunks
    imgs = synth.make_images(eng.cfg, n, 707)

    def launches(fn):
        eng.reset_stage_times()
        fn()
        t = eng.stage_times()
        assert t["images"] == n
        return {s: v["launches"] for s, v in t["stages"].items()}

    probs = launches(lambda: eng.forward(imgs))
    assert probs["softmax"] == 2 * lanes and probs["head"] == 2 * lanes
    for score in ("prob", "logit"):
        assert launches(lambda: eng.topk_host(imgs, 3, score)) == probs, score


def test_invalid_arguments_return_vit_err_arg_and_leave_the_engine_usable(engines):
    L = B.lib()
    eng = engines("tiny", max_batch=4)
    cfg, n = eng.cfg, 3
    imgs = synth.make_images(cfg, n, 708)
    u8 = np.random.default_rng(709).integers(0, 256, size=(n, cfg.img_size, cfg.img_size, cfg.in_chans), dtype=np.uint8)
    ref = eng.topk_host(imgs, 3)
    d_x, d_u8 = B.DeviceArray.from_numpy(imgs), B.DeviceArray.from_numpy(u8)
    d_out = B.DeviceArray((n, 2 * 64), np.int32)
    spec = lambda k, score=0, reserved=0: C.byref(B.CTopkSpec(k, score, reserved))
    mean, std = (C.c_float * 3)(*B.IMAGENET_MEAN), (C.c_float * 3)(*B.IMAGENET_STD)
    zero_std = (C.c_float * 3)(0.229, 0.0, 0.225)

    def refused(rc, needle=()):
        assert rc == VIT_ERR_ARG
        msg = L.vit_engine_last_error(eng._h).decode()
        assert msg and all(word in msg for word in needle), msg
        assert same_bits(eng.topk_host(imgs, 3), ref)

    for d_images, nn, sp, out in [(None, n, spec(3), d_out.ptr), (d_x.ptr, n, spec(3), None), (d_x.ptr, n, None, d_out.ptr),
                                  (d_x.ptr, 0, spec(3), d_out.ptr), (d_x.ptr, -1, spec(3), d_out.ptr), (d_x.ptr, n, spec(3, 2), d_out.ptr),
                                  (d_x.ptr, n, spec(3, -1), d_out.ptr), (d_x.ptr, n, spec(3, 0, 1), d_out.ptr)]:
        refused(L.vit_engine_topk_device(eng._h, d_images, nn, sp, out, None))
    for k in (0, -1, 11, 64, 65):  # 10 classes: k = 11 is already too many
        refused(L.vit_engine_topk_device(eng._h, d_x.ptr, n, spec(k), d_out.ptr, None), (f"k = {k}", "1..10", "VIT_MAX_TOPK", "num_classes"))
        assert L.vit_engine_topk_row_elems(eng._h, spec(k)) == 0
    for d_images, nn, m, s, sp in [(d_u8.ptr, n, None, std, spec(3)), (d_u8.ptr, n, mean, zero_std, spec(3)), (d_u8.ptr + 1, n, mean, std, spec(3)),
                                   (d_u8.ptr, n, mean, std, spec(11)), (d_u8.ptr, 0, mean, std, spec(3))]:
        refused(L.vit_engine_topk_device_u8(eng._h, d_images, nn, m, s, sp, d_out.ptr, None))
    out = np.empty((n, 20), np.int32)
    rows = (B.i32p * n)(*[out[i].ctypes.data_as(B.i32p) for i in range(n)])
    holes = (B.i32p * n)(*[out[i].ctypes.data_as(B.i32p) if i != 1 else None for i in range(n)])
    in_f32 = (B.f32p * n)(*[imgs[i].ctypes.data_as(B.f32p) for i in range(n)])
    in_u8 = (C.c_void_p * n)(*[u8[i].ctypes.data for i in range(n)])
    for ptrs, nn, sp, r in [(None, n, spec(3), rows), (in_f32, n, spec(3), None), (in_f32, 0, spec(3), rows), (in_f32, n, None, rows),
                            (in_f32, n, spec(0), rows), (in_f32, n, spec(3, 5), rows), (in_f32, n, spec(3, 1, -1), rows), (in_f32, n, spec(3), holes)]:
        refused(L.vit_engine_topk_host(eng._h, ptrs, nn, sp, r))
    for ptrs, nn, m, s, sp, r in [(in_u8, n, mean, None, spec(3), rows), (in_u8, n, mean, zero_std, spec(3), rows),
                                  (in_u8, n, mean, std, spec(3, 2), rows), (None, n, mean, std, spec(3), rows)]:
        refused(L.vit_engine_topk_host_u8(eng._h, ptrs, nn, m, s, sp, r))
    S = cfg.img_size
    recs = B.image_records([(d_u8.ptr + i * S * S * 3, S, S) for i in range(n)])
    pp = B.preproc_params(S, *CONSTS, 3)
    small = B.preproc_params(S - 1, *CONSTS, 3)
    for rc_, p, sp in [(recs, None, spec(3)), (recs, C.byref(small), spec(3)), (recs, C.byref(pp), spec(12)), (recs, C.byref(pp), None)]:
        refused(L.vit_engine_topk_device_images(eng._h, rc_, n, p, sp, d_out.ptr, None))
    assert L.vit_engine_topk_row_elems(eng._h, spec(1)) == 2 and L.vit_engine_topk_row_elems(eng._h, spec(10, 1)) == 20
    assert L.vit_engine_topk_row_elems(eng._h, spec(3, 2)) == 0 and L.vit_engine_topk_row_elems(eng._h, spec(3, 0, 7)) == 0
    with pytest.raises(B.VitError):
        eng.topk_shape(n, 11)
    with pytest.raises(B.VitError):
        eng.topk_host(imgs, 3, reserved=1)
    assert same_bits(eng.topk_host(imgs, 3), ref)


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_non_finite_image_gets_empty_slots_and_leaves_the_others_alone(engines, dtype):
    eng = engines("small", max_batch=4, dtype=dtype)
    k = 5
    imgs = synth.make_images(eng.cfg, 3, 710)
    clean = imgs[[0, 2]].copy()
    imgs[1] = np.nan
    for score in ("prob", "logit"):
        got = eng.topk_host(imgs, k, score)
        labels, scores = B.split_topk(got)
        assert (labels[1] == B.TOPK_EMPTY_LABEL).all() and (scores[1] == M.EMPTY_SCORE[score]).all(), score
        assert same_bits(got[[0, 2]], eng.topk_host(clean, k, score)), score
    probs, label, prob = device_forward(eng, B.DeviceArray.from_numpy(imgs), 3)
    got = eng.topk_host(imgs, k)
    assert same_bits(got, prob_records(probs, k))
    assert same_bits(B.split_topk(got)[0][:, 0], label) and same_bits(B.split_topk(got)[1][:, 0], prob)
