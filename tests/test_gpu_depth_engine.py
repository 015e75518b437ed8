"""Linear depth heads on the engine (vit_engine_set_depth_head, vit_engine_dense_* with VIT_DENSE_DEPTH), fp32 and bf16 engines.

Model: VIT_TINY at 48 px (g = 3, depth 2); heads of 32 bins, upsample 4, over the last layer and over both.  Parity is against the
upstream-order head in float64 (tests/depth_head_model.py) computed from the rows Engine.intermediate returns for the same layers and
norm, which isolates the head from the encoder's error; the bar is that of tests/test_gpu_depth_kernel.py with the matmul inside the
fp32 restatement.
"""
import dataclasses

import numpy as np
import pytest

import depth_head_model as M
from engine_helpers import same_bits
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

CFG = dataclasses.replace(synth.VIT_TINY, img_size=48)
G, D, BINS, U = 3, CFG.embed_dim, 32, 4
MIN_DEPTH, MAX_DEPTH = 0.001, 10.0
ERR_STATE = 5


def head(layers, class_token):
    C = len(layers) * (2 if class_token else 1) * D
    rng = np.random.default_rng(C)
    return (3 * rng.standard_normal((BINS, C)) / np.sqrt(C)).astype(np.float32), rng.standard_normal(BINS).astype(np.float32)


@pytest.fixture(scope="module")
def engines():
    cache, W = {}, synth.make_weights(CFG, 41)

    def get(dtype):
        if dtype not in cache:
            cache[dtype] = B.Engine(CFG, dtype=dtype, max_batch=4)
            cache[dtype].load_weights(W)
        cache[dtype].reset_depth_head()
        cache[dtype].reset_dense_head()
        return cache[dtype]

    get.weights = W
    yield get
    for eng in cache.values():
        eng.close()


@pytest.mark.parametrize("dtype,layers,class_token,norm", [("f32", (1,), 1, 0), ("f32", (0, 1), 1, 1), ("f32", (0, 1), 0, 1), ("bf16", (1,), 0, 0),
                                                           ("bf16", (0, 1), 1, 1), ("bf16", (1,), 1, 1)])
def test_depth_rows_match_the_float64_head_on_the_tapped_rows(engines, dtype, layers, class_token, norm):
    eng = engines(dtype)
    w, b = head(layers, class_token)
    eng.set_depth_head(w, b, layers, norm, U, class_token, MIN_DEPTH, MAX_DEPTH)
    imgs = synth.make_images(CFG, 7, 600)  # a full chunk and a ragged one
    rows = [eng.intermediate(imgs, list(layers), "patches", norm).reshape(7, len(layers), G * G, D)]
    if class_token:
        rows.append(np.broadcast_to(eng.intermediate(imgs, list(layers), "cls", norm).reshape(7, len(layers), 1, D), rows[0].shape))
    feats = np.concatenate(rows, axis=3).transpose(0, 2, 1, 3).reshape(7, G * G, -1)  # per layer [patch | class], as the weight's columns
    cell64 = feats.astype(np.float64) @ w.astype(np.float64).T + b.astype(np.float64)
    cell32 = feats @ w.T + b
    centres = np.linspace(MIN_DEPTH, MAX_DEPTH, BINS).astype(np.float32)
    for size in (None, (37, 53)):
        out = size or (CFG.img_size, CFG.img_size)
        got = eng.dense(imgs, "depth", size)
        assert got.shape == (7,) + out and got.dtype == np.float32 and eng.dense_row_bytes("depth", size) == out[0] * out[1] * 4
        ref = M.reference64(cell64, centres, G, U, out, MIN_DEPTH, MAX_DEPTH)
        e32, bar = M.bar(ref, cell32, centres, G, U, out, MIN_DEPTH, MAX_DEPTH)
        err = float(np.abs(got.astype(np.float64) - ref).max())
        print(f"{dtype} layers={layers} cls={class_token} norm={norm} out={out}: max |got - ref| = {err:.3e}, E32 = {e32:.3e}, bar = {bar:.3e}")
        assert err <= bar and np.ptp(got) > 0.01, (err, e32, bar)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_the_depth_head_is_state_of_its_own(engines, dtype):
    eng = engines(dtype)
    imgs = synth.make_images(CFG, 6, 601)
    with pytest.raises(B.VitError) as err:  # no depth head yet; a dense head does not stand in for it
        eng.dense(imgs, "depth")
    assert err.value.code == ERR_STATE and eng.dense_row_bytes("depth") == 0
    rng = np.random.default_rng(3)
    dw, db = rng.standard_normal((21, 2 * D)).astype(np.float32), rng.standard_normal(21).astype(np.float32)
    eng.set_dense_head(dw, db, (0, 1), 1)
    with pytest.raises(B.VitError) as err:
        eng.dense(imgs, "depth")
    assert err.value.code == ERR_STATE
    labels, grid = eng.dense(imgs, "labels", (37, 53)), eng.dense(imgs, "grid")
    w, b = head((0, 1), 1)
    eng.set_depth_head(w, b, (0, 1), 1, U, 1, MIN_DEPTH, MAX_DEPTH)
    depth = eng.dense(imgs, "depth", (37, 53))
    assert same_bits(eng.dense(imgs, "labels", (37, 53)), labels) and same_bits(eng.dense(imgs, "grid"), grid)
    eng.reset_dense_head()  # and the reverse: the depth rows do not look at the dense head
    assert same_bits(eng.dense(imgs, "depth", (37, 53)), depth)
    with pytest.raises(B.VitError) as err:
        eng.dense(imgs, "labels")
    assert err.value.code == ERR_STATE
    # host and device calls give the same bits
    d_x, d_out = B.DeviceArray.from_numpy(imgs), B.DeviceArray((6, 37, 53))
    eng.dense_device(d_x.ptr, 6, d_out.ptr, "depth", (37, 53))
    eng.sync()
    assert same_bits(d_out.numpy(), depth)
    # a non-finite image reaches only its own row
    bad = imgs.copy()
    bad[2, 1, 5:9, 3] = np.nan
    got = eng.dense(bad, "depth", (37, 53))
    assert same_bits(got[[0, 1, 3, 4, 5]], depth[[0, 1, 3, 4, 5]]) and np.isnan(got[2]).any()
    # other centres are other depths; removing the head and every weight install leave none behind
    eng.set_depth_head(w, b, (0, 1), 1, U, 1, MIN_DEPTH, MAX_DEPTH, centres=np.geomspace(MIN_DEPTH, MAX_DEPTH, BINS))
    assert not same_bits(eng.dense(imgs, "depth", (37, 53)), depth)
    eng.load_weights(engines.weights)
    with pytest.raises(B.VitError) as err:
        eng.dense(imgs, "depth")
    assert err.value.code == ERR_STATE
