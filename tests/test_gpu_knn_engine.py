"""vit_engine_set_gallery / vit_engine_neighbours_*: an image's records are the k-NN kernel on the SAME engine's feature rows, bit for
bit -- whatever the lanes, the chunking and the path -- and the gallery is state that outlives a weight install.
"""
import numpy as np
import pytest

from engine_helpers import engines, same_bits, weights  # noqa: F401  (fixtures)
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

VIT_ERR_ARG, VIT_ERR_STATE = 1, 5


def gallery_rows(G, dim, seed=41):
    x = np.random.default_rng(seed).standard_normal((G, dim))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("bank", ["f32", "bf16"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_neighbours_are_the_kernel_on_the_engines_own_features(engines, dtype, bank):
    eng = engines("small", max_batch=4, dtype=dtype)
    cfg, n, k = eng.cfg, 7, 5  # two pieces: 4 and 3 images
    imgs = synth.make_images(cfg, n, 801)
    rows = gallery_rows(300, cfg.embed_dim)
    eng.set_gallery(rows, bank)
    kernel_bank = rows if bank == "f32" else B.to_bf16_bits(rows)
    d_x, d_out = B.DeviceArray.from_numpy(imgs), B.DeviceArray((n, 2 * k), np.int32)
    try:
        for lanes in (1, 2):
            eng.set_lanes(lanes)
            for kind in ("cls", "mean"):
                want = B.knn_topk(eng.features(imgs, kind, True), kernel_bank, k)
                assert (B.split_topk(want)[0] != B.TOPK_EMPTY_LABEL).all()
                got = eng.neighbours(imgs, k, kind)
                assert got.dtype == np.int32 and same_bits(got, want), (lanes, kind)
                eng.neighbours_device(d_x.ptr, n, d_out.ptr, k, kind)
                eng.sync()
                assert same_bits(d_out.numpy(), want), (lanes, kind)
    finally:
        eng.set_lanes(1)
        eng.set_gallery(None)


def test_gallery_outlives_an_install_and_the_error_codes(engines, weights):
    eng = engines("small", seed=77, max_batch=4)
    cfg = eng.cfg
    imgs = synth.make_images(cfg, 3, 802)
    rows = gallery_rows(50, cfg.embed_dim)

    def code(call, *a, **kw):
        with pytest.raises(B.VitError) as ei:
            call(*a, **kw)
        return ei.value.code

    assert code(eng.neighbours, imgs, 3) == VIT_ERR_STATE
    eng.set_gallery(rows)
    first = eng.neighbours(imgs, 3)
    eng.load_weights(weights("small", 77))
    assert same_bits(eng.neighbours(imgs, 3), first)
    eng.set_gallery(None)
    assert code(eng.neighbours, imgs, 3) == VIT_ERR_STATE
    eng.set_gallery(rows, "bf16")
    assert same_bits(eng.neighbours(imgs, 3), B.knn_topk(eng.features(imgs, "cls", True), B.to_bf16_bits(rows), 3))
    for bad in (dict(k=0), dict(k=257), dict(k=3, kind="tokens"), dict(k=3, reserved=1), dict(k=3, kind="head"), dict(k=3, kind=3)):
        assert code(eng.neighbours, imgs, **bad) == VIT_ERR_ARG, bad  # "head": 100 classes wide, the gallery 192
    assert code(eng.set_gallery, gallery_rows(5, 12)) == VIT_ERR_ARG  # dim no multiple of 8
    assert same_bits(eng.neighbours(imgs, 60)[:, 50:60], np.full((3, 10), B.TOPK_EMPTY_LABEL, np.int32))  # k > G: empty slots
    eng.set_gallery(None)
