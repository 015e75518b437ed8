"""The general fp32 patch embedding (vithip_patch_embed_f32_general, csrc/vit_patch_embed_general.hip): any even patch and image size.

Against the oracle's embed (conv_proj -> flatten_transpose -> class_token -> pos_emb of ViT_seq.c) at REL = 2e-5 of the tensor's
magnitude, the bar of test_patch_embed in tests/test_gpu_ops.py; the class row bit-equal to cls + pos[0]; an image's rows bit-equal
wherever the image sits in whatever batch; the write footprint exactly [n][T][D]; nothing read outside the images and conv_w (their
surroundings hold NaN: a tail that multiplied out-of-range data by zero would give NaN); refusals launch nothing.
"""
import numpy as np
import pytest

import strided
from conftest import oracle_config
from engine_helpers import same_bits
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

REL = 2e-5
INVALID = 1  # hipErrorInvalidValue

# (img, patch, chans, D, n)
GEOMETRIES = [
    (28, 14, 3, 64, 5),     # the smallest patch-14 case
    (42, 14, 3, 192, 15),   # 135 patch rows: a 128-row tile straddles images and has a tail; D is no multiple of 128 (nor of 64)
    (4, 2, 1, 64, 3),       # K = 4, below any K step
    (12, 6, 1, 64, 5),      # K = 36
    (18, 6, 3, 64, 7),      # K = 108, img % 4 == 2
    (30, 10, 3, 64, 5),     # K = 300
    (42, 14, 1, 64, 3),     # K = 196
    (32, 16, 3, 128, 3),    # the 16-byte kernel takes it too
    (48, 12, 2, 64, 5),     # the 16-byte kernel takes it too
    (224, 14, 3, 768, 2),   # the real shape: DINOv2 ViT-B/14 at 224
]
SHARED = {(32, 16, 3, 128, 3), (48, 12, 2, 64, 5)}
_cache = {}


def config(img, patch, chans, dim):
    return synth.ModelConfig(img_size=img, patch_size=patch, in_chans=chans, num_classes=10, embed_dim=dim, depth=1,
                             num_heads=dim // 64, hidden_dim=dim)


def operands(cfg, n, seed=5):
    """(images [n][C][S][S], [cls, conv_w, conv_b, pos]), made once per geometry."""
    key = (cfg, n, seed)
    if key not in _cache:
        W = [synth.make_weight(cfg, i, seed) for i in range(4)]
        _cache[key] = (synth.make_images(cfg, n, seed + 1), W)
    return _cache[key]


def oracle_embed(oracle, cfg, imgs, W):
    key = ("ref", cfg, imgs.shape[0], imgs[0, 0, 0, :2].tobytes())
    if key not in _cache:
        ocfg = oracle_config(cfg)
        _cache[key] = np.stack([oracle.embed(ocfg, im, W) for im in imgs])
    return _cache[key]


def worst_rel(got, ref):
    """max over the images of max |d| / max |ref|, as test_patch_embed's close() takes it image by image."""
    return max(float(np.abs(g.astype(np.float64) - r.astype(np.float64)).max()) / (float(np.abs(r).max()) + 1e-30) for g, r in zip(got, ref))


@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda g: "img%d-p%d-c%d-d%d-n%d" % g)
def test_general_kernel_matches_the_oracle(oracle, geom):
    img, patch, chans, dim, n = geom
    cfg = config(img, patch, chans, dim)
    imgs, W = operands(cfg, n)
    got = B.patch_embed_general(cfg, imgs, W[1], W[2], W[0], W[3])
    assert got.shape == (n, cfg.tokens, dim) and np.isfinite(got).all()
    err = worst_rel(got, oracle_embed(oracle, cfg, imgs, W))
    print(f"general embed {geom}: K = {cfg.patch_dim}, max |d| / max |ref| = {err:.3e}")
    assert err <= REL, (geom, err)
    cls_row = (W[0] + W[3].reshape(cfg.tokens, dim)[0]).astype(np.float32)
    for i in range(n):
        assert same_bits(got[i, 0], cls_row), i
    if geom in SHARED:  # recorded in profiles/r14/README.md; equality is not required (the 16-byte kernel's k order inside a K step is another)
        old = B.patch_embed(cfg, imgs, W[1], W[2], W[0], W[3])
        print(f"general embed {geom}: bits equal to vithip_patch_embed_f32's: {same_bits(got, old)}, "
              f"max |d| = {float(np.abs(got - old).max()):.3e}")
        assert worst_rel(old, oracle_embed(oracle, cfg, imgs, W)) <= REL


@pytest.mark.parametrize("geom", [(42, 14, 3, 192, 15), (18, 6, 3, 64, 7)], ids=lambda g: "img%d-p%d" % g[:2])
def test_dispatcher_sends_new_geometries_to_the_general_kernel(geom):
    """vithip_patch_embed_f32 at a geometry its 16-byte kernel refuses gives the general kernel's bits."""
    img, patch, chans, dim, n = geom
    cfg = config(img, patch, chans, dim)
    imgs, W = operands(cfg, n)
    assert same_bits(B.patch_embed(cfg, imgs, W[1], W[2], W[0], W[3]), B.patch_embed_general(cfg, imgs, W[1], W[2], W[0], W[3]))


def test_rows_do_not_depend_on_the_batch_or_the_place_in_it():
    cfg = config(42, 14, 3, 192)
    n = 15
    imgs, W = operands(cfg, n)
    batch = imgs.copy()
    for pos in (0, 7, 14):  # one image at three places among distinct others: tile 0 from its first row, astride tiles, in the tail tile
        batch[pos] = imgs[3]
    got = B.patch_embed_general(cfg, batch, W[1], W[2], W[0], W[3])
    alone = B.patch_embed_general(cfg, imgs[3:4], W[1], W[2], W[0], W[3])
    assert alone.shape == (1, 10, 192)
    for pos in (0, 7, 14):
        assert same_bits(got[pos], alone[0]), pos
    assert not same_bits(got[1], alone[0])


def test_write_footprint_is_the_token_rows_and_reads_stay_inside_the_operands(oracle):
    """x: a frame of sentinel bits with guard rows either side -- every element of [n][T][D] is written, nothing else changes.
    images and conv_w: windows of larger allocations whose surroundings are NaN, two floats into them (8-byte aligned only); bias,
    cls and pos the same.  A K tail, M tail or N tail that read past an operand, even multiplied by zero, would leave a NaN."""
    img, patch, chans, dim, n = 42, 14, 3, 192, 15
    cfg = config(img, patch, chans, dim)
    imgs, W = operands(cfg, n)
    f_img = strided.framed(imgs.reshape(n, -1), offset=2)
    f_w = strided.framed(W[1].reshape(dim, -1), offset=2)
    f_b, f_cls, f_pos = strided.framed(W[2]), strided.framed(W[0]), strided.framed(W[3].reshape(cfg.tokens, dim))
    f_x = strided.out_frame(n * cfg.tokens, dim)
    assert f_img.ptr % 16 == 8 and f_w.ptr % 16 == 8
    rc = B.patch_embed_general_raw(f_img.ptr, f_w.ptr, f_b.ptr, f_cls.ptr, f_pos.ptr, f_x.ptr, n, img, patch, chans, dim)
    assert rc == 0
    got = f_x.check().reshape(n, cfg.tokens, dim)  # untouched outside, no sentinel and no NaN inside
    for f in (f_img, f_w, f_b, f_cls, f_pos):
        f.assert_untouched()
    assert worst_rel(got, oracle_embed(oracle, cfg, imgs, W)) <= REL
    assert same_bits(got, B.patch_embed_general(cfg, imgs, W[1], W[2], W[0], W[3]))


def test_refused_geometries_and_null_pointers_launch_nothing():
    floats = 64 * 588 + 64  # the valid call at the end: conv_w [64][588]
    d = [B.DeviceArray.from_numpy(np.zeros(floats, np.float32)) for _ in range(5)]  # images, conv_w, conv_b, cls, pos: room for every case
    pattern = np.full(floats, 0x7FC0DEAD, np.uint32)
    dx = B.DeviceArray.from_numpy(pattern.view(np.float32))

    def call(ptrs=None, null_x=False, n=2, img=28, patch=14, chans=3, dim=64, general=True):
        p = [a.ptr for a in d] if ptrs is None else ptrs
        return B.patch_embed_general_raw(p[0], p[1], p[2], p[3], p[4], None if null_x else dx.ptr, n, img, patch, chans, dim, general)

    cases = {"odd patch": dict(img=28, patch=7), "odd patch and image": dict(img=21, patch=7), "odd image": dict(img=15, patch=2),
             "img % patch": dict(img=30, patch=14), "patch 0": dict(patch=0), "patch > img": dict(img=14, patch=28),
             "dim % 4": dict(dim=66), "dim 0": dict(dim=0), "chans 0": dict(chans=0), "n 0": dict(n=0), "null x": dict(null_x=True)}
    for k in range(5):
        ptrs = [a.ptr for a in d]
        ptrs[k] = None
        cases[f"null operand {k}"] = dict(ptrs=ptrs)
    cases["misaligned images"] = dict(ptrs=[d[0].ptr + 4] + [a.ptr for a in d[1:]])
    cases["misaligned conv_w"] = dict(ptrs=[d[0].ptr, d[1].ptr + 4] + [a.ptr for a in d[2:]])
    for name, kw in cases.items():
        assert call(**kw) == INVALID, name
        assert (dx.numpy().view(np.uint32) == pattern).all(), name  # nothing was launched
    # the dispatcher refuses the same: an odd patch or image goes to the general kernel's checks
    for kw in (dict(img=28, patch=7), dict(img=21, patch=7), dict(img=30, patch=14), dict(dim=66)):
        assert call(general=False, **kw) == INVALID, kw
        assert (dx.numpy().view(np.uint32) == pattern).all(), kw
    assert call() == 0  # and a valid call behind the refusals runs
    got = dx.numpy()[:2 * 5 * 64]
    assert np.isfinite(got).all() and (got == 0).all()  # zero operands: cls + pos = 0, bias + 0 . 0 + pos = 0
