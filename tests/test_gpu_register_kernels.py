"""The kernels of register-token models: the three patch embeddings with a prefix of 1 + R rows (vithip_patch_embed_f32_reg, the
general kernel, the bf16 patch-row GEMM) and the tap with its patch rows behind `prefix` (vithip_tap_f32_prefix_eps).

Embedding: against tests/register_model.embed in float64 with the op bar of tests/test_gpu_ops.py (REL = 2e-5 of max |ref|; bf16: on
the bf16-rounded pixels and weights, 2e-5 * max(1, max |ref|), the bar of tests/test_gpu_bf16.py); register rows, the class row and
the patch rows are compared bit for bit with prefix, prefix[0] + pos[0] and the entry without registers on the same operands.
Tap: bit for bit against the entry without a prefix, vithip_layernorm_f32 and its own PATCHES layout.
"""
import numpy as np
import pytest

import register_model
from engine_helpers import same_bits
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

REL = 2e-5
D = 128
SENTINEL = np.float32(-7.25)
GUARD = 256


def model(patch, img, R):
    return synth.ModelConfig(img_size=img, patch_size=patch, num_classes=10, embed_dim=D, depth=1, num_heads=2, hidden_dim=256,
                             num_register_tokens=R)


def operands(cfg, n):
    W = [synth.make_weight(cfg, i, 5) for i in range(4)]
    imgs = synth.make_images(cfg, n, 6)
    return W, imgs


def plain_entry(kind, cfg0, imgs, W0):
    """The entry without registers on the same operands (class token = prefix row 0)."""
    fn = {"f32": B.patch_embed, "general": B.patch_embed_general, "bf16": B.patch_embed_bf16}[kind]
    return fn(cfg0, imgs, W0[1], W0[2], W0[0], W0[3])


# patch, image, n, the kernels that geometry reaches: "f32" is the dispatching entry (the 16-byte gather at patch 16, the general
# kernel at patch 14), "general" the general kernel by name, "bf16" the patch-row GEMM
SHAPES = [(16, 32, 3, ("f32", "bf16")),        # P = 4
          (14, 28, 3, ("f32", "general")),     # P = 4
          (14, 42, 3, ("f32", "general")),     # P = 9, img % 4 == 2
          (14, 84, 5, ("f32", "general")),     # P = 36, 180 rows: a 128-row tile spans images
          (16, 96, 5, ("f32", "general", "bf16"))]  # the same for the gather and the bf16 GEMM (and the general kernel off patch 14)


@pytest.mark.parametrize("R", [1, 4])
@pytest.mark.parametrize("patch,img,n,kinds", SHAPES, ids=[f"p{s[0]}-s{s[1]}-n{s[2]}" for s in SHAPES])
def test_embeddings_put_the_prefix_rows_in_front_and_keep_the_patch_rows_bits(patch, img, n, kinds, R):
    cfg, cfg0 = model(patch, img, R), model(patch, img, 0)
    W, imgs = operands(cfg, n)
    assert W[0].shape == (1 + R, D) and W[3].shape == (cfg.patches + 1, D)
    W0 = [W[0][0].copy()] + W[1:]
    T, P = cfg.tokens, cfg.patches
    assert T == 1 + R + P
    for kind in kinds:
        x, front, back = B.patch_embed_reg(cfg, imgs, W[1], W[2], W[0], W[3], kind=kind, guard=GUARD, fill=SENTINEL)
        assert x.shape == (n, T, D) and np.isfinite(x).all()
        assert (front == SENTINEL).all() and (back == SENTINEL).all(), kind  # nothing outside x[n][T][D]
        # float64
        if kind == "bf16":
            Wr = [W[0], B.from_bf16_bits(B.to_bf16_bits(W[1])).reshape(W[1].shape), W[2], W[3]]
            ir = B.from_bf16_bits(B.to_bf16_bits(imgs)).reshape(imgs.shape)
            ref = np.stack([register_model.embed(cfg, im, Wr) for im in ir])
            bar = REL * max(1.0, float(np.abs(ref).max()))
        else:
            ref = np.stack([register_model.embed(cfg, im, W) for im in imgs])
            bar = REL * float(np.abs(ref).max())
        err = float(np.abs(x - ref).max())
        print(f"embed {kind} patch {patch} img {img} n {n} R {R}: max err {err:.3e} (bar {bar:.3e})")
        assert err <= bar, (kind, err, bar)
        # bits
        for i in range(n):
            assert same_bits(x[i, 1:1 + R], W[0][1:]), (kind, i)          # register rows: prefix[1 + r], no position embedding
            assert same_bits(x[i, 0], W[0][0] + W[3][0]), (kind, i)      # the class row
        old = plain_entry(kind, cfg0, imgs, W0)
        assert old.shape == (n, 1 + P, D)
        assert same_bits(x[:, 1 + R:], old[:, 1:]) and same_bits(x[:, 0], old[:, 0]), kind
        # the _reg entry at zero registers is the entry without
        assert same_bits(B.patch_embed_reg(cfg0, imgs, W[1], W[2], W0[0], W[3], kind=kind), old), kind
        # an image's rows do not depend on the batch or on its place in it
        if n == 5:
            moved = B.patch_embed_reg(cfg, imgs[[1, 2, 3, 4, 0]], W[1], W[2], W[0], W[3], kind=kind)
            assert same_bits(moved[4], x[0]) and same_bits(moved[0], x[1]), kind
            assert same_bits(B.patch_embed_reg(cfg, imgs[:1], W[1], W[2], W[0], W[3], kind=kind)[0], x[0]), kind


def test_embeddings_refuse_register_counts_off_the_range_and_write_nothing():
    cfg = model(14, 28, 4)
    W, imgs = operands(cfg, 2)
    for kind in ("f32", "general"):
        for R in (-1, 17):
            with pytest.raises(B.VitError) as err:
                B.patch_embed_reg(cfg, imgs, W[1], W[2], np.zeros((18, D), np.float32), W[3], kind=kind, registers=R)
            assert err.value.code == 1, (kind, R)
    cfg16 = model(16, 32, 4)
    W, imgs = operands(cfg16, 2)
    with pytest.raises(B.VitError) as err:
        B.patch_embed_reg(cfg16, imgs, W[1], W[2], np.zeros((18, D), np.float32), W[3], kind="bf16", registers=17)
    assert err.value.code == 1


# ---- tap ---------------------------------------------------------------------------------------------------------------------------

LAYOUTS = ("cls", "tokens", "patches", "map")


def tap_operands(tokens, dim, images=3, seed=11):
    rng = np.random.default_rng(seed + tokens * 7 + dim)
    x = rng.normal(0, 1, (images * tokens, dim)).astype(np.float32)
    g = rng.uniform(0.5, 1.5, dim).astype(np.float32)
    b = rng.uniform(-0.5, 0.5, dim).astype(np.float32)
    return x, g, b


@pytest.mark.parametrize("dim", [128, 768, 2048])
@pytest.mark.parametrize("P", [1, 4, 9, 16, 196])
def test_tap_with_a_prefix_reads_the_patch_rows_behind_it(P, dim):
    images = 3
    for prefix in (1, 5):
        tokens = prefix + P
        x, g, b = tap_operands(tokens, dim, images)
        rows = x.reshape(images, tokens, dim)
        normed = B.layernorm(x, g, b).reshape(images, tokens, dim)
        for norm in (False, True):
            gb = (g, b) if norm else (None, None)
            src = normed if norm else rows
            got = {lay: B.tap(x, *gb, images, tokens, lay, prefix=prefix) for lay in LAYOUTS}
            assert got["cls"].shape == (images, dim) and got["tokens"].shape == (images, tokens, dim)
            assert got["patches"].shape == (images, P, dim) and got["map"].shape == (images, dim, P)
            # the bits of vithip_layernorm_f32 on the same rows (or of x): CLS row 0, TOKENS every row, PATCHES rows prefix..
            assert same_bits(got["cls"], src[:, 0]) and same_bits(got["tokens"], src), (prefix, norm)
            assert same_bits(got["patches"], src[:, prefix:]), (prefix, norm)
            assert same_bits(got["map"], np.ascontiguousarray(got["patches"].transpose(0, 2, 1))), (prefix, norm)  # the exact transpose
            if prefix == 1:  # the bits of the entry without a prefix
                for lay in LAYOUTS:
                    assert same_bits(got[lay], B.tap(x, *gb, images, tokens, lay)), (lay, norm)


@pytest.mark.parametrize("P,dim", [(4, 128), (9, 768), (196, 128), (16, 2048)])
def test_tap_with_a_prefix_writes_its_block_only(P, dim):
    images, prefix = 3, 5
    tokens = prefix + P
    x, g, b = tap_operands(tokens, dim, images)
    for lay in LAYOUTS:
        block = {"cls": dim, "tokens": tokens * dim, "patches": P * dim, "map": P * dim}[lay]
        stride = block + 64
        raw = np.full(GUARD + images * stride + GUARD, SENTINEL, np.float32)
        d = B.DeviceArray.from_numpy(raw)
        B.tap(x, g, b, images, tokens, lay, prefix=prefix, d_out=d.ptr + 4 * GUARD, out_image_stride=stride)
        back = d.numpy()
        assert (back[:GUARD] == SENTINEL).all() and (back[-GUARD:] == SENTINEL).all(), lay
        body = back[GUARD:-GUARD].reshape(images, stride)
        assert (body[:, block:] == SENTINEL).all(), lay  # the floats between the blocks are not touched
        want = B.tap(x, g, b, images, tokens, lay, prefix=prefix).reshape(images, block)
        assert same_bits(body[:, :block], want), lay


@pytest.mark.parametrize("P,dim", [(4, 128), (9, 128), (196, 768)])
def test_a_nan_in_a_register_row_reaches_no_patch_output(P, dim):
    images, prefix = 3, 5
    tokens = prefix + P
    x, g, b = tap_operands(tokens, dim, images)
    dirty = x.copy().reshape(images, tokens, dim)
    dirty[1, 2, 7] = np.nan      # a register row of image 1
    dirty[2, 4, :] = np.inf      # the last register row of image 2: the row next to the first patch row
    dirty = dirty.reshape(images * tokens, dim)
    for norm in (False, True):
        gb = (g, b) if norm else (None, None)
        for lay in ("patches", "map"):
            got = B.tap(dirty, *gb, images, tokens, lay, prefix=prefix)
            assert np.isfinite(got).all(), (lay, norm)
            assert same_bits(got, B.tap(x, *gb, images, tokens, lay, prefix=prefix)), (lay, norm)
        tok = B.tap(dirty, *gb, images, tokens, "tokens", prefix=prefix)
        clean = B.tap(x, *gb, images, tokens, "tokens", prefix=prefix)
        assert not np.isfinite(tok[1, 2]).all() and not np.isfinite(tok[2, 4]).all()  # TOKENS does return the register rows
        keep = np.ones((images, tokens), bool)
        keep[1, 2] = keep[2, 4] = False
        assert same_bits(tok[keep], clean[keep]), norm


def test_tap_refuses_a_prefix_off_the_range_and_leaves_the_buffer_untouched():
    images, tokens, dim = 2, 9, 128
    x, g, b = tap_operands(tokens, dim, images)
    cases = [(0, lay) for lay in LAYOUTS] + [(-1, "tokens"), (tokens + 1, "cls"), (tokens + 1, "tokens"), (tokens, "patches"), (tokens, "map")]
    for prefix, lay in cases:
        raw = np.full(images * tokens * dim, SENTINEL, np.float32)
        d = B.DeviceArray.from_numpy(raw)
        with pytest.raises(B.VitError) as err:
            B.tap(x, g, b, images, tokens, lay, prefix=prefix, d_out=d.ptr, out_image_stride=tokens * dim)
        assert err.value.code == 1, (prefix, lay)
        assert (d.numpy() == SENTINEL).all(), (prefix, lay)
    # prefix == tokens is a model without patches: CLS and TOKENS still have their rows
    assert same_bits(B.tap(x, g, b, images, tokens, "tokens", prefix=tokens), B.tap(x, g, b, images, tokens, "tokens"))
    assert same_bits(B.tap(x, g, b, images, tokens, "cls", prefix=tokens), B.tap(x, g, b, images, tokens, "cls"))
