"""The operand table an install resolves (host/vit_engine.c, finish_install): what every GEMM and LayerNorm of the forward reads is
cached per layer when weights are installed, so it has to follow the weights -- whichever route installs them, and every time one does.

Equality is bitwise, engine against engine: no tolerance anywhere.  TINY (D = 128) hands the pruned layer's K/V GEMM the pre-split
image at a panel boundary, SMALL (D = 192) hands it none and it splits on the fly: the two smallest shapes at which that view differs.
"""
import numpy as np
import pytest

from engine_helpers import CONFIGS, same_bits
from vit_amd import binding as B
from vit_amd import synth

pytestmark = pytest.mark.gpu

N = 3  # images per call
_cache = {}


def _weights(name, seed):
    if (name, seed) not in _cache:
        _cache[(name, seed)] = synth.make_weights(CONFIGS[name], seed)
    return _cache[(name, seed)]


def _images(name):
    if name not in _cache:
        _cache[name] = synth.make_images(CONFIGS[name], N, 17)
    return _cache[name]


def _outputs(eng, images):
    return eng.forward(images), eng.features(images, kind="tokens"), eng.cls_attention(images, kind="heads")


ROUTES = {
    "image_with_bf16": lambda e, a, cfg, w: e.load_weight_image(B.WeightImage.build(cfg, w, with_bf16=True)),
    "image_without_bf16": lambda e, a, cfg, w: e.load_weight_image(B.WeightImage.build(cfg, w, with_bf16=False)),
    "copy": lambda e, a, cfg, w: e.copy_weights_from(a),
    "copy_resampled_equal_size": lambda e, a, cfg, w: e.copy_weights_from(a, pos_mode="bicubic"),
    "image_read_back": lambda e, a, cfg, w: e.load_weight_image(a.read_weight_image()),
    "load_resampled_equal_size": lambda e, a, cfg, w: e.load_weights(w, pos_from=cfg.img_size),
}


@pytest.mark.parametrize("prune", [False, True], ids=["full", "pruned"])
@pytest.mark.parametrize("ln_fold", [-1, 0], ids=["nofold", "fold"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ["tiny", "small"])
def test_every_install_route_gives_the_bits_of_load_weights(name, dtype, ln_fold, prune):
    cfg, w, images = CONFIGS[name], _weights(name, 3), _images(name)
    opt = dict(max_batch=4, dtype=dtype, ln_fold=ln_fold, prune_last_layer=prune)
    a = B.Engine(cfg, **opt)
    engines = [a]
    try:
        a.load_weights(w)
        want = _outputs(a, images)
        for route, install in ROUTES.items():
            e = B.Engine(cfg, **opt)
            engines.append(e)
            install(e, a, cfg, w)
            for what, got, ref in zip(("forward", "tokens", "cls_attention"), _outputs(e, images), want):
                assert same_bits(got, ref), f"{route}: {what} differs from the load_weights engine"
    finally:
        for e in engines:
            e.close()


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_a_reinstall_rebuilds_the_table(dtype, use_graph):
    """Seed 1, then seed 2 into the same engine, then seed 1 again by replication: every result is the one of the weights installed
    last.  A graphed engine keeps its images and its output where they are, so that only the install can have dropped the capture."""
    cfg, images = CONFIGS["tiny"], _images("tiny")
    opt = dict(max_batch=4, dtype=dtype, ln_fold=0, prune_last_layer=True, use_graph=use_graph)
    engines = [B.Engine(cfg, **opt) for _ in range(3)]
    eng, fresh2, source1 = engines
    d_images, d_probs = B.DeviceArray.from_numpy(images), B.DeviceArray((N, cfg.num_classes))

    def forward(e):
        if not use_graph:
            return e.forward(images)
        for _ in range(2):  # the second call replays what the first captured
            e.forward_device(d_images.ptr, N, d_probs.ptr)
        e.sync()
        return d_probs.numpy()

    try:
        eng.load_weights(_weights("tiny", 1))
        first = forward(eng)
        eng.load_weights(_weights("tiny", 2))
        second = forward(eng)
        fresh2.load_weights(_weights("tiny", 2))
        assert same_bits(second, forward(fresh2)), "after a second load_weights the engine does not compute with the new weights"
        assert not same_bits(second, first)  # the two seeds are told apart at all
        source1.load_weights(_weights("tiny", 1))
        eng.copy_weights_from(source1)
        assert same_bits(forward(eng), first), "after copy_weights_from the engine does not compute with the source's weights"
    finally:
        for e in engines:
            e.close()
