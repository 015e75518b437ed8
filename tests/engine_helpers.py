"""What the engine's GPU test modules share: bitwise comparison, the engine and weight caches, device calls read back.

A plain module, imported by name.  A test module that imports the `weights` and `engines` fixtures gets its own module-scoped
instances of them, as if it had defined them itself.
"""
import ctypes as C

import numpy as np
import pytest

from vit_amd import binding as B
from vit_amd import synth

CONFIGS = {"tiny": synth.VIT_TINY, "small": synth.VIT_SMALL, "b16": synth.VIT_B16}
CONSTS = (B.IMAGENET_MEAN, B.IMAGENET_STD)


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def cfloats(v):
    return (C.c_float * len(v))(*v)


@pytest.fixture(scope="module")
def weights():
    cache = {}

    def get(name, seed):
        if (name, seed) not in cache:
            cache[(name, seed)] = synth.make_weights(CONFIGS[name], seed)
        return cache[(name, seed)]

    return get


@pytest.fixture(scope="module")
def engines(weights):
    """Engines by (config name, weight seed, options), created on first use."""
    cache = {}

    def get(name, seed=1234, **opt):
        key = (name, seed, tuple(sorted(opt.items())))
        if key not in cache:
            eng = B.Engine(CONFIGS[name], **opt)
            eng.load_weights(weights(name, seed))
            cache[key] = eng
        return cache[key]

    yield get
    for eng in cache.values():
        eng.close()


def read_back(eng, d_out, shape) -> np.ndarray:
    """The fp32 rows a device call of `eng` wrote to d_out, once everything on the device has finished."""
    eng.sync()
    got = np.empty(shape, np.float32)
    B.hip_check(B.lib().vithip_device_sync(), "sync")
    B.hip_check(B.lib().vithip_memcpy_d2h(got.ctypes.data, d_out.ptr, got.nbytes, None), "d2h")
    B.hip_check(B.lib().vithip_device_sync(), "sync")
    return got


def device_forward(eng, d_images, n, u8_consts=None, stream=0):
    """(probs, top-1 labels, top-1 probs) of one forward_device / forward_device_u8 call on device images d_images."""
    NC = eng.cfg.num_classes
    d_p, d_l, d_q = B.DeviceArray((n, NC)), B.DeviceArray((n,), np.int32), B.DeviceArray((n,))
    if u8_consts is None:
        eng.forward_device(d_images.ptr, n, d_p.ptr, d_l.ptr, d_q.ptr, stream)
    else:
        eng.forward_device_u8(d_images.ptr, n, d_p.ptr, u8_consts[0], u8_consts[1], d_l.ptr, d_q.ptr, stream)
    eng.sync()
    return d_p.numpy(), d_l.numpy(), d_q.numpy()


def device_features(eng, d_images, n, kind, l2=False, u8=False, stream=0, d_out=None):
    d_out = d_out or B.DeviceArray(eng.feature_shape(n, kind, l2))
    if u8:
        eng.features_device_u8(d_images.ptr, n, d_out.ptr, kind, l2, *CONSTS, stream=stream)
    else:
        eng.features_device(d_images.ptr, n, d_out.ptr, kind, l2, stream=stream)
    return read_back(eng, d_out, eng.feature_shape(n, kind, l2))


def device_attention(eng, d_images, n, kind, u8=False, stream=0, d_out=None):
    d_out = d_out or B.DeviceArray(eng.attention_shape(n, kind))
    if u8:
        eng.cls_attention_device_u8(d_images.ptr, n, d_out.ptr, kind, *CONSTS, stream=stream)
    else:
        eng.cls_attention_device(d_images.ptr, n, d_out.ptr, kind, stream=stream)
    return read_back(eng, d_out, eng.attention_shape(n, kind))
