"""The 8-bit input's arithmetic on the host (no GPU): the numpy restatement that tests/test_gpu_input_u8.py compares the device
against, checked bit for bit against torchvision's two ops as torch computes them on the CPU, and the C-ABI symbols of the feature.

torchvision's ToTensor() is img.float().div(255) on the HWC -> CHW permuted bytes, Normalize(mean, std) is
sub_(mean[:, None, None]).div_(std[:, None, None]); torchvision itself is not needed to state that.
"""
import os
import subprocess

import numpy as np
import pytest

from vit_amd import binding as B

CONSTANTS = [
    (B.IMAGENET_MEAN, B.IMAGENET_STD),
    ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5)),
    ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
    ((0.1234567, -0.75, 3.0), (0.0171, -0.3, 7.5)),   # a negative std too
    ((-1e-3, 0.999, 0.25), (-2.5, 1e-3, 0.333)),
]


def normalise_u8(images: np.ndarray, mean, std) -> np.ndarray:
    """uint8 [n][S][S][C] -> fp32 [n][C][S][S]: ((float)u / 255 - mean[c]) / std[c], every step one fp32 operation."""
    x = np.ascontiguousarray(np.moveaxis(np.asarray(images, np.uint8), -1, 1)).astype(np.float32)
    m = np.asarray(mean, np.float32)[None, :, None, None]
    s = np.asarray(std, np.float32)[None, :, None, None]
    return (x / np.float32(255.0) - m) / s


def torch_reference(images: np.ndarray, mean, std) -> np.ndarray:
    torch = pytest.importorskip("torch")
    t = torch.from_numpy(np.ascontiguousarray(images)).permute(0, 3, 1, 2).contiguous()
    m = torch.tensor(mean, dtype=torch.float32)[:, None, None]
    s = torch.tensor(std, dtype=torch.float32)[:, None, None]
    return t.float().div(255).sub(m).div(s).numpy()


@pytest.mark.parametrize("mean,std", CONSTANTS)
def test_restatement_equals_torch_on_every_byte_value(mean, std):
    every = np.arange(256, dtype=np.uint8)
    imgs = np.stack([np.roll(every, 85 * c) for c in range(3)], axis=-1).reshape(1, 16, 16, 3)  # every value in every channel
    got, ref = normalise_u8(imgs, mean, std), torch_reference(imgs, mean, std)
    assert got.dtype == np.float32 and got.shape == (1, 3, 16, 16)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_restatement_equals_torch_on_random_images():
    rng = np.random.default_rng(5)
    imgs = rng.integers(0, 256, size=(3, 32, 32, 3), dtype=np.uint8)
    for mean, std in CONSTANTS:
        assert np.array_equal(normalise_u8(imgs, mean, std).view(np.uint32), torch_reference(imgs, mean, std).view(np.uint32))


def test_restatement_is_not_a_reciprocal_multiply():
    """The comparison must be able to fail: u * (1 / 255) instead of u / 255 differs in some bits."""
    u = np.arange(256, dtype=np.float32)
    assert not np.array_equal(u / np.float32(255.0), u * (np.float32(1.0) / np.float32(255.0)))


def test_imagenet_constants_are_torchvisions():
    assert B.IMAGENET_MEAN == (0.485, 0.456, 0.406)
    assert B.IMAGENET_STD == (0.229, 0.224, 0.225)


def test_product_library_exports_the_u8_entry_points():
    product = os.path.join(os.path.dirname(B.LIB_PATH), "libvit_mi355x.so")
    syms = subprocess.run(["nm", "-D", "--defined-only", product], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in syms.splitlines() if ln.strip()}
    assert {"vithip_images_u8_to_f32", "vit_engine_forward_device_u8", "vit_engine_forward_host_u8"} <= names
    L = B.lib()
    for fn in ("vithip_images_u8_to_f32", "vit_engine_forward_device_u8", "vit_engine_forward_host_u8"):
        assert getattr(L, fn).argtypes, fn
