"""MI355X-native ViT inference hot path (drop-in for the reference's ViT_opencl path).

The directory name is not a Python identifier; load it with
``importlib.import_module("vision-transformer-opencl_amd")`` (tests/conftest.py and
__graft_entry__.py register it under the alias ``vit_amd``).
"""
from . import dp, launch, synth  # noqa: F401
from .synth import CLIP_B16, CLIP_BIGG14, CLIP_H14, CLIP_L14, DINOV2_B14_REG4, ModelConfig, VIT_B16, VIT_G14, VIT_H14, VIT_L16_384, VIT_SMALL, VIT_TINY  # noqa: F401
