"""ctypes binding of libvit_mi355x.so -- the C-ABI library is the product, this is plumbing.

Everything numeric goes through the shared library (HIP kernels on gfx950).  There is no Python
or CPU fallback: if the library has not been built, loading fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np

from .synth import MLP_CODES, MLP_SHIFT, REG_SHIFT, ModelConfig

HERE = os.path.dirname(os.path.abspath(__file__))
# VIT_HIP_LIBRARY: the probe build (make probes -> libvit_mi355x_probe.so) for the tools/ scripts; default = the product
LIB_PATH = os.environ.get("VIT_HIP_LIBRARY") or os.path.join(HERE, "libvit_mi355x.so")

f32p = C.POINTER(C.c_float)
i32p = C.POINTER(C.c_int)

STAGES = ("embed", "ln", "qkv", "attn", "outproj", "fc1", "fc2", "head", "softmax")
# torchvision's ImageNet normalisation (transforms.Normalize(mean, std) of its vit_b_16 weights), for the 8-bit input
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RESIDUAL = 0, 1, 2
EPI_BIAS_QGELU = 6  # VITHIP_EPI_BIAS_QGELU (3, 4, 5 and 7 are the library's own fold forms)
ARITH_F32, ARITH_SPLIT3 = 0, 1   # vithip_gemm_args.arith


class VitError(RuntimeError):
    pass


class CConfig(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("img_size", "patch_size", "in_chans", "num_classes",
                                       "embed_dim", "depth", "num_heads", "hidden_dim")]

    @classmethod
    def of(cls, cfg: ModelConfig) -> "CConfig":
        return cls(cfg.img_size, cfg.patch_size | (cfg.num_register_tokens << REG_SHIFT), cfg.in_chans, cfg.num_classes, cfg.embed_dim,
                   cfg.depth, cfg.num_heads, cfg.hidden_dim | (MLP_CODES.get(cfg.mlp, cfg.mlp) << MLP_SHIFT))


class CNetwork(C.Structure):  # Network.h:18-21
    _fields_ = [("data", f32p), ("size", C.c_size_t)]


class CImageData(C.Structure):  # Network.h:7-13
    _fields_ = [("n", C.c_int), ("c", C.c_int), ("h", C.c_int), ("w", C.c_int), ("data", f32p)]


class COptions(C.Structure):
    _fields_ = [("device", C.c_int), ("max_batch", C.c_int), ("profile", C.c_int), ("lanes", C.c_int),
                ("dtype", C.c_int), ("prune_last_layer", C.c_int), ("use_graph", C.c_int), ("gemm_tile", C.c_int), ("ln_fold", C.c_int),
                ("gemm_handover_test", C.c_int), ("host_first_piece", C.c_int), ("fp32_split", C.c_int)]


class CFeatureSpec(C.Structure):  # vit_feature_spec
    _fields_ = [("kind", C.c_int), ("l2_normalize", C.c_int)]


FEATURE_KINDS = {"cls": 0, "mean": 1, "tokens": 2, "head": 4}  # VIT_FEAT_* (3 is unassigned)


class CAttentionSpec(C.Structure):  # vit_attention_spec
    _fields_ = [("kind", C.c_int), ("reserved", C.c_int)]


ATTENTION_KINDS = {"heads": 0, "head_mean": 1}  # VIT_ATTN_*


VIT_MAX_TAPS = 32


class CIntermediateSpec(C.Structure):  # vit_intermediate_spec
    _fields_ = [("kind", C.c_int), ("norm", C.c_int), ("num_layers", C.c_int), ("layers", C.c_int * VIT_MAX_TAPS), ("reserved", C.c_int)]


TAP_KINDS = {"cls": 0, "tokens": 1, "patches": 2, "map": 3}  # VIT_TAP_* / VITHIP_TAP_*


class CHeadSpec(C.Structure):  # vit_head_spec
    _fields_ = [("num_cls_layers", C.c_int), ("cls_layers", C.c_int * VIT_MAX_TAPS), ("pool", C.c_int), ("reserved", C.c_int)]


HEAD_POOLS = {"none": 0, "avg": 1, "avg_fcnorm": 2}  # VIT_HEAD_POOL_*


def head_spec(cls_layers=(), pool="none", depth: Optional[int] = None, reserved: int = 0) -> CHeadSpec:
    """cls_layers: the layers whose class rows the head reads, in increasing order; with `depth` given, negative entries count from
    the last layer (-1 = depth - 1).  pool: "none" | "avg" | "avg_fcnorm" (or a raw VIT_HEAD_POOL_* integer); everything is passed
    through unchecked for the C side to judge: num_cls_layers is len(cls_layers) even where that exceeds VIT_MAX_TAPS."""
    ls = [int(l) for l in (cls_layers if hasattr(cls_layers, "__iter__") else [cls_layers])]
    if depth is not None:
        ls = [l + depth if l < 0 else l for l in ls]
    spec = CHeadSpec(len(ls))
    for j, l in enumerate(ls[:VIT_MAX_TAPS]):
        spec.cls_layers[j] = l
    spec.pool = HEAD_POOLS[pool] if isinstance(pool, str) else int(pool)
    spec.reserved = int(reserved)
    return spec


class CDenseHeadSpec(C.Structure):  # vit_dense_head_spec
    _fields_ = [("num_layers", C.c_int), ("layers", C.c_int * VIT_MAX_TAPS), ("norm", C.c_int), ("num_classes", C.c_int), ("reserved", C.c_int)]


class CDenseSpec(C.Structure):  # vit_dense_spec
    _fields_ = [("kind", C.c_int), ("out_h", C.c_int), ("out_w", C.c_int), ("reserved", C.c_int)]


DENSE_KINDS = {"labels": 0, "grid": 1}  # VIT_DENSE_*
DENSE_NO_LABEL = 255  # the label of a pixel no class was a candidate for (every value NaN)


def dense_head_spec(layers, norm=True, num_classes: int = 0, depth: Optional[int] = None, reserved: int = 0) -> CDenseHeadSpec:
    """layers: the encoder layers whose patch tokens the head reads, in increasing order (mmseg out_indices); with `depth` given,
    negative entries count from the last layer.  Everything is passed through unchecked for the C side to judge."""
    ls = [int(l) for l in (layers if hasattr(layers, "__iter__") else [layers])]
    if depth is not None:
        ls = [l + depth if l < 0 else l for l in ls]
    spec = CDenseHeadSpec(len(ls))
    for j, l in enumerate(ls[:VIT_MAX_TAPS]):
        spec.layers[j] = l
    spec.norm, spec.num_classes, spec.reserved = int(norm), int(num_classes), int(reserved)
    return spec


def dense_spec(kind="labels", out_size=None, reserved: int = 0) -> CDenseSpec:
    """kind: "labels" | "grid" (or a raw VIT_DENSE_* integer); out_size: None (img_size x img_size), an int (square) or (out_h,
    out_w); passed through unchecked for the C side to judge."""
    k = DENSE_KINDS[kind] if isinstance(kind, str) else int(kind)
    h, w = (0, 0) if out_size is None else (out_size, out_size) if isinstance(out_size, (int, np.integer)) else out_size
    return CDenseSpec(k, int(h), int(w), int(reserved))


class CTopkSpec(C.Structure):  # vit_topk_spec
    _fields_ = [("k", C.c_int), ("score", C.c_int), ("reserved", C.c_int)]


SCORES = {"prob": 0, "logit": 1}  # VIT_SCORE_* / VITHIP_SCORE_*
VIT_MAX_TOPK = 64
TOPK_EMPTY_LABEL = 0x7FFFFFFF  # the label of a slot no candidate was left for; its score: -1.0 (prob) or -inf (logit)


def _score(score) -> int:
    return SCORES[score] if isinstance(score, str) else int(score)


class CPosResample(C.Structure):  # vit_pos_resample
    _fields_ = [("src_img_size", C.c_int), ("mode", C.c_int), ("reserved", C.c_int)]


POS_MODES = {"bicubic": 0, "bicubic_aa": 1}  # VIT_POS_* / VITHIP_POS_*


def _pos_mode(mode) -> int:
    return POS_MODES[mode] if isinstance(mode, str) else int(mode)


class CImageU8(C.Structure):  # vit_image_u8 / vithip_image_u8: one decoded image, [height][width][chans] uint8
    _fields_ = [("pixels", C.c_void_p), ("height", C.c_int), ("width", C.c_int)]


class CPreproc(C.Structure):  # vit_preproc: Resize(resize_shorter) -> CenterCrop(cfg.img_size) -> Normalize(mean, std)
    _fields_ = [("resize_shorter", C.c_int), ("mean", C.c_float * 4), ("std", C.c_float * 4)]


RESIZE_FILTERS = {"bilinear": 0, "bicubic": 1}  # VIT_RESIZE_* / VITHIP_RESIZE_*


def _resize_filter(filter) -> int:
    return RESIZE_FILTERS[filter] if isinstance(filter, str) else int(filter)


def feature_spec(kind, l2_normalize=False) -> CFeatureSpec:
    """kind: "cls" | "mean" | "tokens" (or a raw VIT_FEAT_* integer, passed through unchecked for the C side to judge)."""
    k = FEATURE_KINDS[kind] if isinstance(kind, str) else int(kind)
    return CFeatureSpec(k, int(l2_normalize))


def attention_spec(kind, reserved: int = 0) -> CAttentionSpec:
    """kind: "heads" | "head_mean" (or a raw VIT_ATTN_* integer, passed through unchecked for the C side to judge)."""
    k = ATTENTION_KINDS[kind] if isinstance(kind, str) else int(kind)
    return CAttentionSpec(k, int(reserved))


def topk_spec(k: int, score="prob", reserved: int = 0) -> CTopkSpec:
    """score: "prob" | "logit" (or a raw VIT_SCORE_* integer); everything is passed through unchecked for the C side to judge."""
    return CTopkSpec(int(k), _score(score), int(reserved))


def split_topk(records):
    """[n][2k] int32 records -> (labels int32 [n][k], scores float32 [n][k]): a row is k labels, then the k scores' bit patterns."""
    records = np.ascontiguousarray(records, np.int32)
    k = records.shape[-1] // 2
    assert records.shape[-1] == 2 * k, records.shape
    return records[..., :k].copy(), records[..., k:].copy().view(np.float32)


def intermediate_spec(layers, kind="cls", norm=True, depth: Optional[int] = None, reserved: int = 0) -> CIntermediateSpec:
    """layers: the encoder layers to tap, in increasing order; with `depth` given, negative entries count from the last layer as
    Python indices do (-1 = depth - 1) -- resolved here, the C side takes 0..depth-1 only.  kind: "cls" | "tokens" | "patches" | "map"
    (or a raw VIT_TAP_* integer); everything else is passed through unchecked for the C side to judge: num_layers is len(layers) even
    where that exceeds the VIT_MAX_TAPS entries the struct holds."""
    k = TAP_KINDS[kind] if isinstance(kind, str) else int(kind)
    ls = [int(l) for l in (layers if hasattr(layers, "__iter__") else [layers])]
    if depth is not None:
        ls = [l + depth if l < 0 else l for l in ls]
    spec = CIntermediateSpec(k, int(norm), len(ls))
    for j, l in enumerate(ls[:VIT_MAX_TAPS]):
        spec.layers[j] = l
    spec.reserved = int(reserved)
    return spec


class CStageTimes(C.Structure):
    _fields_ = [("ms", C.c_double * len(STAGES)), ("launches", C.c_long * len(STAGES)), ("images", C.c_long)]


class CDeviceInfo(C.Structure):
    _fields_ = [("name", C.c_char * 256), ("arch", C.c_char * 64), ("compute_units", C.c_int),
                ("clock_mhz", C.c_int), ("wavefront", C.c_int), ("lds_per_block", C.c_int),
                ("hbm_bytes", C.c_ulonglong)]


class CGemmArgs(C.Structure):
    _fields_ = [("A", C.c_void_p), ("lda", C.c_int), ("W", C.c_void_p), ("ldw", C.c_int),
                ("bias", C.c_void_p), ("residual", C.c_void_p), ("ldr", C.c_int),
                ("C", C.c_void_p), ("ldc", C.c_int), ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
                ("epilogue", C.c_int), ("tile", C.c_int), ("group_m", C.c_int), ("workspace", C.c_void_p),
                ("handover_test", C.c_int), ("ln_rows", C.c_void_p), ("ln_colsum", C.c_void_p),
                ("stats_out", C.c_void_p), ("stats_partials", C.c_void_p), ("arith", C.c_int), ("w_split", C.c_void_p), ("stats_eps", C.c_double)]


_lib: Optional[C.CDLL] = None


DP_LIB_PATH = os.path.join(HERE, "libvit_mi355x_dp.so")
_dp_lib = None


def dp_lib() -> C.CDLL:
    """libvit_mi355x_dp.so (include/vit_dp.h): the RCCL all-gather of the top-1 records behind the C-ABI."""
    global _dp_lib
    if _dp_lib is None:
        if not os.path.exists(DP_LIB_PATH):
            raise VitError(f"{DP_LIB_PATH} is missing: run `make -C {HERE}`")
        L = C.CDLL(DP_LIB_PATH)
        L.vit_dp_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_int), C.c_int]
        L.vit_dp_destroy.argtypes = [C.c_void_p]
        L.vit_dp_destroy.restype = None
        L.vit_dp_size.argtypes = [C.c_void_p]
        L.vit_dp_device.argtypes = [C.c_void_p, C.c_int]
        L.vit_dp_last_error.argtypes = [C.c_void_p]
        L.vit_dp_last_error.restype = C.c_char_p
        L.vit_dp_gather_top1.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_size_t, C.POINTER(C.c_void_p)]
        _dp_lib = L
    return _dp_lib


class DpGroup:
    """vit_dp (include/vit_dp.h): one RCCL communicator per listed device of this process."""

    def __init__(self, devices):
        self.devices = [int(d) for d in devices]
        self._h = C.c_void_p()
        arr = (C.c_int * len(self.devices))(*self.devices)
        rc = dp_lib().vit_dp_create(C.byref(self._h), arr, len(self.devices))
        if rc != 0:
            raise VitError(f"vit_dp_create({self.devices}) failed: {rc}")

    def gather_top1(self, send_ptrs, recv_ptrs, records: int, streams=None) -> None:
        n = len(self.devices)
        send = (C.c_void_p * n)(*send_ptrs)
        recv = (C.c_void_p * n)(*recv_ptrs)
        st = (C.c_void_p * n)(*streams) if streams is not None else None
        rc = dp_lib().vit_dp_gather_top1(self._h, send, recv, records, st)
        if rc != 0:
            raise VitError(f"vit_dp_gather_top1: {dp_lib().vit_dp_last_error(self._h).decode()} ({rc})")

    def close(self) -> None:
        if self._h:
            dp_lib().vit_dp_destroy(self._h)
            self._h = C.c_void_p()


def lib() -> C.CDLL:
    """Load the native library; never falls back to anything else."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise VitError(f"{LIB_PATH} is missing: the HIP extension has not been built "
                           "(run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C "
                           f"{HERE}`); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        L.vithip_error_string.restype = C.c_char_p
        L.vit_engine_last_error.restype = C.c_char_p
        L.vit_engine_last_error.argtypes = [C.c_void_p]
        L.vit_engine_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(CConfig), C.POINTER(COptions)]
        L.vit_engine_destroy.argtypes = [C.c_void_p]
        L.vit_engine_load_weights.argtypes = [C.c_void_p, C.POINTER(CNetwork), C.c_int]
        # the forward surface, output kind x place x input kind: (engine, images, n) + normalisation + spec + destination
        norm = {"": [], "_u8": [f32p, f32p], "_images": [C.POINTER(CPreproc)]}
        spec = {"forward": [], "features": [C.POINTER(CFeatureSpec)], "cls_attention": [C.POINTER(CAttentionSpec)],
                "intermediate": [C.POINTER(CIntermediateSpec)], "topk": [C.POINTER(CTopkSpec)], "dense": [C.POINTER(CDenseSpec)]}
        for out in spec:
            for place in ("host", "device"):
                for kind in norm:
                    images = C.POINTER(CImageU8) if kind == "_images" else C.c_void_p if place == "device" else \
                        C.POINTER(C.c_void_p if kind == "_u8" else f32p)
                    # host: a row per image; device: the rows, a forward's top-1 labels and probabilities, the stream
                    dst = [C.POINTER(i32p if out == "topk" else C.c_void_p if out == "dense" else f32p)] if place == "host" else [C.c_void_p] * (4 if out == "forward" else 2)
                    name = f"vit_engine_{out}_{place}{kind}"
                    if hasattr(L, name):  # VIT_HIP_LIBRARY may name an earlier build (A/B timing), which lacks the later calls
                        getattr(L, name).argtypes = [C.c_void_p, images, C.c_int] + norm[kind] + spec[out] + dst
        if hasattr(L, "vit_engine_features_device"):  # an earlier build (see above) has no feature calls
            L.vit_engine_feature_row_elems.restype = C.c_size_t
            L.vit_engine_feature_row_elems.argtypes = [C.c_void_p, C.POINTER(CFeatureSpec)]
            L.vithip_layernorm_pool_f32_workspace_floats.restype = C.c_size_t
            L.vithip_layernorm_pool_f32_workspace_floats.argtypes = [C.c_int] * 4
            L.vithip_layernorm_pool_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                    C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
            L.vithip_l2_normalize_rows_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int]
            L.vit_engine_debug_pool_scratch.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_size_t)]
        L.vithip_images_u8_to_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, f32p, f32p]
        if hasattr(L, "vit_engine_forward_device_images"):  # an earlier build (see above) has no decoded-image calls
            recs = C.POINTER(CImageU8)
            L.vithip_images_u8_resize_crop_to_f32.argtypes = [C.c_void_p, recs, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, f32p, f32p]
            L.vithip_images_u8_resize_crop_check.argtypes = [recs, C.c_int, C.c_int, C.c_int, C.c_int]
        if hasattr(L, "vit_engine_set_resize_filter"):  # an earlier build (see above) resizes bilinearly only
            recs = C.POINTER(CImageU8)
            L.vithip_images_u8_resize_crop_to_f32_filter.argtypes = [C.c_void_p, recs, C.c_int, C.c_void_p] + [C.c_int] * 4 + [f32p, f32p]
            L.vithip_images_u8_resize_crop_check_filter.argtypes = [recs] + [C.c_int] * 5
            L.vit_engine_set_resize_filter.argtypes = [C.c_void_p, C.c_int]
            L.vit_engine_get_resize_filter.argtypes = [C.c_void_p]
        if hasattr(L, "vit_engine_cls_attention_device"):  # an earlier build (see above) has no attention calls
            L.vit_engine_attention_row_elems.restype = C.c_size_t
            L.vit_engine_attention_row_elems.argtypes = [C.c_void_p, C.POINTER(CAttentionSpec)]
        if hasattr(L, "vit_engine_intermediate_device"):  # an earlier build (see above) has no intermediate calls
            L.vit_engine_intermediate_row_elems.restype = C.c_size_t
            L.vit_engine_intermediate_row_elems.argtypes = [C.c_void_p, C.POINTER(CIntermediateSpec)]
            L.vithip_tap_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p] + [C.c_int] * 4
        if hasattr(L, "vit_engine_topk_device"):  # an earlier build (see above) has no top-k calls
            L.vit_engine_topk_row_elems.restype = C.c_size_t
            L.vit_engine_topk_row_elems.argtypes = [C.c_void_p, C.POINTER(CTopkSpec)]
            L.vithip_softmax_topk_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_int] * 4
        if hasattr(L, "vit_engine_load_weights_resampled"):  # an earlier build (see above) cannot resample a position embedding
            L.vit_engine_load_weights_resampled.argtypes = [C.c_void_p, C.POINTER(CNetwork), C.c_int, C.POINTER(CPosResample)]
            L.vit_engine_copy_weights_resampled.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
            L.vithip_pos_resample_table.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), f32p, C.c_int]
            L.vithip_pos_resample_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int]
        if hasattr(L, "vit_engine_set_head"):  # an earlier build (see above) has the checkpoint's own head only
            L.vit_engine_head_in_features.restype = C.c_size_t
            L.vit_engine_head_in_features.argtypes = [C.c_void_p, C.POINTER(CHeadSpec)]
            L.vit_engine_set_head.argtypes = [C.c_void_p, C.POINTER(CHeadSpec), f32p, f32p]
            L.vit_engine_read_head_operand.argtypes = [C.c_void_p, f32p, C.c_int]
            L.vithip_pool_layernorm_f32_workspace_floats.restype = C.c_size_t
            L.vithip_pool_layernorm_f32_workspace_floats.argtypes = [C.c_int] * 4
            L.vithip_pool_layernorm_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p,
                                                    C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        if hasattr(L, "vit_engine_set_dense_head"):  # an earlier build (see above) has no dense heads
            L.vit_engine_set_dense_head.argtypes = [C.c_void_p, C.POINTER(CDenseHeadSpec), f32p, f32p]
            L.vit_engine_dense_row_bytes.restype = C.c_size_t
            L.vit_engine_dense_row_bytes.argtypes = [C.c_void_p, C.POINTER(CDenseSpec)]
            L.vit_dense_head_fold_batchnorm.argtypes = [f32p, f32p, C.c_int, C.c_int, f32p, f32p, f32p, f32p, C.c_double]
            L.vithip_dense_upsample_argmax_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t] + [C.c_int] * 5
            L.vithip_dense_grid_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t] + [C.c_int] * 3
        L.vit_engine_read_logits.argtypes = [C.c_void_p, f32p, C.c_int]
        L.vit_engine_sync.argtypes = [C.c_void_p]
        L.vit_engine_get_stage_times.argtypes = [C.c_void_p, C.POINTER(CStageTimes)]
        L.vit_engine_reset_stage_times.argtypes = [C.c_void_p]
        L.vit_engine_set_profile.argtypes = [C.c_void_p, C.c_int]
        L.vit_config_weight_size.restype = C.c_size_t
        L.vit_config_weight_size.argtypes = [C.POINTER(CConfig), C.c_int]
        L.vit_config_macs_per_image.restype = C.c_ulonglong
        L.vit_config_macs_per_image.argtypes = [C.POINTER(CConfig)]
        L.vit_config_macs_per_image_pruned.restype = C.c_ulonglong
        L.vit_config_macs_per_image_pruned.argtypes = [C.POINTER(CConfig)]
        L.vit_config_b16.restype = CConfig
        L.load_image_data.restype = C.POINTER(CImageData)
        L.load_image_data.argtypes = [C.c_char_p]
        L.free_image_data.argtypes = [C.POINTER(CImageData)]
        L.load_weights.argtypes = [C.c_char_p, C.POINTER(CNetwork), C.c_int]
        L.free_weights.argtypes = [C.POINTER(CNetwork), C.c_int]
        L.vit_round_weights.argtypes = [f32p, C.c_size_t]
        L.vit_compare_results.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_float]
        L.vit_synth_uniform.argtypes = [C.c_ulonglong, C.c_int, C.c_size_t, C.c_float, C.c_float, f32p]
        L.vit_synth_weights.argtypes = [C.POINTER(CConfig), C.c_ulonglong, C.POINTER(CNetwork), C.c_int]
        L.vit_synth_images.restype = C.POINTER(CImageData)
        L.vit_synth_images.argtypes = [C.POINTER(CConfig), C.c_int, C.c_ulonglong]
        L.vit_argmax.argtypes = [f32p, C.c_int]
        L.ViT_hip.argtypes = [C.POINTER(CImageData), C.POINTER(CNetwork), C.POINTER(f32p)]
        L.ViT_opencl.argtypes = [C.POINTER(CImageData), C.POINTER(CNetwork), C.POINTER(f32p)]
        for fn in ("vithip_malloc", "vithip_host_alloc"):
            getattr(L, fn).argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        L.vithip_free.argtypes = [C.c_void_p]
        for fn in ("vithip_memcpy_h2d", "vithip_memcpy_d2h", "vithip_memcpy_d2d"):
            getattr(L, fn).argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.vithip_gemm_f32.argtypes = [C.c_void_p, C.POINTER(CGemmArgs)]
        L.vithip_split3_weights_bytes.argtypes = [C.c_int, C.c_int]
        L.vithip_split3_weights_bytes.restype = C.c_size_t
        L.vithip_split3_weights_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        L.vithip_patch_embed_f32.argtypes = [C.c_void_p] + [C.c_void_p] * 6 + [C.c_int] * 5
        if hasattr(L, "vithip_patch_embed_f32_general"):  # an earlier build (see above) has neither the general embedding nor the fold
            L.vithip_patch_embed_f32_general.argtypes = [C.c_void_p] + [C.c_void_p] * 6 + [C.c_int] * 5
            L.vit_weights_fold_layer_scale.argtypes = [C.POINTER(CConfig), C.POINTER(CNetwork), C.c_int, C.POINTER(CNetwork), C.c_int]
        L.vithip_layernorm_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                           C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        # the attention entries: (stream, qkv, out) or (stream, qkv, row stride, out, ld_out), then ints (include/vit_hip_kernels.h)
        pv, cls = [C.c_void_p] * 3, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
        for fn in ("vithip_attention_f32", "vithip_attention_bf16io", "vithip_attention_bf16io_f32math"):
            getattr(L, fn).argtypes = pv + [C.c_int] * 3
        for fn in ("vithip_attention_f32_rows", "vithip_attention_bf16io_rows", "vithip_attention_bf16io_qscaled"):
            getattr(L, fn).argtypes = pv + [C.c_int] * 4
        if hasattr(L, "vit_engine_cls_attention_device"):  # an earlier build (see above) has no attention calls
            L.vithip_cls_attention_f32.argtypes = cls + [C.c_int] * 4
            L.vithip_cls_attention_bf16.argtypes = cls + [C.c_int] * 5
        if hasattr(L, "vithip_attention_f32_hd"):  # an earlier build (see above) has head_dim 64 only
            L.vithip_qscale.restype = C.c_float
            L.vithip_qscale.argtypes = [C.c_int]
            L.vithip_attention_f32_hd.argtypes = pv + [C.c_int] * 5
            L.vithip_attention_bf16io_hd.argtypes = pv + [C.c_int] * 6
            L.vithip_cls_attention_f32_hd.argtypes = cls + [C.c_int] * 5
            L.vithip_cls_attention_bf16_hd.argtypes = cls + [C.c_int] * 6
        if hasattr(L, "vithip_attention_f32_split"):  # an earlier build (see above) has fp32 arithmetic only
            L.vithip_attention_f32_split.argtypes = pv + [C.c_int] * 5
        L.vithip_softmax_top1_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                              C.c_void_p, C.c_int, C.c_int]
        L.vithip_event_create.argtypes = [C.POINTER(C.c_void_p)]
        L.vithip_event_record.argtypes = [C.c_void_p, C.c_void_p]
        L.vithip_event_sync.argtypes = [C.c_void_p]
        L.vithip_event_destroy.argtypes = [C.c_void_p]
        L.vithip_event_elapsed_ms.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        L.vithip_stream_sync.argtypes = [C.c_void_p]
        L.vithip_get_device_info.argtypes = [C.c_int, C.POINTER(CDeviceInfo)]
        _lib = L
    return _lib


def hip_check(rc: int, what: str = "HIP call") -> None:
    if rc != 0:
        err = VitError(f"{what}: HIP error {rc} ({lib().vithip_error_string(rc).decode()})")
        err.code = int(rc)   # hipErrorInvalidValue = 1: what a launcher answers to a layout it refuses
        raise err


def _as_f32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32)


def networks_from(weights: Sequence[np.ndarray]):
    """(ctypes Network[count], keep-alive list).  `None` entries become {NULL, 0}."""
    arr = (CNetwork * len(weights))()
    keep = []
    for i, w in enumerate(weights):
        if w is None:
            arr[i].data = None
            arr[i].size = 0
        else:
            w = _as_f32(w)
            keep.append(w)
            arr[i].data = w.ctypes.data_as(f32p)
            arr[i].size = w.size
    return arr, keep


# --------------------------------------------------------------------------------------------------
# Device buffers for the op-level entry points
# --------------------------------------------------------------------------------------------------
class DeviceArray:
    """A float32/int32 array in HBM owned through the C-ABI (vithip_malloc / vithip_free)."""

    def __init__(self, shape, dtype=np.float32):
        self.shape = tuple(int(s) for s in np.atleast_1d(shape))
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        p = C.c_void_p()
        hip_check(lib().vithip_malloc(C.byref(p), max(self.nbytes, 16)), "vithip_malloc")
        self.ptr = p.value

    @classmethod
    def from_numpy(cls, a: np.ndarray) -> "DeviceArray":
        a = np.ascontiguousarray(a)
        d = cls(a.shape, a.dtype)
        hip_check(lib().vithip_memcpy_h2d(d.ptr, a.ctypes.data, a.nbytes, None), "h2d")
        hip_check(lib().vithip_device_sync(), "sync")
        return d

    def numpy(self) -> np.ndarray:
        out = np.empty(self.shape, self.dtype)
        hip_check(lib().vithip_device_sync(), "sync")
        hip_check(lib().vithip_memcpy_d2h(out.ctypes.data, self.ptr, self.nbytes, None), "d2h")
        hip_check(lib().vithip_device_sync(), "sync")
        return out

    def free(self) -> None:
        if self.ptr:
            lib().vithip_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _PlainBuffer:
    """A rows x width matrix with leading dimension ld, `offset` elements into its allocation: what the op wrappers below place
    every operand in.  tests/strided.py's Frame has the same .ptr / .ld / .window() and adds guard rows and a sentinel."""

    def __init__(self, rows, width, ld=None, dtype=np.float32, offset=0, data=None):
        self.rows, self.width, self.ld = int(rows), int(width), int(width if ld is None else ld)
        self.dtype, self.offset = np.dtype(dtype), int(offset)
        img = np.zeros(self.offset + self.rows * self.ld, self.dtype)
        if data is not None:
            img[self.offset:].reshape(self.rows, self.ld)[:, :self.width] = np.asarray(data, self.dtype).reshape(self.rows, self.width)
        self.dev = DeviceArray.from_numpy(img)
        self.ptr = self.dev.ptr + self.offset * self.dtype.itemsize

    def window(self):
        return self.dev.numpy()[self.offset:].reshape(self.rows, self.ld)[:, :self.width].copy()


class _Plain:
    """The default `frames` of the op wrappers: exact allocations, no guards (tests pass the module tests/strided.py instead)."""

    @staticmethod
    def framed(data, ld=None, dtype=None, offset=0):
        data = np.asarray(data)
        d2 = data.reshape(1, -1) if data.ndim == 1 else data.reshape(data.shape[0], -1)
        return _PlainBuffer(d2.shape[0], d2.shape[1], ld, dtype or data.dtype, offset, d2)

    @staticmethod
    def out_frame(rows, width, ld=None, dtype=np.float32, offset=0, preload=None):
        return _PlainBuffer(rows, width, ld, dtype, offset, preload)


def _ln_fn(name: str, eps):
    """(function, extra arguments) of a LayerNorm entry point: `name` itself, or with an epsilon its sibling `name_eps`, which takes
    one more, last, double.  Call it behind the place that sets `name`'s argtypes."""
    L = lib()
    base = getattr(L, name)
    if eps is None:
        return base, ()
    fn = getattr(L, name + "_eps")
    assert base.argtypes, name
    fn.argtypes = list(base.argtypes) + [C.c_double]
    return fn, (float(eps),)


def _note(sink, **frames):
    """Hand the output frames of a call to the caller's dict (before the launch: a refused call leaves them to be inspected)."""
    if sink is not None:
        sink.update({k: v for k, v in frames.items() if v is not None})


def gemm(A, W, bias, residual=None, epilogue=EPI_BIAS, tile: int = 0, group_m: int = 0, workspace: bool = False,
         handover_test: int = 0, stats: Optional[dict] = None, ln=None, row_stats: Optional[dict] = None,
         arith: int = ARITH_F32, w_split: bool = False, lda: Optional[int] = None, ldw: Optional[int] = None,
         ldr: Optional[int] = None, ldc: Optional[int] = None, in_place: bool = False, offset: int = 0, frames=None,
         out: Optional[dict] = None, stats_eps: float = 0.0, walk: Optional[dict] = None) -> np.ndarray:
    """C = epilogue(A . W^T + bias) through vithip_gemm_f32 (tile / group_m: per-call tuning fields, 0 = auto;
    workspace: lend the scratch that enables the helper pieces of the persistent walk; handover_test: see
    vithip_gemm_args; stats: receives the hand-over counters {"taken", "recomputed"} of the launch;
    ln = (rows [M][2], colsum [N] or None): the consumer side of the LayerNorm fold, W / bias being the folded operands (None: the
    CENTRED weight of ln_fold_weights_f32_centered, nothing to subtract);
    row_stats: a dict that receives "rows" = vithip_gemm_args.stats_out [M][2] and "in_epilogue" = what
    vithip_gemm_f32_stats_in_epilogue said; its key "scratch" (default True) lends stats_partials);
    arith: ARITH_F32 (fp32 MFMA) or ARITH_SPLIT3 (the three-piece split on the bf16 matrix pipe; tiles 0, 9, 10, 11);
    w_split: make W's pre-split image on the device (split3_weights_device) and pass it as vithip_gemm_args.w_split;
    lda / ldw / ldr / ldc: leading dimensions (default: dense); in_place: C is the residual's buffer (ldr = ldc);
    offset: C, bias and the residual start this many floats past a 16-byte boundary;
    frames: who allocates the operands (default: exact buffers; tests/strided.py: guarded, sentinel-filled frames);
    out: a dict that receives the output frames "C", "stats" and "partials";
    stats_eps: the LayerNorm epsilon of row_stats (vithip_gemm_args.stats_eps; 0 = the default, the double 1e-6);
    walk: a dict that receives "tile" = (bm, bn), what vithip_gemm_f32_walk_tile says the persistent walk takes for this call."""
    A, W, bias = _as_f32(A), _as_f32(W), _as_f32(bias)
    M, K = A.shape
    N = W.shape[0]
    F = frames or _Plain
    dA, dW, db = F.framed(A, lda), F.framed(W, ldw), F.framed(bias, offset=offset)
    if in_place:
        dC = dR = F.out_frame(M, N, ldc, offset=offset, preload=_as_f32(residual))
    else:
        dC = F.out_frame(M, N, ldc, offset=offset)
        dR = F.framed(_as_f32(residual), ldr, offset=offset) if residual is not None else None
    ws = gemm_workspace() if workspace else None
    dRows = DeviceArray.from_numpy(_as_f32(ln[0])) if ln is not None else None
    dCs = DeviceArray.from_numpy(_as_f32(ln[1])) if ln is not None and ln[1] is not None else None   # None: centred weights
    dSt = F.out_frame(M, 2) if row_stats is not None else None
    dPart = F.out_frame(max(N // 64, 1) * M, 2) if row_stats is not None and row_stats.get("scratch", True) else None
    _note(out, C=dC, stats=dSt, partials=dPart)
    args = CGemmArgs(dA.ptr, dA.ld, dW.ptr, dW.ld, db.ptr, dR.ptr if dR else None, dR.ld if dR else N, dC.ptr, dC.ld, M, N, K, epilogue,
                     tile, group_m, ws, handover_test, dRows.ptr if dRows else None, dCs.ptr if dCs else None,
                     dSt.ptr if dSt else None, dPart.ptr if dPart else None, arith)
    dImg = split3_weights_device(dW, N, K, dW.ld) if w_split else None
    if dImg is not None:
        args.w_split = dImg.ptr
    args.stats_eps = stats_eps
    if row_stats is not None:
        row_stats["in_epilogue"] = int(lib().vithip_gemm_f32_stats_in_epilogue(C.byref(args)))
    if walk is not None:
        walk["tile"] = gemm_walk_tile(args)
    try:
        hip_check(lib().vithip_gemm_f32(None, C.byref(args)), "vithip_gemm_f32")
    except VitError:
        if ws:
            lib().vithip_gemm_f32_workspace_destroy(C.c_void_p(ws))
        raise
    result = dC.window()
    if row_stats is not None:
        row_stats["rows"] = dSt.window()
    if ws:
        if stats is not None:
            stats.update(gemm_workspace_stats(ws))
        lib().vithip_gemm_f32_workspace_destroy(C.c_void_p(ws))
    return result


def gemm_walk_tile(args: "CGemmArgs") -> tuple:
    """vithip_gemm_f32_walk_tile: (rows, columns) of the tile the persistent walk takes for these arguments (host only)."""
    bm, bn = C.c_int(), C.c_int()
    hip_check(lib().vithip_gemm_f32_walk_tile(C.byref(args), C.byref(bm), C.byref(bn)), "vithip_gemm_f32_walk_tile")
    return bm.value, bn.value


def split3_weights_device(dW: "DeviceArray", N: int, K: int, ldw: Optional[int] = None) -> "DeviceArray":
    """vithip_split3_weights_f32: the pre-split image of the device matrix dW [N][ldw] (vithip_gemm_args.w_split), as a DeviceArray of bytes."""
    nbytes = int(lib().vithip_split3_weights_bytes(N, K))
    if nbytes == 0:
        raise VitError(f"vithip_split3_weights_bytes({N}, {K}): bad shape")
    out = DeviceArray((nbytes,), np.uint8)
    hip_check(lib().vithip_split3_weights_f32(None, dW.ptr, K if ldw is None else ldw, N, K, out.ptr), "vithip_split3_weights_f32")
    return out


def split3_weights(W) -> np.ndarray:
    """The pre-split image of W [N][K] (fp32), copied back: uint16 [ceil(N / 128)][K / 16][3][128][16] bf16 bit patterns."""
    W = _as_f32(W)
    N, K = W.shape
    img = split3_weights_device(DeviceArray.from_numpy(W), N, K).numpy()
    return img.view(np.uint16).reshape((N + 127) // 128, K // 16, 3, 128, 16)


def gemm_workspace() -> int:
    """vithip_gemm_f32_workspace_create: the handle for vithip_gemm_args.workspace (free with vithip_gemm_f32_workspace_destroy)."""
    p = C.c_void_p()
    hip_check(lib().vithip_gemm_f32_workspace_create(C.byref(p)), "vithip_gemm_f32_workspace_create")
    return p.value


def gemm_workspace_stats(ws: int) -> dict:
    """vithip_gemm_f32_workspace_stats: hand-overs since the last call (syncs the device first)."""
    L = lib()
    hip_check(L.vithip_device_sync(), "vithip_device_sync")
    t, r = C.c_int(), C.c_int()
    L.vithip_gemm_f32_workspace_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    hip_check(L.vithip_gemm_f32_workspace_stats(ws, C.byref(t), C.byref(r)), "vithip_gemm_f32_workspace_stats")
    return {"taken": t.value, "recomputed": r.value}


def gemm_workspace_flags(ws: int, count: int = 1016) -> np.ndarray:
    """The per-owner flags of a workspace (0 = empty after every complete launch)."""
    L = lib()
    L.vithip_gemm_f32_workspace_device_ptr.restype = C.c_void_p
    L.vithip_gemm_f32_workspace_device_ptr.argtypes = [C.c_void_p]
    flags = np.empty(count, np.int32)
    hip_check(L.vithip_device_sync(), "sync")
    hip_check(L.vithip_memcpy_d2h(flags.ctypes.data, L.vithip_gemm_f32_workspace_device_ptr(ws), flags.nbytes, None), "d2h")
    hip_check(L.vithip_device_sync(), "sync")
    return flags


def gemm_workspace_set_flags(ws: int, values) -> None:
    """Overwrite the first len(values) per-owner flags (tests: what an aborted launch may have left behind)."""
    L = lib()
    L.vithip_gemm_f32_workspace_device_ptr.restype = C.c_void_p
    L.vithip_gemm_f32_workspace_device_ptr.argtypes = [C.c_void_p]
    v = np.ascontiguousarray(values, np.int32)
    hip_check(L.vithip_device_sync(), "sync")
    hip_check(L.vithip_memcpy_h2d(L.vithip_gemm_f32_workspace_device_ptr(ws), v.ctypes.data, v.nbytes, None), "h2d")
    hip_check(L.vithip_device_sync(), "sync")


class CGemmBf16Args(C.Structure):
    _fields_ = [("A", C.c_void_p), ("lda", C.c_int), ("W", C.c_void_p), ("ldw", C.c_int), ("bias", C.c_void_p),
                ("residual", C.c_void_p), ("ldr", C.c_int), ("C", C.c_void_p), ("ldc", C.c_int),
                ("M", C.c_int), ("N", C.c_int), ("K", C.c_int), ("epilogue", C.c_int),
                ("variant", C.c_int),
                ("ln_rows", C.c_void_p), ("ln_colsum", C.c_void_p), ("x16", C.c_void_p), ("ldx16", C.c_int),
                ("row_partials", C.c_void_p)]


BF16_EPI_BF16, BF16_EPI_BF16_GELU, BF16_EPI_F32_RESIDUAL = 0, 1, 2
BF16_EPI_BF16_QGELU = 4  # VITHIP_BF16_EPI_BF16_QGELU (3 is the patch embedding's own)


def to_bf16_bits(x: np.ndarray) -> np.ndarray:
    """fp32 -> bf16 bit patterns (uint16), round to nearest even (host model of v_cvt_pk_bf16_f32)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def from_bf16_bits(b: np.ndarray) -> np.ndarray:
    return (b.astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16_device(x: np.ndarray) -> np.ndarray:
    """The device conversion kernel (vithip_f32_to_bf16)."""
    x = _as_f32(x)
    L = lib()
    L.vithip_f32_to_bf16.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    dx = DeviceArray.from_numpy(x)
    dy = DeviceArray(x.shape, np.uint16)
    hip_check(L.vithip_f32_to_bf16(None, dx.ptr, dy.ptr, x.size), "vithip_f32_to_bf16")
    return dy.numpy()


def gemm_bf16(A_bits, W_bits, bias, residual=None, epilogue=BF16_EPI_BF16, variant: int = 0, ln_rows=None, ln_colsum=None,
              ln_producer: bool = False, lda: Optional[int] = None, ldw: Optional[int] = None, ldr: Optional[int] = None,
              ldc: Optional[int] = None, in_place: bool = False, ldx16: Optional[int] = None, frames=None, out: Optional[dict] = None):
    """vithip_gemm_bf16 on bf16 bit patterns; returns bf16 bits (uint16) or fp32 for the residual epilogue.
    variant: 0 auto, 1 two-stage kernel, 2 ping-pong kernel (fails for K < 128).
    LayerNorm fold: ln_rows [M][2] + ln_colsum [N] make this the consumer; ln_producer (residual epilogue) also returns
    (C, bf16(C) bits, row partials [strips][M][2]).
    lda / ldw / ldr / ldc / ldx16, in_place, frames, out: as for gemm(); the output frames are "C", "x16" and "partials"."""
    L = lib()
    L.vithip_gemm_bf16.argtypes = [C.c_void_p, C.POINTER(CGemmBf16Args)]
    M, K = A_bits.shape
    N = W_bits.shape[0]
    F = frames or _Plain
    dA, dW = F.framed(np.ascontiguousarray(A_bits, np.uint16), lda), F.framed(np.ascontiguousarray(W_bits, np.uint16), ldw)
    db = F.framed(_as_f32(bias))
    out_f32 = epilogue == BF16_EPI_F32_RESIDUAL
    if in_place:
        dC = dR = F.out_frame(M, N, ldc, np.float32, preload=_as_f32(residual))
    else:
        dC = F.out_frame(M, N, ldc, np.float32 if out_f32 else np.uint16)
        dR = F.framed(_as_f32(residual), ldr) if residual is not None else None
    dRows = DeviceArray.from_numpy(_as_f32(ln_rows)) if ln_rows is not None else None
    dCs = DeviceArray.from_numpy(_as_f32(ln_colsum)) if ln_colsum is not None else None
    strips = ln_strips(N)
    dX16 = F.out_frame(M, N, ldx16, np.uint16) if ln_producer else None
    dPart = F.out_frame(strips * M, 2) if ln_producer else None
    _note(out, C=dC, x16=dX16, partials=dPart)
    args = CGemmBf16Args(dA.ptr, dA.ld, dW.ptr, dW.ld, db.ptr, dR.ptr if dR else None, dR.ld if dR else N, dC.ptr, dC.ld, M, N, K,
                         epilogue, variant, dRows.ptr if dRows else None, dCs.ptr if dCs else None,
                         dX16.ptr if dX16 else None, dX16.ld if dX16 else N, dPart.ptr if dPart else None)
    hip_check(L.vithip_gemm_bf16(None, C.byref(args)), "vithip_gemm_bf16")
    if ln_producer:
        return dC.window(), dX16.window(), dPart.window().reshape(strips, M, 2)
    return dC.window()


def ln_strips(N: int) -> int:
    return int(lib().vithip_ln_strips(int(N)))


def ln_fold_weights(W, bias, gamma, beta):
    """vithip_ln_fold_weights -> (Wf bf16 bits [N][K], colsum [N], bias_f [N])."""
    W = _as_f32(W)
    N, K = W.shape
    L = lib()
    L.vithip_ln_fold_weights.argtypes = [C.c_void_p] * 8 + [C.c_int, C.c_int]
    dW, db, dg, dbe = (DeviceArray.from_numpy(_as_f32(a)) for a in (W, bias, gamma, beta))
    dWf, dcs, dbf = DeviceArray((N, K), np.uint16), DeviceArray((N,), np.float32), DeviceArray((N,), np.float32)
    hip_check(L.vithip_ln_fold_weights(None, dW.ptr, db.ptr, dg.ptr, dbe.ptr, dWf.ptr, dcs.ptr, dbf.ptr, N, K), "vithip_ln_fold_weights")
    return dWf.numpy(), dcs.numpy(), dbf.numpy()


def rowstats_bf16(x, ldx: Optional[int] = None, ldx16: Optional[int] = None, frames=None, out: Optional[dict] = None, eps=None):
    """vithip_rowstats_bf16 -> (bf16(x) bits, rows [M][2] = (rstd, mean * rstd)).  ldx / ldx16, frames, out: as for gemm(); the
    output frames are "x16" and "rows"."""
    x = _as_f32(x)
    rows, dim = x.shape
    L = lib()
    L.vithip_rowstats_bf16.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int]
    F = frames or _Plain
    dx, d16, dr = F.framed(x, ldx), F.out_frame(rows, dim, ldx16, np.uint16), F.out_frame(rows, 2)
    _note(out, x16=d16, rows=dr)
    fn, e = _ln_fn("vithip_rowstats_bf16", eps)
    hip_check(fn(None, dx.ptr, dx.ld, d16.ptr, d16.ld, dr.ptr, rows, dim, *e), "vithip_rowstats_bf16")
    return d16.window(), dr.window()


def rowstats_finalize(partials, dim: int, eps=None, f32: bool = False):
    """vithip_rowstats_finalize: partials [strips][M][2] -> rows [M][2] = (rstd, mean * rstd); f32: vithip_rowstats_finalize_f32, the
    fp32 fold's (rstd, mean) of [dim / 64][M][2].  eps: the _eps sibling."""
    partials = _as_f32(partials)
    strips, rows, _ = partials.shape
    L = lib()
    L.vithip_rowstats_finalize.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    dp, dr = DeviceArray.from_numpy(partials), DeviceArray((rows, 2), np.float32)
    if f32:
        L.vithip_rowstats_finalize_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        fn, e = _ln_fn("vithip_rowstats_finalize_f32", eps)
        hip_check(fn(None, dp.ptr, rows, dim, dr.ptr, *e), "vithip_rowstats_finalize_f32")
        return dr.numpy()
    fn, e = _ln_fn("vithip_rowstats_finalize", eps)
    hip_check(fn(None, dp.ptr, strips, rows, dim, dr.ptr, *e), "vithip_rowstats_finalize")
    return dr.numpy()


def layernorm_bf16out(x, gamma, beta, ldx: Optional[int] = None, ldy: Optional[int] = None, frames=None,
                      out: Optional[dict] = None, eps=None) -> np.ndarray:
    """vithip_layernorm_f32_bf16out -> bf16 bits.  ldx / ldy, frames, out: as for gemm(); the output frame is "y"."""
    x = _as_f32(x)
    rows, dim = x.shape
    L = lib()
    L.vithip_layernorm_f32_bf16out.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                               C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    F = frames or _Plain
    dx, dg, db = F.framed(x, ldx), F.framed(_as_f32(gamma)), F.framed(_as_f32(beta))
    dy = F.out_frame(rows, dim, ldy, np.uint16)
    _note(out, y=dy)
    fn, e = _ln_fn("vithip_layernorm_f32_bf16out", eps)
    hip_check(fn(None, dx.ptr, dx.ld, dy.ptr, dy.ld, dg.ptr, db.ptr, rows, dim, *e), "vithip_layernorm_f32_bf16out")
    return dy.window()


QSCALE = 0.18033688011112042  # VITHIP_QSCALE: (1/sqrt(64)) * log2(e)


def _attention(name, qkv, n_images, tokens, heads, head_dim, args, fill=0, frames=None, out=None):
    """The P.V entry `name`(stream, qkv, out, n_images, tokens, heads, *args): qkv [n_images * tokens][3 * heads * head_dim], fp32 or
    bf16 bits, -> [n_images * tokens][heads * head_dim] of the same type.  Rows the call does not write keep `fill` (with `frames`:
    the frame's sentinel), and `out` receives the frame "out"."""
    rows, D = n_images * tokens, heads * head_dim
    qkv = qkv.reshape(rows, 3 * D)
    if frames is None:
        dq, do = _Plain.framed(qkv), _Plain.out_frame(rows, D, dtype=qkv.dtype, preload=np.full((rows, D), fill, qkv.dtype))
    else:
        dq, do = frames.framed(qkv), frames.out_frame(rows, D, dtype=qkv.dtype)
    _note(out, out=do)
    hip_check(getattr(lib(), name)(None, dq.ptr, do.ptr, n_images, tokens, heads, *args), name)
    return do.window()


def _bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.uint16)


def attention_bf16io(qkv_bits, n_images: int, tokens: int, heads: int, f32math: bool = False, q_scaled: bool = False,
                     q_rows: Optional[int] = None) -> np.ndarray:
    """vithip_attention_bf16io (bf16 MFMA), vithip_attention_bf16io_f32math (fp32 arithmetic) or, q_scaled,
    vithip_attention_bf16io_qscaled (the Q columns hold QSCALE * q) -> bf16 bits."""
    if q_scaled:
        return _attention("vithip_attention_bf16io_qscaled", _bits(qkv_bits), n_images, tokens, heads, 64, (q_rows or tokens,))
    return _attention("vithip_attention_bf16io_f32math" if f32math else "vithip_attention_bf16io", _bits(qkv_bits), n_images, tokens,
                      heads, 64, ())


def layernorm(x, gamma, beta, ldx: Optional[int] = None, ldy: Optional[int] = None, frames=None,
              out: Optional[dict] = None, eps=None, in_place: bool = False) -> np.ndarray:
    """vithip_layernorm_f32 (eps: vithip_layernorm_f32_eps).  ldx / ldy, frames, out: as for gemm(); the output frame is "y".
    in_place: y is x's own frame (y == x, ldy == ldx)."""
    x = _as_f32(x)
    rows, dim = x.shape
    F = frames or _Plain
    dg, db = F.framed(_as_f32(gamma)), F.framed(_as_f32(beta))
    if in_place:
        dx = dy = F.out_frame(rows, dim, ldx, preload=x)
    else:
        dx = F.framed(x, ldx)
        dy = F.out_frame(rows, dim, ldy)
    _note(out, y=dy)
    fn, e = _ln_fn("vithip_layernorm_f32", eps)
    hip_check(fn(None, dx.ptr, dx.ld, dy.ptr, dy.ld, dg.ptr, db.ptr, rows, dim, *e), "vithip_layernorm_f32")
    return dy.window()


def swiglu_raw(u_ptr, ldu: int, h_ptr, ldh: int, rows: int, H: int, bf16: bool = False) -> int:
    """vithip_swiglu_f32 / vithip_swiglu_bf16 on caller-owned device addresses; returns the HIP status (no exception)."""
    fn = lib().vithip_swiglu_bf16 if bf16 else lib().vithip_swiglu_f32
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int]
    return int(fn(None, u_ptr, ldu, h_ptr, ldh, rows, H))


def swiglu(u, H: int, in_place: bool = False, ldu: Optional[int] = None, ldh: Optional[int] = None, frames=None,
           out: Optional[dict] = None) -> np.ndarray:
    """vithip_swiglu_f32 (u float32) or vithip_swiglu_bf16 (u uint16 = bf16 bits): u [rows][2H] = gate | value -> h [rows][H].
    in_place: h is written over the gate half of u's own rows (ldh = ldu); the returned rows are then all 2H columns of u after the
    launch, [h | value].  ldu / ldh, frames, out: as for gemm(); the output frame is "h" (in place: u's frame)."""
    u = np.ascontiguousarray(u)
    bf16 = u.dtype == np.uint16
    if not bf16:
        u = _as_f32(u)
    rows, two_h = u.shape
    assert two_h == 2 * H, (u.shape, H)
    F = frames or _Plain
    du = F.framed(u, ldu)
    dh = du if in_place else F.out_frame(rows, H, ldh, u.dtype)
    _note(out, h=dh)
    hip_check(swiglu_raw(du.ptr, du.ld, dh.ptr, dh.ld, rows, H, bf16), "vithip_swiglu_bf16" if bf16 else "vithip_swiglu_f32")
    return dh.window()


def tap_block(images: int, tokens: int, dim: int, layout) -> tuple:
    """Shape of one image's block of vithip_tap_f32 for `layout` ("cls" | "tokens" | "patches" | "map" or a VITHIP_TAP_* integer)."""
    k = TAP_KINDS[layout] if isinstance(layout, str) else int(layout)
    return {0: (dim,), 1: (tokens, dim), 2: (tokens - 1, dim), 3: (dim, tokens - 1)}[k]


def tap(x, gamma, beta, images: int, tokens: int, layout, ldx: Optional[int] = None, out_image_stride: Optional[int] = None,
        frames=None, out: Optional[dict] = None, d_out: Optional[int] = None, eps=None, prefix: Optional[int] = None) -> Optional[np.ndarray]:
    """vithip_tap_f32: x [images * tokens][dim] -> per image the block of `layout`; gamma = beta = None copies the rows unnormalised.
    ldx, frames, out: as for layernorm(); the output frame "out" has one row per image, a block wide, out_image_stride apart.
    d_out: a raw device address to write to instead (out_image_stride is then required); nothing is returned.
    prefix: the rows in front of an image's patch rows (1 + register tokens) -- vithip_tap_f32_prefix_eps; None: the entries without."""
    if prefix is not None:
        return _tap_prefix(x, gamma, beta, images, tokens, layout, int(prefix), out_image_stride, d_out, eps)
    x = _as_f32(x)
    rows, dim = x.shape
    k = TAP_KINDS[layout] if isinstance(layout, str) else int(layout)
    F = frames or _Plain
    dx = F.framed(x, ldx)
    dg = F.framed(_as_f32(gamma)) if gamma is not None else None
    db = F.framed(_as_f32(beta)) if beta is not None else None
    fn, e = _ln_fn("vithip_tap_f32", eps)
    args = (dg.ptr if dg else None, db.ptr if db else None, images, tokens, dim, k) + e
    if d_out is not None:
        hip_check(fn(None, dx.ptr, dx.ld, d_out, out_image_stride, *args), "vithip_tap_f32")
        hip_check(lib().vithip_device_sync(), "sync")
        return None
    shape = tap_block(images, tokens, dim, k)
    do = F.out_frame(images, int(np.prod(shape)), out_image_stride)
    _note(out, out=do)
    hip_check(fn(None, dx.ptr, dx.ld, do.ptr, do.ld, *args), "vithip_tap_f32")
    return do.window().reshape((images,) + shape)


def _tap_prefix(x, gamma, beta, images, tokens, layout, prefix, out_image_stride, d_out, eps):
    x = _as_f32(x)
    rows, dim = x.shape
    k = TAP_KINDS[layout] if isinstance(layout, str) else int(layout)
    L = lib()
    L.vithip_tap_f32_prefix_eps.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p] + [C.c_int] * 5 + [C.c_double]
    dx = DeviceArray.from_numpy(x)
    dg = DeviceArray.from_numpy(_as_f32(gamma)) if gamma is not None else None
    db = DeviceArray.from_numpy(_as_f32(beta)) if beta is not None else None
    args = (dg.ptr if dg else None, db.ptr if db else None, images, tokens, prefix, dim, k, float(1e-6 if eps is None else eps))  # VITHIP_LN_EPS
    if d_out is not None:
        hip_check(L.vithip_tap_f32_prefix_eps(None, dx.ptr, dim, d_out, out_image_stride, *args), "vithip_tap_f32_prefix_eps")
        hip_check(L.vithip_device_sync(), "sync")
        return None
    shape = {0: (dim,), 1: (tokens, dim), 2: (tokens - prefix, dim), 3: (dim, tokens - prefix)}[k]
    block = int(np.prod(shape))
    do = DeviceArray((images, block if out_image_stride is None else out_image_stride))
    hip_check(L.vithip_tap_f32_prefix_eps(None, dx.ptr, dim, do.ptr, do.shape[1], *args), "vithip_tap_f32_prefix_eps")
    return do.numpy()[:, :block].reshape((images,) + shape)


def pos_resample_table(mode, n_in: int, n_out: int):
    """vithip_pos_resample_table (host only, no GPU): the table of one axis as (first [n_out] int32, count [n_out] int32, weights
    [n_out][widest] float32); the source index of tap k is clamp(first + k, 0, n_in - 1).  VitError when the library refuses."""
    L, m = lib(), _pos_mode(mode)
    taps = L.vithip_pos_resample_table(m, n_in, n_out, None, None, None, 0)
    if taps < 1:
        raise VitError(f"vithip_pos_resample_table refused mode {m}, {n_in} -> {n_out} ({taps})")
    first, count = np.empty(n_out, np.int32), np.empty(n_out, np.int32)
    weights = np.empty((n_out, taps), np.float32)
    got = L.vithip_pos_resample_table(m, n_in, n_out, first.ctypes.data_as(C.POINTER(C.c_int)), count.ctypes.data_as(C.POINTER(C.c_int)),
                                      weights.ctypes.data_as(f32p), taps)
    if got != taps:
        raise VitError(f"vithip_pos_resample_table: {got} after a sizing call that said {taps}")
    return first, count, weights


def pos_resample(pos, g_dst: int, mode, g_src: Optional[int] = None, guard: int = 0, fill_bits: int = 0, dst_offset: int = 0,
                 out: Optional[dict] = None) -> np.ndarray:
    """vithip_pos_resample_f32: pos [1 + g_src^2][dim] -> [1 + g_dst^2][dim] (g_src defaults to the grid pos holds).
    guard, fill_bits: dst gets `guard` floats either side of it and every float of the allocation is preset to the bit pattern
    fill_bits; `out` receives the allocation as the call left it under "raw".  dst_offset: floats dst is shifted by (a misaligned
    destination)."""
    pos = _as_f32(pos)
    T, dim = pos.shape
    if g_src is None:
        g_src = int(round((T - 1) ** 0.5))
    n = (1 + g_dst * g_dst) * dim if g_dst > 0 else dim
    raw = np.full(2 * guard + dst_offset + n, fill_bits, np.uint32).view(np.float32)
    d_src, d_raw = DeviceArray.from_numpy(pos), DeviceArray.from_numpy(raw)
    try:
        hip_check(lib().vithip_pos_resample_f32(None, d_src.ptr, g_src, d_raw.ptr + 4 * (guard + dst_offset), g_dst, dim, _pos_mode(mode)),
                  "vithip_pos_resample_f32")
        raw = d_raw.numpy()
    finally:
        d_src.free()
        d_raw.free()
    if out is not None:
        out["raw"] = raw
    return raw[guard + dst_offset:guard + dst_offset + n].reshape(-1, dim).copy()


def layernorm_pool(x, gamma, beta, images: int, tokens: int, first_tok: int = 1, l2_normalize: bool = False, eps=None) -> np.ndarray:
    """vithip_layernorm_pool_f32: x [images * tokens][ld >= dim] (dim = len(gamma)) -> [images][dim], the mean over tokens
    first_tok.. of the LayerNorm rows, optionally L2-normalised.  Columns dim.. of x are padding (ldx > dim)."""
    x = _as_f32(x)
    rows, ldx = x.shape
    dim = int(np.asarray(gamma).size)
    assert rows == images * tokens and ldx >= dim
    L = lib()
    dx, dg, db = DeviceArray.from_numpy(x), DeviceArray.from_numpy(_as_f32(gamma)), DeviceArray.from_numpy(_as_f32(beta))
    do = DeviceArray((images, dim))
    ws = DeviceArray((max(1, L.vithip_layernorm_pool_f32_workspace_floats(images, tokens, first_tok, dim)),))
    fn, e = _ln_fn("vithip_layernorm_pool_f32", eps)
    hip_check(fn(None, dx.ptr, ldx, do.ptr, dim, dg.ptr, db.ptr, images, tokens, first_tok, dim, int(l2_normalize), ws.ptr, *e),
              "vithip_layernorm_pool_f32")
    return do.numpy()


def pool_layernorm(x, gamma, beta, images: int, tokens: int, first_tok: int = 1, ldx: Optional[int] = None, ldo: Optional[int] = None,
                   frames=None, out: Optional[dict] = None, override: Optional[dict] = None, out_offset: int = 0, eps=None) -> np.ndarray:
    """vithip_pool_layernorm_f32: x [images * tokens][dim] -> [images][dim], the LayerNorm of the mean over tokens first_tok..;
    gamma = beta = None stores the mean itself.  ldx / ldo, frames, out: as for layernorm(); the output frames are "out" (a row per
    image) and "ws" (the workspace, exactly the declared floats).  override: C arguments by name (x, ldx, out, ldo, gamma, beta,
    images, tokens, first_tok, dim, workspace) that replace the ones derived here, for the refusal tests; out_offset: elements by
    which the output's base is moved off its alignment."""
    x = _as_f32(x)
    rows, dim = x.shape
    assert rows == images * tokens
    L = lib()
    F = frames or _Plain
    dx = F.framed(x, ldx)
    dg = F.framed(_as_f32(gamma)) if gamma is not None else None
    db = F.framed(_as_f32(beta)) if beta is not None else None
    do = F.out_frame(images, dim, ldo, offset=out_offset)
    ws = F.out_frame(1, max(1, L.vithip_pool_layernorm_f32_workspace_floats(images, tokens, first_tok, dim)))
    _note(out, out=do, ws=ws)
    a = dict(x=dx.ptr, ldx=dx.ld, out=do.ptr, ldo=do.ld, gamma=dg.ptr if dg else None, beta=db.ptr if db else None, images=images,
             tokens=tokens, first_tok=first_tok, dim=dim, workspace=ws.ptr)
    a.update(override or {})
    fn, e = _ln_fn("vithip_pool_layernorm_f32", eps)
    hip_check(fn(None, *a.values(), *e), "vithip_pool_layernorm_f32")
    return do.window()


def l2_normalize_rows(x) -> np.ndarray:
    """vithip_l2_normalize_rows_f32: row / max(||row||_2, 1e-12)."""
    x = _as_f32(x)
    rows, dim = x.shape
    dx = DeviceArray.from_numpy(x)
    hip_check(lib().vithip_l2_normalize_rows_f32(None, dx.ptr, dim, rows, dim), "vithip_l2_normalize_rows_f32")
    return dx.numpy()


def ln_fold_weights_f32(W, bias, gamma, beta):
    """vithip_ln_fold_weights_f32 -> (Wf [N][K], colsum [N], bias_f [N])."""
    W, bias, gamma, beta = _as_f32(W), _as_f32(bias), _as_f32(gamma), _as_f32(beta)
    N, K = W.shape
    dW, db, dg, dbe = (DeviceArray.from_numpy(a) for a in (W, bias, gamma, beta))
    dWf, dcs, dbf = DeviceArray((N, K)), DeviceArray((N,)), DeviceArray((N,))
    lib().vithip_ln_fold_weights_f32.argtypes = [C.c_void_p] * 8 + [C.c_int, C.c_int]
    hip_check(lib().vithip_ln_fold_weights_f32(None, dW.ptr, db.ptr, dg.ptr, dbe.ptr, dWf.ptr, dcs.ptr, dbf.ptr, N, K),
              "vithip_ln_fold_weights_f32")
    return dWf.numpy(), dcs.numpy(), dbf.numpy()


def ln_fold_weights_f32_centered(W, bias, gamma, beta):
    """vithip_ln_fold_weights_f32_centered -> (Wc [N][K] = gamma * W - column mean, residual colsum [N], bias_f [N]): pass Wc and bias_f
    to gemm(..., ln=(rows, None))."""
    W, bias, gamma, beta = _as_f32(W), _as_f32(bias), _as_f32(gamma), _as_f32(beta)
    N, K = W.shape
    dW, db, dg, dbe = (DeviceArray.from_numpy(a) for a in (W, bias, gamma, beta))
    dWf, dcs, dbf = DeviceArray((N, K)), DeviceArray((N,)), DeviceArray((N,))
    lib().vithip_ln_fold_weights_f32_centered.argtypes = [C.c_void_p] * 8 + [C.c_int, C.c_int]
    hip_check(lib().vithip_ln_fold_weights_f32_centered(None, dW.ptr, db.ptr, dg.ptr, dbe.ptr, dWf.ptr, dcs.ptr, dbf.ptr, N, K),
              "vithip_ln_fold_weights_f32_centered")
    return dWf.numpy(), dcs.numpy(), dbf.numpy()


def rowstats_f32(x, ldx: Optional[int] = None, frames=None, out: Optional[dict] = None, eps=None) -> np.ndarray:
    """vithip_rowstats_f32 -> [rows][2] = (rstd, mean).  ldx, frames, out: as for gemm(); the output frame is "rows"."""
    x = _as_f32(x)
    rows, dim = x.shape
    L = lib()
    L.vithip_rowstats_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int]
    F = frames or _Plain
    dx, dr = F.framed(x, ldx), F.out_frame(rows, 2)
    _note(out, rows=dr)
    fn, e = _ln_fn("vithip_rowstats_f32", eps)
    hip_check(fn(None, dx.ptr, dx.ld, dr.ptr, rows, dim, *e), "vithip_rowstats_f32")
    return dr.window()


def gather_rows(src, src_stride: Optional[int] = None, dst_stride: Optional[int] = None, frames=None, out: Optional[dict] = None,
                rows: Optional[int] = None, width: Optional[int] = None, null: str = "") -> np.ndarray:
    """vithip_gather_rows_f32: dst[r][0..width) = src[r * src_stride .. + width).  src [rows][width] is placed with the leading
    dimension src_stride (its other columns are padding); the output frame is "dst".  rows / width: the counts passed (default:
    src's shape); null: "src" or "dst" passes that pointer as NULL (refusal tests)."""
    src = _as_f32(src)
    L = lib()
    L.vithip_gather_rows_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int]
    F = frames or _Plain
    ds, dd = F.framed(src), F.out_frame(src.shape[0], src.shape[1])
    if src_stride is not None and src_stride >= src.shape[1]:
        ds = F.framed(src, src_stride)
    if dst_stride is not None and dst_stride >= src.shape[1]:
        dd = F.out_frame(src.shape[0], src.shape[1], dst_stride)
    _note(out, dst=dd)
    hip_check(L.vithip_gather_rows_f32(None, None if null == "src" else ds.ptr, ds.ld if src_stride is None else src_stride,
                                       None if null == "dst" else dd.ptr, dd.ld if dst_stride is None else dst_stride,
                                       src.shape[0] if rows is None else rows, src.shape[1] if width is None else width),
              "vithip_gather_rows_f32")
    return dd.window()


def attention(qkv, n_images: int, tokens: int, heads: int) -> np.ndarray:
    return _attention("vithip_attention_f32", _as_f32(qkv), n_images, tokens, heads, 64, ())


def attention_rows(qkv, n_images: int, tokens: int, heads: int, q_rows: int, fill: float = 0.0, frames=None,
                   out: Optional[dict] = None) -> np.ndarray:
    """vithip_attention_f32_rows: the output buffer is pre-filled with `fill` to show which rows are written (with `frames`: the
    frame's sentinel instead, and `out` receives the frame "out")."""
    return _attention("vithip_attention_f32_rows", _as_f32(qkv), n_images, tokens, heads, 64, (q_rows,), fill, frames, out)


def attention_bf16io_rows(qkv_bits, n_images: int, tokens: int, heads: int, q_rows: int, q_scaled: bool = False, frames=None,
                          out: Optional[dict] = None) -> np.ndarray:
    """vithip_attention_bf16io_rows or, q_scaled, vithip_attention_bf16io_qscaled -> bf16 bits [n * tokens][heads * 64]; rows
    q_rows.. of every image keep what the buffer held (zeros, or the sentinel of `frames`); `out` receives the frame "out"."""
    name = "vithip_attention_bf16io_qscaled" if q_scaled else "vithip_attention_bf16io_rows"
    return _attention(name, _bits(qkv_bits), n_images, tokens, heads, 64, (q_rows,), 0, frames, out)


def qscale(head_dim: int) -> float:
    """vithip_qscale: (1/sqrt(head_dim)) * log2(e) as the fp32 value the kernels and the engine's fold use; 0.0 for a head_dim they
    refuse.  qscale(64) == QSCALE."""
    return float(lib().vithip_qscale(int(head_dim)))


def attention_hd(qkv, n_images: int, tokens: int, heads: int, head_dim: int, q_rows: Optional[int] = None, fill: float = 0.0,
                 frames=None, out: Optional[dict] = None) -> np.ndarray:
    """vithip_attention_f32_hd: qkv [n_images * tokens][3 * heads * head_dim] fp32 -> [n_images * tokens][heads * head_dim]; only
    the first q_rows (default: all) query rows of every image are written, the others keep `fill` (with `frames`: the frame's
    sentinel, and `out` receives the frame "out")."""
    return _attention("vithip_attention_f32_hd", _as_f32(qkv), n_images, tokens, heads, head_dim,
                      (head_dim, tokens if q_rows is None else q_rows), fill, frames, out)


def attention_split(qkv, n_images: int, tokens: int, heads: int, q_rows: Optional[int] = None, fill: float = 0.0, frames=None,
                    out: Optional[dict] = None) -> np.ndarray:
    """vithip_attention_f32_split: attention_hd() at head_dim 64 with both products on the bf16 matrix pipe (three-piece split)."""
    return _attention("vithip_attention_f32_split", _as_f32(qkv), n_images, tokens, heads, 64,
                      (64, tokens if q_rows is None else q_rows), fill, frames, out)


def attention_bf16io_hd(qkv_bits, n_images: int, tokens: int, heads: int, head_dim: int, q_rows: Optional[int] = None,
                        q_scaled: bool = False, fill: int = 0, frames=None, out: Optional[dict] = None) -> np.ndarray:
    """vithip_attention_bf16io_hd: the same on bf16 bits (uint16); q_scaled: the Q columns hold qscale(head_dim) * q."""
    return _attention("vithip_attention_bf16io_hd", _bits(qkv_bits), n_images, tokens, heads, head_dim,
                      (head_dim, tokens if q_rows is None else q_rows, int(q_scaled)), fill, frames, out)


def _cls_attention(name, qkv, n_images, tokens, heads, head_dim, head_mean, q_scaled, ld_out, fill):
    """The class-row entry `name`(stream, qkv, row stride, out, ld_out, n_images, tokens, heads[, head_dim], head_mean[, q_scaled]):
    head_dim goes to the _hd entries, q_scaled (None for fp32) to the bf16 ones."""
    assert qkv.shape == (n_images * tokens, 3 * heads * head_dim)
    args = ((head_dim,) if name.endswith("_hd") else ()) + (int(head_mean),) + (() if q_scaled is None else (int(q_scaled),))
    row = tokens if head_mean else heads * tokens
    ld = row if ld_out is None else int(ld_out)
    do = DeviceArray((n_images, ld)) if fill is None else DeviceArray.from_numpy(np.full((n_images, ld), fill, np.float32))
    dq = DeviceArray.from_numpy(qkv)
    hip_check(getattr(lib(), name)(None, dq.ptr, 3 * heads * head_dim, do.ptr, ld, n_images, tokens, heads, *args), name)
    res = do.numpy()
    if ld_out is not None:
        return res
    return res if head_mean else res.reshape(n_images, heads, tokens)


def cls_attention(qkv, n_images: int, tokens: int, heads: int, head_mean: bool = False, ld_out: Optional[int] = None,
                  fill: Optional[float] = None) -> np.ndarray:
    """vithip_cls_attention_f32: qkv [n_images * tokens][3 * heads * 64] fp32 -> the class rows' softmax [n][heads][tokens], or
    [n][tokens] with head_mean.  ld_out (>= the row): the raw [n][ld_out] buffer comes back, pre-filled with `fill`, to show what
    the kernel wrote."""
    return _cls_attention("vithip_cls_attention_f32", _as_f32(qkv), n_images, tokens, heads, 64, head_mean, None, ld_out, fill)


def cls_attention_bf16(qkv_bits, n_images: int, tokens: int, heads: int, head_mean: bool = False, q_scaled: bool = False,
                       ld_out: Optional[int] = None, fill: Optional[float] = None) -> np.ndarray:
    """vithip_cls_attention_bf16: the same from bf16 bits (uint16); q_scaled: the Q columns hold QSCALE * q.  fp32 out."""
    return _cls_attention("vithip_cls_attention_bf16", _bits(qkv_bits), n_images, tokens, heads, 64, head_mean, q_scaled, ld_out, fill)


def cls_attention_hd(qkv, n_images: int, tokens: int, heads: int, head_dim: int, head_mean: bool = False, ld_out: Optional[int] = None,
                     fill: Optional[float] = None) -> np.ndarray:
    """vithip_cls_attention_f32_hd: cls_attention() for qkv [n_images * tokens][3 * heads * head_dim]."""
    return _cls_attention("vithip_cls_attention_f32_hd", _as_f32(qkv), n_images, tokens, heads, head_dim, head_mean, None, ld_out, fill)


def cls_attention_bf16_hd(qkv_bits, n_images: int, tokens: int, heads: int, head_dim: int, head_mean: bool = False,
                          q_scaled: bool = False, ld_out: Optional[int] = None, fill: Optional[float] = None) -> np.ndarray:
    """vithip_cls_attention_bf16_hd: the same from bf16 bits (uint16); q_scaled: the Q columns hold qscale(head_dim) * q."""
    return _cls_attention("vithip_cls_attention_bf16_hd", _bits(qkv_bits), n_images, tokens, heads, head_dim, head_mean, q_scaled,
                          ld_out, fill)


def patch_embed(cfg: ModelConfig, images, conv_w, conv_b, cls, pos) -> np.ndarray:
    images = _as_f32(images)
    n = images.shape[0]
    d = [DeviceArray.from_numpy(_as_f32(a)) for a in (images, conv_w, conv_b, cls, pos)]
    dx = DeviceArray((n * cfg.tokens, cfg.embed_dim))
    hip_check(lib().vithip_patch_embed_f32(None, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, dx.ptr, n,
                                           cfg.img_size, cfg.patch_size, cfg.in_chans, cfg.embed_dim),
              "vithip_patch_embed_f32")
    return dx.numpy().reshape(n, cfg.tokens, cfg.embed_dim)


def patch_embed_reg_raw(kind: str, images_ptr, conv_w_ptr, conv_b_ptr, prefix_ptr, pos_ptr, x_ptr, n: int, img_size: int,
                        patch_size: int, in_chans: int, embed_dim: int, registers: int, patches16_ptr=None) -> int:
    """vithip_patch_embed_f32_reg ("f32": the dispatching entry), _f32_general_reg ("general") or _bf16_reg ("bf16": conv_w_ptr holds
    bf16 bits, patches16_ptr the workspace) on raw device addresses; returns the launcher's code after the stream has drained."""
    L = lib()
    ints = (n, img_size, patch_size, in_chans, embed_dim, registers)
    if kind == "bf16":
        L.vithip_patch_embed_bf16_reg.argtypes = [C.c_void_p] * 8 + [C.c_int] * 6
        rc = L.vithip_patch_embed_bf16_reg(None, images_ptr, conv_w_ptr, conv_b_ptr, prefix_ptr, pos_ptr, x_ptr, patches16_ptr, *ints)
    else:
        fn = {"f32": L.vithip_patch_embed_f32_reg, "general": L.vithip_patch_embed_f32_general_reg}[kind]
        fn.argtypes = [C.c_void_p] * 7 + [C.c_int] * 6
        rc = fn(None, images_ptr, conv_w_ptr, conv_b_ptr, prefix_ptr, pos_ptr, x_ptr, *ints)
    hip_check(L.vithip_device_sync(), "sync")
    return int(rc)


def patch_embed_reg(cfg: ModelConfig, images, conv_w, conv_b, prefix, pos, kind: str = "f32", registers: Optional[int] = None,
                    guard: int = 0, fill: float = 0.0):
    """The embedding of a register model: prefix [(1 + registers)][D] (class token, then registers), pos [(patches + 1)][D];
    registers defaults to cfg.num_register_tokens.  kind: "f32" | "general" | "bf16" (patch_embed_reg_raw; "bf16" rounds conv_w here).
    Returns x [n][1 + registers + patches][D]; with guard > 0, (x, front, back): x lies between two runs of `guard` floats preset
    to `fill` like x itself, returned as they are afterwards."""
    images = _as_f32(images)
    n, R, D = images.shape[0], cfg.num_register_tokens if registers is None else int(registers), cfg.embed_dim
    T = 1 + max(R, 0) + cfg.patches
    d = [DeviceArray.from_numpy(_as_f32(a)) for a in (images, conv_b, prefix, pos)]
    w = _as_f32(conv_w).reshape(D, -1)
    dw = DeviceArray.from_numpy(to_bf16_bits(w) if kind == "bf16" else w)
    dp = DeviceArray((n * cfg.patches, cfg.patch_dim), np.uint16) if kind == "bf16" else None
    assert guard % 4 == 0, "x stays 16-byte aligned"
    dx = DeviceArray.from_numpy(np.full(2 * guard + n * T * D, fill, np.float32))
    hip_check(patch_embed_reg_raw(kind, d[0].ptr, dw.ptr, d[1].ptr, d[2].ptr, d[3].ptr, dx.ptr + 4 * guard, n, cfg.img_size, cfg.patch_size,
                                  cfg.in_chans, D, R, dp.ptr if dp else None), f"vithip_patch_embed_{kind}_reg")
    flat = dx.numpy()
    x = flat[guard:guard + n * T * D].reshape(n, T, D)
    return (x, flat[:guard], flat[guard + n * T * D:]) if guard else x


def patch_embed_general_raw(images_ptr, conv_w_ptr, conv_b_ptr, cls_ptr, pos_ptr, x_ptr, n: int, img_size: int, patch_size: int,
                            in_chans: int, embed_dim: int, general: bool = True) -> int:
    """vithip_patch_embed_f32_general (general=False: the dispatching vithip_patch_embed_f32) on raw device addresses; returns the
    launcher's code (0, or a hipError_t: 1 = hipErrorInvalidValue) after the stream has drained."""
    L = lib()
    fn = L.vithip_patch_embed_f32_general if general else L.vithip_patch_embed_f32
    rc = int(fn(None, images_ptr, conv_w_ptr, conv_b_ptr, cls_ptr, pos_ptr, x_ptr, n, img_size, patch_size, in_chans, embed_dim))
    hip_check(L.vithip_device_sync(), "sync")
    return rc


def patch_embed_general(cfg: ModelConfig, images, conv_w, conv_b, cls, pos) -> np.ndarray:
    """vithip_patch_embed_f32_general: the 8-byte implicit GEMM for any even geometry, always the general kernel."""
    images = _as_f32(images)
    n = images.shape[0]
    d = [DeviceArray.from_numpy(_as_f32(a)) for a in (images, conv_w, conv_b, cls, pos)]
    dx = DeviceArray((n * cfg.tokens, cfg.embed_dim))
    hip_check(patch_embed_general_raw(d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, dx.ptr, n, cfg.img_size, cfg.patch_size,
                                      cfg.in_chans, cfg.embed_dim), "vithip_patch_embed_f32_general")
    return dx.numpy().reshape(n, cfg.tokens, cfg.embed_dim)


def fold_layer_scale_raw(cfg: ModelConfig, weights, scales, count: Optional[int] = None, scale_count: Optional[int] = None) -> int:
    """vit_weights_fold_layer_scale on the arrays themselves, IN PLACE (float32, C-contiguous; None = an absent tensor; weights / scales
    None = a NULL array); returns the C call's code: 0, or nonzero for a refused call, which has written nothing."""
    for a in list(weights or []) + list(scales or []):
        assert a is None or (a.dtype == np.float32 and a.flags.c_contiguous and a.flags.writeable), "float32, C-contiguous, writable"
    w_arr, _kw = networks_from(weights) if weights is not None else (None, None)
    s_arr, _ks = networks_from(scales) if scales is not None else (None, None)
    return int(lib().vit_weights_fold_layer_scale(C.byref(CConfig.of(cfg)), w_arr, len(weights or []) if count is None else count,
                                                  s_arr, len(scales or []) if scale_count is None else scale_count))


def fold_batchnorm_raw(weight, bias, classes: int, in_features: int, gamma, beta, mean, var, eps: float) -> int:
    """vit_dense_head_fold_batchnorm on the arrays themselves, IN PLACE (float32, C-contiguous; None = a NULL pointer), every argument
    passed through unchecked: returns the C return code (0, or nonzero with nothing written)."""
    ptr = lambda a: None if a is None else a.ctypes.data_as(f32p)
    return int(lib().vit_dense_head_fold_batchnorm(ptr(weight), ptr(bias), int(classes), int(in_features), ptr(gamma), ptr(beta), ptr(mean),
                                                   ptr(var), float(eps)))


def fold_batchnorm(weight, bias, gamma, beta, mean, var, eps: float = 1e-5):
    """An eval-mode BatchNorm over the input channels (mmseg BNHead: decode_head.bn.weight / .bias / .running_mean / .running_var)
    folded into a dense head's weight [classes][in_features] (conv_seg.weight, its trailing 1 x 1 dropped) and bias [classes]: returns
    new (weight, bias) float32 arrays for Engine.set_dense_head.  No GPU involved."""
    w = np.array(weight, np.float32, order="C")
    b = np.array(bias, np.float32, order="C").reshape(-1)
    w = w.reshape(b.size, -1)
    bn = [np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1)) for a in (gamma, beta, mean, var)]
    if any(a.size != w.shape[1] for a in bn):
        raise VitError(f"fold_batchnorm: the BatchNorm has {[a.size for a in bn]} channels, the weight {w.shape[1]} input features")
    rc = fold_batchnorm_raw(w, b, w.shape[0], w.shape[1], *bn, eps)
    if rc:
        raise VitError(f"vit_dense_head_fold_batchnorm refused the call ({rc}): non-finite values, eps < 0 or var + eps <= 0")
    return w, b


def fold_layer_scale(cfg: ModelConfig, weights: Sequence[np.ndarray], scales: Sequence[np.ndarray]) -> list:
    """LayerScale folded into out_proj and fc2 (vit_weights_fold_layer_scale): scales = [ls1 of layer 0, ls2 of layer 0, ls1 of layer
    1, ...], each [embed_dim].  Returns the folded tensors as new arrays (the caller's stay as they are): ordinary weights for
    Engine.load_weights / WeightImage.build."""
    folded = [np.array(w, dtype=np.float32, order="C") for w in weights]
    rc = fold_layer_scale_raw(cfg, folded, [np.array(s, dtype=np.float32, order="C").reshape(-1) for s in scales])
    if rc != 0:
        raise VitError(f"vit_weights_fold_layer_scale refused the call ({rc}): {len(folded)} tensors and {len(scales)} scales for depth "
                       f"{cfg.depth}; every tensor and scale must be present, of the model's size and finite")
    return folded


def patch_embed_bf16(cfg: ModelConfig, images, conv_w, conv_b, cls, pos, implicit: bool = False) -> np.ndarray:
    """vithip_patch_embed_bf16 (two passes) or vithip_patch_embed_bf16_implicit (one implicit GEMM over the NCHW pixels):
    conv weight given in fp32 and rounded to bf16 here (as the engine does on upload)."""
    images = _as_f32(images)
    n = images.shape[0]
    L = lib()
    if implicit:
        L.vithip_patch_embed_bf16_implicit.argtypes = [C.c_void_p] * 7 + [C.c_int] * 5
        d = [DeviceArray.from_numpy(_as_f32(a)) for a in (images, conv_b, cls, pos)]
        dw = DeviceArray.from_numpy(to_bf16_bits(_as_f32(conv_w).reshape(cfg.embed_dim, -1)))
        dx = DeviceArray((n * cfg.tokens, cfg.embed_dim))
        hip_check(L.vithip_patch_embed_bf16_implicit(None, d[0].ptr, dw.ptr, d[1].ptr, d[2].ptr, d[3].ptr, dx.ptr, n, cfg.img_size,
                                                     cfg.patch_size, cfg.in_chans, cfg.embed_dim), "vithip_patch_embed_bf16_implicit")
        return dx.numpy().reshape(n, cfg.tokens, cfg.embed_dim)
    L.vithip_patch_embed_bf16.argtypes = [C.c_void_p] * 8 + [C.c_int] * 5
    d = [DeviceArray.from_numpy(_as_f32(a)) for a in (images, conv_b, cls, pos)]
    dw = DeviceArray.from_numpy(to_bf16_bits(_as_f32(conv_w).reshape(cfg.embed_dim, -1)))
    dx = DeviceArray((n * cfg.tokens, cfg.embed_dim))
    dp = DeviceArray((n * cfg.patches, cfg.patch_dim), np.uint16)
    hip_check(L.vithip_patch_embed_bf16(None, d[0].ptr, dw.ptr, d[1].ptr, d[2].ptr, d[3].ptr, dx.ptr, dp.ptr, n,
                                        cfg.img_size, cfg.patch_size, cfg.in_chans, cfg.embed_dim), "vithip_patch_embed_bf16")
    return dx.numpy().reshape(n, cfg.tokens, cfg.embed_dim)


def softmax_top1(logits, ld_logits: Optional[int] = None, ld_probs: Optional[int] = None, want_label: bool = True,
                 want_prob: bool = True, frames=None, out: Optional[dict] = None):
    """vithip_softmax_top1_f32 -> (probs, labels, top-1 probabilities).  ld_logits / ld_probs, frames, out: as for gemm(); the
    output frames are "probs", "label" and "prob".  want_label / want_prob False: that pointer is passed as NULL (its frame is
    still made, and must stay untouched); the value returned for it is None."""
    logits = _as_f32(logits)
    rows, classes = logits.shape
    F = frames or _Plain
    dl = F.framed(logits, ld_logits)
    dp = F.out_frame(rows, classes, ld_probs)
    dlab = F.out_frame(rows, 1, dtype=np.int32)
    dpr = F.out_frame(rows, 1)
    _note(out, probs=dp, label=dlab, prob=dpr)
    hip_check(lib().vithip_softmax_top1_f32(None, dl.ptr, dl.ld, dp.ptr, dp.ld, dlab.ptr if want_label else None,
                                            dpr.ptr if want_prob else None, rows, classes), "vithip_softmax_top1_f32")
    return dp.window(), dlab.window().reshape(rows) if want_label else None, dpr.window().reshape(rows) if want_prob else None


def softmax_topk(logits, k: int, score="prob", ld_logits: Optional[int] = None, ld_out: Optional[int] = None, guard: int = 0,
                 fill_bits: int = 0, out_offset: int = 0, out: Optional[dict] = None) -> np.ndarray:
    """vithip_softmax_topk_f32 -> the records [rows][2k] int32 (split_topk() takes them apart).  ld_logits (>= classes): the rows
    of logits are laid out at that step, the pad columns preset to fill_bits; ld_out (>= 2k): 32-bit words per output row.
    guard, fill_bits: the records get `guard` words either side of them and every word of the allocation is preset to the bit pattern
    fill_bits; out_offset: words the records are shifted by (a misaligned destination).  `out` receives the output allocation as the
    call left it under "raw" and the logits allocation as the call left it under "logits_raw" (uint32 views of both under the
    same names + "_before" as they were uploaded)."""
    logits = _as_f32(logits)
    rows, classes = logits.shape
    ldl = classes if ld_logits is None else int(ld_logits)
    ldo = 2 * int(k) if ld_out is None else int(ld_out)
    src = np.full((rows, max(ldl, 1)), fill_bits, np.uint32).view(np.float32)
    if ldl >= classes:
        src[:, :classes] = logits
    else:  # a leading dimension the launcher must refuse: it never reads the buffer
        src = logits.copy()
    raw = np.full(2 * guard + out_offset + rows * max(ldo, 1), fill_bits, np.uint32)
    d_src, d_raw = DeviceArray.from_numpy(src), DeviceArray.from_numpy(raw)
    try:
        hip_check(lib().vithip_softmax_topk_f32(None, d_src.ptr, ldl, d_raw.ptr + 4 * (guard + out_offset), ldo, rows, classes, int(k),
                                                _score(score)), "vithip_softmax_topk_f32")
        after, src_after = d_raw.numpy(), d_src.numpy()
    finally:
        d_src.free()
        d_raw.free()
    if out is not None:
        out.update(raw=after, raw_before=raw, logits_raw=src_after.view(np.uint32), logits_raw_before=src.view(np.uint32))
    lo = guard + out_offset
    return after[lo:lo + rows * ldo].reshape(rows, ldo)[:, :2 * int(k)].copy().view(np.int32)


def dense_upsample_argmax_raw(logits_ptr, ld_logits: int, image_stride: int, out_ptr, out_image_stride: int, images: int, g: int,
                              classes: int, out_h: int, out_w: int) -> int:
    """vithip_dense_upsample_argmax_f32 on raw addresses, every argument passed through unchecked: returns the HIP error code."""
    return int(lib().vithip_dense_upsample_argmax_f32(None, logits_ptr, int(ld_logits), int(image_stride), out_ptr, int(out_image_stride),
                                                      int(images), int(g), int(classes), int(out_h), int(out_w)))


def dense_upsample_argmax(logits, out_h: int, out_w: int, ld_logits: Optional[int] = None, image_rows: Optional[int] = None,
                          out_ld_words: Optional[int] = None, pad_value: float = 0.0, frames=None, out: Optional[dict] = None) -> np.ndarray:
    """vithip_dense_upsample_argmax_f32: logits [n][g * g][classes] -> labels uint8 [n][out_h][out_w].
    ld_logits (>= classes): floats from one cell's row to the next; image_rows (>= g * g): rows from one image to the next, the rows
    behind an image's g * g holding pad_value; out_ld_words: 32-bit words from one image's labels to the next (the byte stride is 4 x
    that; default: out_h * out_w rounded up to a word).  frames: who allocates (default: exact buffers; tests/strided.py: guarded,
    sentinel-filled frames -- the labels then sit in an int32 frame of one row per image); `out` receives the frames "logits" and
    "labels" (before the launch: a refused call leaves them to be inspected)."""
    logits = _as_f32(logits)
    n, P, classes = logits.shape
    g = int(round(P ** 0.5))
    assert g * g == P, P
    rows = P if image_rows is None else int(image_rows)
    src = np.full((n, rows, classes), pad_value, np.float32)
    src[:, :P] = logits
    F = frames or _Plain
    dL = F.framed(src.reshape(n * rows, classes), ld_logits)
    words = (out_h * out_w + 3) // 4
    dO = F.out_frame(n, words, out_ld_words, dtype=np.int32)
    _note(out, logits=dL, labels=dO)
    hip_check(dense_upsample_argmax_raw(dL.ptr, dL.ld, rows * dL.ld, dO.ptr, 4 * dO.ld, n, g, classes, out_h, out_w),
              "vithip_dense_upsample_argmax_f32")
    return np.ascontiguousarray(dO.window()).view(np.uint8)[:, :out_h * out_w].reshape(n, out_h, out_w).copy()


def dense_grid(logits) -> np.ndarray:
    """vithip_dense_grid_f32: logits [n][g * g][classes] -> fp32 [n][classes][g][g], the transpose."""
    logits = _as_f32(logits)
    n, P, classes = logits.shape
    g = int(round(P ** 0.5))
    assert g * g == P, P
    d_src, d_out = DeviceArray.from_numpy(logits), DeviceArray((n, classes, g, g))
    hip_check(lib().vithip_dense_grid_f32(None, d_src.ptr, classes, P * classes, d_out.ptr, P * classes, n, g, classes), "vithip_dense_grid_f32")
    return d_out.numpy()


def _norm_consts(mean, std, chans: int):
    """mean / std as the host float arrays of `chans` entries the C-ABI reads (None stays NULL)."""
    out = []
    for v in (mean, std):
        if v is None:
            out.append(None)
            continue
        v = np.ascontiguousarray(v, np.float32).reshape(-1)
        if v.size != chans:
            raise ValueError(f"expected {chans} normalisation constants, got {v.size}")
        out.append((C.c_float * chans)(*v.tolist()))
    return out


def images_u8_to_f32(images, mean=IMAGENET_MEAN, std=IMAGENET_STD) -> np.ndarray:
    """vithip_images_u8_to_f32: uint8 images [n][S][S][C] -> [n][C][S][S] fp32, ((float)u / 255 - mean[c]) / std[c]."""
    images = np.ascontiguousarray(images, np.uint8)
    n, S, S2, chans = images.shape
    assert S == S2
    m, s = _norm_consts(mean, std, chans)
    ds, dd = DeviceArray.from_numpy(images), DeviceArray((n, chans, S, S))
    hip_check(lib().vithip_images_u8_to_f32(None, ds.ptr, dd.ptr, n, S, chans, m, s), "vithip_images_u8_to_f32")
    return dd.numpy()


def image_records(images):
    """(ptr, H, W) triples -> the CImageU8 array the C-ABI reads."""
    images = list(images)
    return (CImageU8 * len(images))(*[CImageU8(int(p) or None, int(h), int(w)) for p, h, w in images])


def host_image_records(images, chans: int):
    """A list of [H][W][C] uint8 arrays -> (contiguous arrays to keep alive, their CImageU8 records with host pointers)."""
    keep = []
    for im in images:
        im = np.ascontiguousarray(im, np.uint8)
        if im.ndim == 2:
            im = im[:, :, None]
        if im.ndim != 3 or im.shape[2] != chans:
            raise ValueError(f"expected [H][W][{chans}] uint8 images, got shape {im.shape}")
        keep.append(im)
    return keep, image_records((im.ctypes.data, im.shape[0], im.shape[1]) for im in keep)


def preproc_params(resize_shorter: int, mean, std, chans: int) -> CPreproc:
    pp = CPreproc()
    pp.resize_shorter = int(resize_shorter)
    for name, v in (("mean", mean), ("std", std)):
        v = np.ascontiguousarray(v, np.float32).reshape(-1)
        if v.size != chans:
            raise ValueError(f"expected {chans} normalisation constants, got {v.size}")
        for c in range(chans):
            getattr(pp, name)[c] = float(v[c])
    return pp


def images_u8_resize_crop_to_f32(images, img_size: int, resize_shorter: int, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                                 filter="bilinear") -> np.ndarray:
    """vithip_images_u8_resize_crop_to_f32_filter: a list of uint8 images [H][W][C] of any sizes -> [n][C][S][S] fp32, torchvision's
    Resize(resize_shorter) -> CenterCrop(img_size) -> ToTensor() -> Normalize(mean, std); filter: "bilinear" | "bicubic", Pillow's."""
    chans = 1 if np.asarray(images[0]).ndim == 2 else np.asarray(images[0]).shape[2]
    keep, _ = host_image_records(images, chans)
    m, s = _norm_consts(mean, std, chans)
    dev = [DeviceArray.from_numpy(im) for im in keep]
    recs = image_records((d.ptr, im.shape[0], im.shape[1]) for d, im in zip(dev, keep))
    dd = DeviceArray((len(keep), chans, img_size, img_size))
    hip_check(lib().vithip_images_u8_resize_crop_to_f32_filter(None, recs, len(keep), dd.ptr, img_size, chans, resize_shorter,
                                                               _resize_filter(filter), m, s), "vithip_images_u8_resize_crop_to_f32_filter")
    return dd.numpy()


def device_info(device: int = 0) -> dict:
    info = CDeviceInfo()
    hip_check(lib().vithip_get_device_info(device, C.byref(info)), "vithip_get_device_info")
    return {"name": info.name.decode(), "arch": info.arch.decode(), "compute_units": info.compute_units,
            "clock_mhz": info.clock_mhz, "wavefront": info.wavefront, "lds_per_block": info.lds_per_block,
            "hbm_bytes": int(info.hbm_bytes)}


# --------------------------------------------------------------------------------------------------
# The engine
# --------------------------------------------------------------------------------------------------
class Engine:
    """vit_engine (include/vit_engine.h): weights resident in HBM, batched forward."""

    def __init__(self, cfg: ModelConfig, max_batch: int = 256, device: int = 0, profile: bool = False,
                 lanes: int = 1, dtype: str = "f32", prune_last_layer: bool = False, use_graph: bool = False,
                 gemm_tile: int = 0, ln_fold: int = 0, gemm_handover_test: int = 0, host_first_piece: int = 0,
                 fp32_split: int = 0):
        self.cfg = cfg
        self._h = C.c_void_p()
        self._head_in = None  # floats per operand row of a head set by set_head(); None: the checkpoint's own head (embed_dim)
        cc = CConfig.of(cfg)
        opt = COptions(device, max_batch, 1 if profile else 0, lanes, {"f32": 0, "bf16": 1}[dtype],
                       1 if prune_last_layer else 0, 1 if use_graph else 0, gemm_tile, ln_fold, gemm_handover_test, host_first_piece,
                       fp32_split)
        rc = lib().vit_engine_create(C.byref(self._h), C.byref(cc), C.byref(opt))
        if rc != 0:
            msg = lib().vit_engine_last_error(self._h).decode() if self._h else "allocation failed"
            if self._h:
                lib().vit_engine_destroy(self._h)
                self._h = C.c_void_p()
            raise VitError(f"vit_engine_create failed ({rc}): {msg}")

    def _check(self, rc: int, what: str) -> None:
        if rc != 0:
            err = VitError(f"{what} failed ({rc}): {lib().vit_engine_last_error(self._h).decode()}")
            err.code = int(rc)  # VIT_ERR_*
            raise err

    def load_weights(self, weights: Sequence[np.ndarray], pos_from: Optional[int] = None, pos_mode="bicubic") -> None:
        """pos_from: the input size the checkpoint was trained at; its position embedding (tensor 3, for that size) is resampled on
        the device to this engine's cfg.img_size, pos_mode "bicubic" | "bicubic_aa" (vit_engine_load_weights_resampled)."""
        arr, keep = networks_from(weights)
        self._head_in = None  # every install restores the checkpoint's own head
        if pos_from is None:
            self._check(lib().vit_engine_load_weights(self._h, arr, len(weights)), "vit_engine_load_weights")
            return
        rs = CPosResample(int(pos_from), _pos_mode(pos_mode), 0)
        self._check(lib().vit_engine_load_weights_resampled(self._h, arr, len(weights), C.byref(rs)), "vit_engine_load_weights_resampled")

    def load_weight_image(self, img: "WeightImage") -> None:
        self._head_in = None
        self._check(lib().vit_engine_load_weight_image(self._h, C.byref(img.c)), "vit_engine_load_weight_image")

    def read_weight_image(self) -> "WeightImage":
        img = WeightImage()
        self._check(lib().vit_engine_read_weight_image(self._h, C.byref(img.c)), "vit_engine_read_weight_image")
        return img

    def copy_weights_from(self, other: "Engine", pos_mode=None) -> None:
        """pos_mode "bicubic" | "bicubic_aa": `other` may run at another img_size; its resident position embedding is resampled to
        this engine's (vit_engine_copy_weights_resampled).  None: the plain replication between equal configurations."""
        L = lib()
        self._head_in = None
        if pos_mode is not None:
            self._check(L.vit_engine_copy_weights_resampled(self._h, other._h, _pos_mode(pos_mode)), "vit_engine_copy_weights_resampled")
            return
        L.vit_engine_copy_weights.argtypes = [C.c_void_p, C.c_void_p]
        self._check(L.vit_engine_copy_weights(self._h, other._h), "vit_engine_copy_weights")

    # ---- the forward surface: vit_engine_<out>_<place><inp>, out "forward" | "features" | "cls_attention" | "intermediate" | "topk" | "dense", inp "" | "_u8" | "_images" ----
    def _call_args(self, out, inp, kind, l2_normalize, mean, std, resize_shorter, layers=None, norm=True, topk=None, dense=None) -> list:
        """What lies between n and the destination in the C call: the normalisation of the input kind, the spec of the output kind."""
        args = []
        if inp == "_u8":
            args += _norm_consts(mean, std, self.cfg.in_chans)
        elif inp == "_images":
            args.append(C.byref(preproc_params(resize_shorter, mean, std, self.cfg.in_chans)))
        if out == "intermediate":
            args.append(C.byref(intermediate_spec(layers, kind, norm, self.cfg.depth)))
        elif out == "topk":
            args.append(C.byref(topk))
        elif out == "dense":
            args.append(C.byref(dense))
        elif out != "forward":
            args.append(C.byref(feature_spec(kind, l2_normalize) if out == "features" else attention_spec(kind)))
        return args

    def _host(self, out, inp, images, kind=None, l2_normalize=False, mean=None, std=None, resize_shorter=None, layers=None,
              norm=True, topk=None, dense=None) -> np.ndarray:
        """A host-path call: per-image pointers (or records) in, per-image rows of a new array out."""
        if inp == "_images":
            keep, in_ptrs = host_image_records(images, self.cfg.in_chans)
        elif inp == "_u8":
            keep = np.ascontiguousarray(images, np.uint8)
            in_ptrs = (C.c_void_p * len(keep))(*[im.ctypes.data for im in keep])
        else:
            keep = _as_f32(images)
            in_ptrs = (f32p * len(keep))(*[im.ctypes.data_as(f32p) for im in keep])
        n = len(keep)
        args = self._call_args(out, inp, kind, l2_normalize, mean, std, resize_shorter, layers, norm, topk, dense)
        if out == "forward":
            shape = (n, self.cfg.num_classes)
        elif out == "dense":
            shape = self.dense_shape(n, dense)
        elif out == "topk":
            shape = (n, 2 * max(topk.k, 1))  # a spec the C side refuses still gets rows: the call must see its own arguments
        elif out == "intermediate":
            shape = self.intermediate_shape(n, layers, kind, norm)
        else:
            shape = self.feature_shape(n, kind, l2_normalize) if out == "features" else self.attention_shape(n, kind)
        rowp = i32p if out == "topk" else C.c_void_p if out == "dense" else f32p
        labels = out == "dense" and dense.kind == DENSE_KINDS["labels"]
        rows = np.empty(shape, np.int32 if out == "topk" else np.uint8 if labels else np.float32)
        out_ptrs = (rowp * n)(*[rows[i].ctypes.data if out == "dense" else rows[i].ctypes.data_as(rowp) for i in range(n)])
        name = f"vit_engine_{out}_host{inp}"
        self._check(getattr(lib(), name)(self._h, in_ptrs, n, *args, out_ptrs), name)
        return rows

    def _device(self, out, inp, images, n, dst, kind=None, l2_normalize=False, mean=None, std=None, resize_shorter=None, d_label=0,
                d_prob=0, stream=0, layers=None, norm=True, topk=None, dense=None) -> None:
        """A device-path call: raw HBM addresses (images: a list of (ptr, H, W) for "_images"), async on `stream`."""
        if inp == "_images":
            images = image_records(images)
            n = len(images)
        args = self._call_args(out, inp, kind, l2_normalize, mean, std, resize_shorter, layers, norm, topk, dense)
        top1 = [d_label or None, d_prob or None] if out == "forward" else []
        name = f"vit_engine_{out}_device{inp}"
        self._check(getattr(lib(), name)(self._h, images, n, *args, dst, *top1, stream or None), name)

    def forward(self, images: np.ndarray) -> np.ndarray:
        """Host path (the ViT_opencl-shaped one): per-image pointers in, per-image rows out."""
        return self._host("forward", "", images)

    def forward_device(self, d_images: int, n: int, d_probs: int, d_label: int = 0, d_prob: int = 0,
                       stream: int = 0) -> None:
        """Device-resident path: raw HBM addresses (e.g. torch data_ptr()), async on `stream`."""
        self._device("forward", "", d_images, n, d_probs, d_label=d_label, d_prob=d_prob, stream=stream)

    def forward_u8(self, images: np.ndarray, mean=IMAGENET_MEAN, std=IMAGENET_STD) -> np.ndarray:
        """Host path from 8-bit pixels: images [n][S][S][C] uint8 (as decoders write them), normalised on the device by
        ((float)u / 255 - mean[c]) / std[c]; per-image pointers in, per-image rows out."""
        return self._host("forward", "_u8", images, mean=mean, std=std)

    def forward_device_u8(self, d_images: int, n: int, d_probs: int, mean=IMAGENET_MEAN, std=IMAGENET_STD, d_label: int = 0,
                          d_prob: int = 0, stream: int = 0) -> None:
        """Device-resident path from 8-bit pixels [n][S][S][C] in HBM (raw addresses), async on `stream`."""
        self._device("forward", "_u8", d_images, n, d_probs, mean=mean, std=std, d_label=d_label, d_prob=d_prob, stream=stream)

    # ---- embedding outputs (vit_engine_features_*): kind "cls" | "mean" | "tokens" | "head", fp32 rows for both dtypes ----
    def feature_shape(self, n: int, kind="cls", l2_normalize=False) -> tuple:
        """Shape of the rows n images give: (n, D), (n, tokens, D) for "tokens", (n, num_classes) for "head"."""
        spec = feature_spec(kind, l2_normalize)
        elems = lib().vit_engine_feature_row_elems(self._h, C.byref(spec))
        if elems == 0:
            raise VitError(f"bad feature spec (kind={kind!r}, l2_normalize={l2_normalize!r})")
        D = self.cfg.embed_dim
        if FEATURE_KINDS.get(kind, kind) == FEATURE_KINDS["head"]:
            return (n, elems)
        return (n, D) if elems == D else (n, elems // D, D)

    def features(self, images: np.ndarray, kind="cls", l2_normalize=False) -> np.ndarray:
        """Host path: per-image pointers in, per-image rows out (class token, patch-token mean, or all tokens)."""
        return self._host("features", "", images, kind, l2_normalize)

    def features_u8(self, images: np.ndarray, kind="cls", l2_normalize=False, mean=IMAGENET_MEAN, std=IMAGENET_STD) -> np.ndarray:
        """Host path from 8-bit pixels [n][S][S][C] (see forward_u8)."""
        return self._host("features", "_u8", images, kind, l2_normalize, mean, std)

    def features_device(self, d_images: int, n: int, d_out: int, kind="cls", l2_normalize=False, stream: int = 0) -> None:
        """Device-resident path: raw HBM addresses, d_out [n][row] fp32, async on `stream`."""
        self._device("features", "", d_images, n, d_out, kind, l2_normalize, stream=stream)

    def features_device_u8(self, d_images: int, n: int, d_out: int, kind="cls", l2_normalize=False, mean=IMAGENET_MEAN,
                           std=IMAGENET_STD, stream: int = 0) -> None:
        """Device-resident path from 8-bit pixels [n][S][S][C] in HBM (raw addresses), async on `stream`."""
        self._device("features", "_u8", d_images, n, d_out, kind, l2_normalize, mean, std, stream=stream)

    # ---- decoded images of any size (vit_engine_*_images): Resize(resize_shorter) -> CenterCrop(img_size) -> Normalize on the device ----
    def forward_images(self, images, resize_shorter: int, mean=IMAGENET_MEAN, std=IMAGENET_STD) -> np.ndarray:
        """Host path: a list of [H][W][C] uint8 arrays of any sizes in, probabilities [n][classes] out."""
        return self._host("forward", "_images", images, mean=mean, std=std, resize_shorter=resize_shorter)

    def forward_device_images(self, images, d_probs: int, resize_shorter: int, mean=IMAGENET_MEAN, std=IMAGENET_STD, d_label: int = 0,
                              d_prob: int = 0, stream: int = 0) -> None:
        """Device-resident path: images = a list of (ptr, H, W), pixels [H][W][C] uint8 in HBM (raw addresses); async on `stream`."""
        self._device("forward", "_images", images, None, d_probs, mean=mean, std=std, resize_shorter=resize_shorter, d_label=d_label,
                     d_prob=d_prob, stream=stream)

    def features_images(self, images, resize_shorter: int, kind="cls", l2_normalize=False, mean=IMAGENET_MEAN, std=IMAGENET_STD) -> np.ndarray:
        """Host path: a list of [H][W][C] uint8 arrays of any sizes in, embedding rows out (see features)."""
        return self._host("features", "_images", images, kind, l2_normalize, mean, std, resize_shorter)

    def features_device_images(self, images, d_out: int, resize_shorter: int, kind="cls", l2_normalize=False, mean=IMAGENET_MEAN,
                               std=IMAGENET_STD, stream: int = 0) -> None:
        """Device-resident path: images = a list of (ptr, H, W) in HBM, d_out [n][row] fp32; async on `stream`."""
        self._device("features", "_images", images, None, d_out, kind, l2_normalize, mean, std, resize_shorter, stream=stream)

    # ---- the class token's attention over the tokens in the last layer (vit_engine_cls_attention_*): kind "heads" | "head_mean" ----
    def attention_shape(self, n: int, kind="heads") -> tuple:
        """Shape of the rows n images give: (n, heads, tokens) for "heads", (n, tokens) for "head_mean"."""
        spec = attention_spec(kind)
        elems = lib().vit_engine_attention_row_elems(self._h, C.byref(spec))
        if elems == 0:
            raise VitError(f"bad attention spec (kind={kind!r})")
        heads = self.cfg.num_heads
        return (n, heads, elems // heads) if spec.kind == ATTENTION_KINDS["heads"] else (n, elems)

    def cls_attention(self, images: np.ndarray, kind="heads") -> np.ndarray:
        """Host path: per-image pointers in, per-image rows out: softmax of the class query over all tokens, per head or head-averaged."""
        return self._host("cls_attention", "", images, kind)

    def cls_attention_u8(self, images: np.ndarray, kind="heads", mean=IMAGENET_MEAN, std=IMAGENET_STD) -> np.ndarray:
        """Host path from 8-bit pixels [n][S][S][C] (see forward_u8)."""
        return self._host("cls_attention", "_u8", images, kind, mean=mean, std=std)

    def cls_attention_images(self, images, resize_shorter: int, kind="heads", mean=IMAGENET_MEAN, std=IMAGENET_STD) -> np.ndarray:
        """Host path: a list of [H][W][C] uint8 arrays of any sizes in, attention rows out (see cls_attention)."""
        return self._host("cls_attention", "_images", images, kind, mean=mean, std=std, resize_shorter=resize_shorter)

    def cls_attention_device(self, d_images: int, n: int, d_out: int, kind="heads", stream: int = 0) -> None:
        """Device-resident path: raw HBM addresses, d_out [n][row] fp32, async on `stream`."""
        self._device("cls_attention", "", d_images, n, d_out, kind, stream=stream)

    def cls_attention_device_u8(self, d_images: int, n: int, d_out: int, kind="heads", mean=IMAGENET_MEAN, std=IMAGENET_STD,
                                stream: int = 0) -> None:
        """Device-resident path from 8-bit pixels [n][S][S][C] in HBM (raw addresses), async on `stream`."""
        self._device("cls_attention", "_u8", d_images, n, d_out, kind, mean=mean, std=std, stream=stream)

    def cls_attention_device_images(self, images, d_out: int, resize_shorter: int, kind="heads", mean=IMAGENET_MEAN, std=IMAGENET_STD,
                                    stream: int = 0) -> None:
        """Device-resident path: images = a list of (ptr, H, W) in HBM, d_out [n][row] fp32; async on `stream`."""
        self._device("cls_attention", "_images", images, None, d_out, kind, mean=mean, std=std, resize_shorter=resize_shorter, stream=stream)

    # ---- intermediate layers (vit_engine_intermediate_*): the residual stream behind `layers`, kind "cls" | "tokens" | "patches" | "map" ----
    def intermediate_shape(self, n: int, layers, kind="cls", norm=True) -> tuple:
        """Shape of the rows n images give, K = len(layers): (n, K, D) for "cls", (n, K, T, D) for "tokens", (n, K, P, D) for
        "patches", (n, K, D, g, g) for "map"; P = g * g patches, T = 1 + register tokens + P."""
        spec = intermediate_spec(layers, kind, norm, self.cfg.depth)
        elems = lib().vit_engine_intermediate_row_elems(self._h, C.byref(spec))
        if elems == 0:
            raise VitError(f"bad intermediate spec (layers={layers!r}, kind={kind!r}, norm={norm!r})")
        D, T, K = self.cfg.embed_dim, self.cfg.tokens, spec.num_layers
        g = self.cfg.img_size // self.cfg.patch_size
        shape = {0: (n, K, D), 1: (n, K, T, D), 2: (n, K, self.cfg.patches, D), 3: (n, K, D, g, g)}[spec.kind]
        assert int(np.prod(shape[1:])) == elems, (shape, elems)
        return shape

    def intermediate(self, images: np.ndarray, layers, kind="cls", norm=True) -> np.ndarray:
        """Host path: per-image pointers in, per-image rows out: a block per tapped layer (negative layers count from the last)."""
        return self._host("intermediate", "", images, kind, layers=layers, norm=norm)

    def intermediate_u8(self, images: np.ndarray, layers, kind="cls", norm=True, mean=IMAGENET_MEAN, std=IMAGENET_STD) -> np.ndarray:
        """Host path from 8-bit pixels [n][S][S][C] (see forward_u8)."""
        return self._host("intermediate", "_u8", images, kind, mean=mean, std=std, layers=layers, norm=norm)

    def intermediate_images(self, images, resize_shorter: int, layers, kind="cls", norm=True, mean=IMAGENET_MEAN,
                            std=IMAGENET_STD) -> np.ndarray:
        """Host path: a list of [H][W][C] uint8 arrays of any sizes in, intermediate rows out (see intermediate)."""
        return self._host("intermediate", "_images", images, kind, mean=mean, std=std, resize_shorter=resize_shorter, layers=layers, norm=norm)

    def intermediate_device(self, d_images: int, n: int, d_out: int, layers, kind="cls", norm=True, stream: int = 0) -> None:
        """Device-resident path: raw HBM addresses, d_out [n][row] fp32, async on `stream`."""
        self._device("intermediate", "", d_images, n, d_out, kind, stream=stream, layers=layers, norm=norm)

    def intermediate_device_u8(self, d_images: int, n: int, d_out: int, layers, kind="cls", norm=True, mean=IMAGENET_MEAN,
                               std=IMAGENET_STD, stream: int = 0) -> None:
        """Device-resident path from 8-bit pixels [n][S][S][C] in HBM (raw addresses), async on `stream`."""
        self._device("intermediate", "_u8", d_images, n, d_out, kind, mean=mean, std=std, stream=stream, layers=layers, norm=norm)

    def intermediate_device_images(self, images, d_out: int, resize_shorter: int, layers, kind="cls", norm=True, mean=IMAGENET_MEAN,
                                   std=IMAGENET_STD, stream: int = 0) -> None:
        """Device-resident path: images = a list of (ptr, H, W) in HBM, d_out [n][row] fp32; async on `stream`."""
        self._device("intermediate", "_images", images, None, d_out, kind, mean=mean, std=std, resize_shorter=resize_shorter, stream=stream,
                     layers=layers, norm=norm)

    # ---- top-k class records (vit_engine_topk_*): rows of 2k int32 words, k labels then the k scores' bit patterns (split_topk) ----
    def topk_shape(self, n: int, k: int) -> tuple:
        """Shape of the int32 records n images give: (n, 2k)."""
        spec = topk_spec(k)
        elems = lib().vit_engine_topk_row_elems(self._h, C.byref(spec))
        if elems == 0:
            raise VitError(f"bad top-k spec (k={k!r}): k must be 1..min({VIT_MAX_TOPK}, {self.cfg.num_classes})")
        return (n, elems)

    def topk_host(self, images: np.ndarray, k: int, score="prob", reserved: int = 0) -> np.ndarray:
        """Host path: per-image pointers in, per-image records out, int32 [n][2k]; score "prob" | "logit"."""
        return self._host("topk", "", images, topk=topk_spec(k, score, reserved))

    def topk_host_u8(self, images: np.ndarray, k: int, score="prob", mean=IMAGENET_MEAN, std=IMAGENET_STD) -> np.ndarray:
        """Host path from 8-bit pixels [n][S][S][C] (see forward_u8)."""
        return self._host("topk", "_u8", images, mean=mean, std=std, topk=topk_spec(k, score))

    def topk_host_images(self, images, resize_shorter: int, k: int, score="prob", mean=IMAGENET_MEAN, std=IMAGENET_STD) -> np.ndarray:
        """Host path: a list of [H][W][C] uint8 arrays of any sizes in, records out (see topk_host)."""
        return self._host("topk", "_images", images, mean=mean, std=std, resize_shorter=resize_shorter, topk=topk_spec(k, score))

    def topk_device(self, d_images: int, n: int, d_out: int, k: int, score="prob", stream: int = 0, reserved: int = 0) -> None:
        """Device-resident path: raw HBM addresses, d_out [n][2k] int32, async on `stream`."""
        self._device("topk", "", d_images, n, d_out, stream=stream, topk=topk_spec(k, score, reserved))

    def topk_device_u8(self, d_images: int, n: int, d_out: int, k: int, score="prob", mean=IMAGENET_MEAN, std=IMAGENET_STD,
                       stream: int = 0) -> None:
        """Device-resident path from 8-bit pixels [n][S][S][C] in HBM (raw addresses), async on `stream`."""
        self._device("topk", "_u8", d_images, n, d_out, mean=mean, std=std, stream=stream, topk=topk_spec(k, score))

    def topk_device_images(self, images, d_out: int, resize_shorter: int, k: int, score="prob", mean=IMAGENET_MEAN, std=IMAGENET_STD,
                           stream: int = 0) -> None:
        """Device-resident path: images = a list of (ptr, H, W) in HBM, d_out [n][2k] int32; async on `stream`."""
        self._device("topk", "_images", images, None, d_out, mean=mean, std=std, resize_shorter=resize_shorter, stream=stream,
                     topk=topk_spec(k, score))

    def pool_scratch_layout(self, nb: int) -> list:
        """vit_engine_debug_pool_scratch for every lane of a MEAN chunk of nb images: per lane a dict of byte ranges inside the y
        allocation, {"scratch": (lo, hi), "y": (lo, hi), "xa": (lo, hi) or None}.  Launches nothing."""
        out, lane, lanes = [], 0, 1
        while lane < lanes:
            r = (C.c_size_t * 6)()
            lanes = lib().vit_engine_debug_pool_scratch(self._h, nb, lane, r)
            if lanes < 1:
                raise VitError(f"vit_engine_debug_pool_scratch({nb}, {lane}) failed")
            out.append({"scratch": (r[0], r[1]), "y": (r[2], r[3]), "xa": (r[4], r[5]) if r[5] else None})
            lane += 1
        return out

    def sync(self) -> None:
        self._check(lib().vit_engine_sync(self._h), "vit_engine_sync")

    def logits(self, rows: int) -> np.ndarray:
        out = np.empty((rows, self.cfg.num_classes), np.float32)
        self._check(lib().vit_engine_read_logits(self._h, out.ctypes.data_as(f32p), rows), "vit_engine_read_logits")
        return out

    # ---- classifier heads (vit_engine_set_head): pooled and multi-layer operands for the head GEMM ----
    def head_in_features(self, cls_layers=(), pool="none") -> int:
        """Floats per operand row of such a head, (len(cls_layers) + (pool != "none")) * embed_dim; 0 on a bad spec."""
        return int(lib().vit_engine_head_in_features(self._h, C.byref(head_spec(cls_layers, pool, self.cfg.depth))))

    def set_head(self, weight, bias, cls_layers=(), pool="none", reserved: int = 0) -> None:
        """A head of its own for every later probability / top-k call: weight [num_classes][in_features] (nn.Linear.weight), bias
        [num_classes]; the operand row is [final LayerNorm of the class rows behind cls_layers | pooled patch tokens of the last
        layer], pool "none" | "avg" (norm, then mean) | "avg_fcnorm" (mean, then norm).  Negative layers count from the last.
        Every weight install restores the checkpoint's own head: call this again behind it.
          DINOv2 linear head, 1 layer: cls_layers=(-1,), pool="avg";  4 layers: cls_layers=(-4, -3, -2, -1), pool="avg"
          timm global_pool="avg": pool="avg";  with fc_norm: pool="avg_fcnorm" (fc_norm's tensors in the final LayerNorm's slots)"""
        spec = head_spec(cls_layers, pool, self.cfg.depth, reserved)
        w = None if weight is None else _as_f32(weight)
        b = None if bias is None else _as_f32(bias)
        F = int(lib().vit_engine_head_in_features(self._h, C.byref(spec)))
        if F and w is not None and b is not None and (w.size != self.cfg.num_classes * F or b.size != self.cfg.num_classes):
            raise VitError(f"set_head: weight has {w.size} floats and bias {b.size}, the head needs {self.cfg.num_classes} x {F} and "
                           f"{self.cfg.num_classes}")
        self._check(lib().vit_engine_set_head(self._h, C.byref(spec), None if w is None else w.ctypes.data_as(f32p),
                                              None if b is None else b.ctypes.data_as(f32p)), "vit_engine_set_head")
        self._head_in = F

    def reset_head(self) -> None:
        """Back to the checkpoint's own head (vit_engine_set_head with a NULL spec)."""
        self._check(lib().vit_engine_set_head(self._h, None, None, None), "vit_engine_set_head")
        self._head_in = None

    # ---- dense linear heads (vit_engine_set_dense_head, vit_engine_dense_*): a class per pixel from the patch tokens ----
    def set_dense_head(self, weight, bias, layers, norm=True, reserved: int = 0) -> None:
        """A dense linear head for the dense calls: weight [num_classes][len(layers) * embed_dim] (the 1x1 conv's weight, the
        earliest layer's columns first; a BatchNorm in front of it folded by fold_batchnorm), bias [num_classes]; num_classes is
        taken from bias.  layers: the tapped encoder layers (mmseg out_indices; negative entries count from the last), norm: the
        final LayerNorm on every tap (DINOv2).  Independent of the classifier head.  Every weight install removes it: call this
        again behind it.  DINOv2 `linear`: layers=(-1,);  `ms`: layers=(-4, -3, -2, -1) of ViT-S/B (out_indices [8, 9, 10, 11])."""
        w = None if weight is None else _as_f32(weight)
        b = None if bias is None else _as_f32(bias)
        spec = dense_head_spec(layers, norm, 0 if b is None else b.size, self.cfg.depth, reserved)
        F = spec.num_layers * self.cfg.embed_dim
        if w is not None and b is not None and w.size != b.size * F:
            raise VitError(f"set_dense_head: weight has {w.size} floats, {b.size} classes over {spec.num_layers} layers need {b.size} x {F}")
        self._check(lib().vit_engine_set_dense_head(self._h, C.byref(spec), None if w is None else w.ctypes.data_as(f32p),
                                                    None if b is None else b.ctypes.data_as(f32p)), "vit_engine_set_dense_head")

    def reset_dense_head(self) -> None:
        """Remove the dense head (vit_engine_set_dense_head with a NULL spec)."""
        self._check(lib().vit_engine_set_dense_head(self._h, None, None, None), "vit_engine_set_dense_head")

    def dense_row_bytes(self, kind="labels", out_size=None) -> int:
        """Bytes per output row of a dense call; 0 on a bad spec or without a dense head."""
        return int(lib().vit_engine_dense_row_bytes(self._h, C.byref(dense_spec(kind, out_size))))

    def dense_shape(self, n: int, spec) -> tuple:
        """Shape of the rows n images give: (n, out_h, out_w) uint8 labels or (n, num_classes, g, g) fp32 logits.  A spec the C side
        refuses still gets rows (the call must see its own arguments and say what is wrong)."""
        g = self.cfg.img_size // self.cfg.patch_size
        nbytes = int(lib().vit_engine_dense_row_bytes(self._h, C.byref(spec)))
        if spec.kind == DENSE_KINDS["labels"]:
            h, w = spec.out_h or self.cfg.img_size, spec.out_w or self.cfg.img_size
            return (n, h, w) if nbytes == h * w else (n, 1, 1)
        return (n, nbytes // (4 * g * g), g, g) if nbytes else (n, 1, 1, 1)

    def dense(self, images: np.ndarray, kind="labels", out_size=None) -> np.ndarray:
        """Host path: per-image pointers in, per-image rows out -- kind "labels": uint8 [n][out_h][out_w], the argmax over the
        classes of the head's logits resized bilinearly (align_corners=False) to out_size (None: img_size; an int or (h, w));
        kind "grid": fp32 [n][num_classes][g][g], the logits themselves."""
        return self._host("dense", "", images, dense=dense_spec(kind, out_size))

    def dense_u8(self, images: np.ndarray, kind="labels", out_size=None, mean=IMAGENET_MEAN, std=IMAGENET_STD) -> np.ndarray:
        """Host path from 8-bit pixels [n][S][S][C] (see forward_u8)."""
        return self._host("dense", "_u8", images, mean=mean, std=std, dense=dense_spec(kind, out_size))

    def dense_images(self, images, resize_shorter: int, kind="labels", out_size=None, mean=IMAGENET_MEAN, std=IMAGENET_STD) -> np.ndarray:
        """Host path: a list of [H][W][C] uint8 arrays of any sizes in (see forward_images); the labels are those of the crop."""
        return self._host("dense", "_images", images, mean=mean, std=std, resize_shorter=resize_shorter, dense=dense_spec(kind, out_size))

    def dense_device(self, d_images: int, n: int, d_out: int, kind="labels", out_size=None, stream: int = 0) -> None:
        """Device-resident path: raw HBM addresses, d_out [n][dense_row_bytes()] bytes, async on `stream`."""
        self._device("dense", "", d_images, n, d_out, stream=stream, dense=dense_spec(kind, out_size))

    def dense_device_u8(self, d_images: int, n: int, d_out: int, kind="labels", out_size=None, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                        stream: int = 0) -> None:
        """Device-resident path from 8-bit pixels [n][S][S][C] in HBM."""
        self._device("dense", "_u8", d_images, n, d_out, mean=mean, std=std, stream=stream, dense=dense_spec(kind, out_size))

    def dense_device_images(self, images, d_out: int, resize_shorter: int, kind="labels", out_size=None, mean=IMAGENET_MEAN,
                            std=IMAGENET_STD, stream: int = 0) -> None:
        """Device-resident path from decoded images: a list of (ptr, H, W) records (see forward_device_images)."""
        self._device("dense", "_images", images, None, d_out, mean=mean, std=std, resize_shorter=resize_shorter, stream=stream,
                     dense=dense_spec(kind, out_size))

    def head_operand(self, rows: int) -> np.ndarray:
        """vit_engine_read_head_operand: the head GEMM's operand rows of the most recent chunk, [rows][in_features]."""
        out = np.empty((rows, self._head_in or self.cfg.embed_dim), np.float32)
        self._check(lib().vit_engine_read_head_operand(self._h, out.ctypes.data_as(f32p), rows), "vit_engine_read_head_operand")
        return out

    def handover_stats(self) -> dict:
        """vit_engine_handover_stats: fp32 GEMM helper pieces taken / recomputed since the last call (syncs the device)."""
        L = lib()
        t, r = C.c_long(), C.c_long()
        L.vit_engine_handover_stats.argtypes = [C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_long)]
        self._check(L.vit_engine_handover_stats(self._h, C.byref(t), C.byref(r)), "vit_engine_handover_stats")
        return {"taken": int(t.value), "recomputed": int(r.value)}

    def set_lanes(self, lanes: int) -> None:
        L = lib()
        L.vit_engine_set_lanes.argtypes = [C.c_void_p, C.c_int]
        self._check(L.vit_engine_set_lanes(self._h, lanes), "vit_engine_set_lanes")

    def set_layernorm_eps(self, eps: float) -> None:
        """vit_engine_set_layernorm_eps: the epsilon (a double; default 1e-6) of every LayerNorm the engine runs.  It persists across
        weight installs.  CLIP: 1e-5."""
        L = lib()
        L.vit_engine_set_layernorm_eps.argtypes = [C.c_void_p, C.c_double]
        self._check(L.vit_engine_set_layernorm_eps(self._h, float(eps)), "vit_engine_set_layernorm_eps")

    def get_layernorm_eps(self) -> float:
        L = lib()
        L.vit_engine_get_layernorm_eps.argtypes = [C.c_void_p]
        L.vit_engine_get_layernorm_eps.restype = C.c_double
        return float(L.vit_engine_get_layernorm_eps(self._h))

    def set_pre_norm(self, gamma, beta) -> None:
        """vit_engine_set_pre_norm: a LayerNorm in front of layer 0 (CLIP's ln_pre), gamma / beta [embed_dim]; None, None removes it.
        Every weight install removes it: call this again behind it."""
        L = lib()
        L.vit_engine_set_pre_norm.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        g = None if gamma is None else _as_f32(gamma).reshape(-1)
        b = None if beta is None else _as_f32(beta).reshape(-1)
        for a in (g, b):
            if a is not None and a.size != self.cfg.embed_dim:
                raise VitError(f"set_pre_norm: {a.size} floats, the model has embed_dim = {self.cfg.embed_dim}")
        self._check(L.vit_engine_set_pre_norm(self._h, None if g is None else g.ctypes.data, None if b is None else b.ctypes.data),
                    "vit_engine_set_pre_norm")

    def set_resize_filter(self, filter) -> None:
        """vit_engine_set_resize_filter: "bilinear" (the default) | "bicubic", the Resize filter of every *_images call from the next one
        on; read on the host when a call enqueues, so it may change between calls without a sync."""
        self._check(lib().vit_engine_set_resize_filter(self._h, _resize_filter(filter)), "vit_engine_set_resize_filter")

    def get_resize_filter(self) -> str:
        v = lib().vit_engine_get_resize_filter(self._h)
        return {n: k for k, n in RESIZE_FILTERS.items()}[v]

    def set_profile(self, on: bool) -> None:
        self._check(lib().vit_engine_set_profile(self._h, 1 if on else 0), "vit_engine_set_profile")

    def reset_stage_times(self) -> None:
        lib().vit_engine_reset_stage_times(self._h)

    def stage_times(self) -> dict:
        t = CStageTimes()
        self._check(lib().vit_engine_get_stage_times(self._h, C.byref(t)), "vit_engine_get_stage_times")
        return {"images": int(t.images),
                "stages": {s: {"ms": float(t.ms[i]), "launches": int(t.launches[i])} for i, s in enumerate(STAGES)}}

    def close(self) -> None:
        if self._h:
            lib().vit_engine_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# --------------------------------------------------------------------------------------------------
# Facade + io
# --------------------------------------------------------------------------------------------------
def facade_forward(images: np.ndarray, weights: Sequence[np.ndarray], use_reference_names: bool = True) -> np.ndarray:
    """initialize_* -> ViT_*(ImageData*, Network*, float**) -> Release_* exactly as Main.c drives it."""
    L = lib()
    images = _as_f32(images)
    n, c, h, w = images.shape
    imgs = (CImageData * n)()
    rows = [images[i] for i in range(n)]
    for i in range(n):
        imgs[i] = CImageData(n, c, h, w, rows[i].ctypes.data_as(f32p))
    nets, keep = networks_from(weights)
    probs = np.empty((n, 1000), np.float32)
    out_ptrs = (f32p * n)(*[probs[i].ctypes.data_as(f32p) for i in range(n)])
    if use_reference_names:
        L.initialize_opencl()
        L.ViT_opencl(imgs, nets, out_ptrs)
        L.Release_opencl()
    else:
        L.initialize_hip()
        L.ViT_hip(imgs, nets, out_ptrs)
        L.Release_hip()
    return probs


def load_image_file(path: str) -> Optional[np.ndarray]:
    L = lib()
    p = L.load_image_data(path.encode())
    if not p:
        return None
    n, c, h, w = p[0].n, p[0].c, p[0].h, p[0].w
    out = np.stack([np.ctypeslib.as_array(p[i].data, shape=(c, h, w)).copy() for i in range(n)])
    L.free_image_data(p)
    return out


def load_weight_dir(directory: str, count: int):
    """load_weights() -> list of arrays (None where the file is absent)."""
    L = lib()
    nets = (CNetwork * count)()
    L.load_weights(directory.encode(), nets, count)
    out = [np.ctypeslib.as_array(nets[i].data, shape=(nets[i].size,)).copy() if nets[i].data else None
           for i in range(count)]
    L.free_weights(nets, count)
    return out


def load_weight_dir_cached(cfg: ModelConfig, directory: str, cache_path: Optional[str] = None):
    """load_weights_cached(): Network[] through the packed cache file (validated against the directory's files)."""
    L = lib()
    L.load_weights_cached.argtypes = [C.POINTER(CConfig), C.c_char_p, C.POINTER(CNetwork), C.c_int, C.c_char_p]
    count = cfg.n_weights
    nets = (CNetwork * count)()
    cc = CConfig.of(cfg)
    L.load_weights_cached(C.byref(cc), directory.encode(), nets, count, cache_path.encode() if cache_path else None)
    out = [np.ctypeslib.as_array(nets[i].data, shape=(nets[i].size,)).copy() if nets[i].data else None
           for i in range(count)]
    L.free_weights(nets, count)
    return out


class CWeightImage(C.Structure):  # include/vit_io.h: vit_weight_image
    _fields_ = [("cfg", CConfig), ("count", C.c_int), ("f32_floats", C.c_size_t), ("gemm_floats", C.c_size_t),
                ("bf16_elems", C.c_size_t), ("off", C.POINTER(C.c_size_t)), ("size", C.POINTER(C.c_size_t)),
                ("f32", f32p), ("bf16", C.POINTER(C.c_ushort))]


class WeightImage:
    """vit_weight_image: the device layout of a model's weights on the host / in the cache file."""

    def __init__(self):
        self.c = CWeightImage()
        L = lib()
        L.vit_weight_image_build.argtypes = [C.POINTER(CWeightImage), C.POINTER(CConfig), C.POINTER(CNetwork), C.c_int, C.c_int]
        L.vit_weight_image_free.argtypes = [C.POINTER(CWeightImage)]
        L.vit_weight_image_save.argtypes = [C.POINTER(CWeightImage), C.c_char_p, C.c_char_p]
        L.vit_weight_image_load.argtypes = [C.POINTER(CWeightImage), C.c_char_p, C.POINTER(CConfig), C.c_char_p]
        L.vit_engine_load_weight_image.argtypes = [C.c_void_p, C.POINTER(CWeightImage)]
        L.vit_engine_read_weight_image.argtypes = [C.c_void_p, C.POINTER(CWeightImage)]

    @classmethod
    def build(cls, cfg: ModelConfig, weights: Sequence[np.ndarray], with_bf16: bool = True) -> "WeightImage":
        img = cls()
        arr, keep = networks_from(weights)
        cc = CConfig.of(cfg)
        if lib().vit_weight_image_build(C.byref(img.c), C.byref(cc), arr, len(weights), 1 if with_bf16 else 0) != 0:
            raise VitError("vit_weight_image_build: incomplete or mis-sized weight set")
        return img

    @classmethod
    def load(cls, cfg: ModelConfig, path: str, source_dir: Optional[str] = None) -> Optional["WeightImage"]:
        img = cls()
        cc = CConfig.of(cfg)
        rc = lib().vit_weight_image_load(C.byref(img.c), path.encode(), C.byref(cc), source_dir.encode() if source_dir else None)
        return img if rc == 0 else None

    def save(self, path: str, source_dir: Optional[str] = None) -> int:
        return lib().vit_weight_image_save(C.byref(self.c), path.encode(), source_dir.encode() if source_dir else None)

    def tensors(self):
        return [np.ctypeslib.as_array(self.c.f32, shape=(self.c.f32_floats,))[self.c.off[i]:self.c.off[i] + self.c.size[i]].copy()
                for i in range(self.c.count)]

    def f32_section(self) -> np.ndarray:
        return np.ctypeslib.as_array(self.c.f32, shape=(self.c.f32_floats,)).copy()

    def bf16_section(self) -> Optional[np.ndarray]:
        if not self.c.bf16_elems:
            return None
        return np.ctypeslib.as_array(self.c.bf16, shape=(self.c.bf16_elems,)).copy()

    def free(self) -> None:
        lib().vit_weight_image_free(C.byref(self.c))

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def read_image_file_chunked(path: str, chunk: int):
    """vit_image_reader_*: list of (first_index, array) chunks, or None when the file cannot be opened."""
    L = lib()
    L.vit_image_reader_open.restype = C.c_void_p
    L.vit_image_reader_open.argtypes = [C.c_char_p] + [C.POINTER(C.c_int)] * 4
    L.vit_image_reader_next.restype = C.POINTER(CImageData)
    L.vit_image_reader_next.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.vit_image_reader_close.argtypes = [C.c_void_p]
    dims = [C.c_int() for _ in range(4)]
    r = L.vit_image_reader_open(path.encode(), *[C.byref(d) for d in dims])
    if not r:
        return None
    out = []
    while True:
        first = C.c_int()
        p = L.vit_image_reader_next(r, chunk, C.byref(first))
        if not p:
            break
        k, c, h, w = p[0].n, p[0].c, p[0].h, p[0].w
        assert all(p[i].n == k for i in range(k))
        out.append((first.value, np.stack([np.ctypeslib.as_array(p[i].data, shape=(c, h, w)).copy() for i in range(k)])))
        L.free_image_data(p)
    L.vit_image_reader_close(r)
    return dims[0].value, out


def round_weights(w: np.ndarray) -> np.ndarray:
    out = _as_f32(w).copy()
    lib().vit_round_weights(out.ctypes.data_as(f32p), out.size)
    return out


def synth_uniform(seed: int, index: int, n: int, lo: float, hi: float) -> np.ndarray:
    out = np.empty(n, np.float32)
    lib().vit_synth_uniform(seed, index, n, lo, hi, out.ctypes.data_as(f32p))
    return out


def synth_weights_c(cfg: ModelConfig, seed: int):
    """The C generator (vit_synth_uniform + vit_round_weights of the host library, the pair vit_synth_weights() runs per tensor),
    filling numpy arrays in place; must equal synth.make_weights(native=False) bit for bit (tests/test_host_io.py)."""
    from .synth import _RANGE, _kind
    L = lib()
    L.vit_synth_uniform.argtypes = [C.c_ulonglong, C.c_int, C.c_size_t, C.c_float, C.c_float, C.c_void_p]
    L.vit_synth_uniform.restype = None
    L.vit_round_weights.argtypes = [C.c_void_p, C.c_size_t]
    L.vit_round_weights.restype = None
    out = []
    for i, shape in enumerate(cfg.weight_shapes()):
        kind = _kind(cfg, i)
        lo, hi = (0.5, 1.0) if kind == "ln_w" else (-_RANGE[kind], _RANGE[kind])
        w = np.empty(shape, np.float32)
        L.vit_synth_uniform(seed, i, w.size, lo, hi, w.ctypes.data)
        L.vit_round_weights(w.ctypes.data, w.size)
        out.append(w)
    return out


def synth_images_c(cfg: ModelConfig, n: int, seed: int) -> np.ndarray:
    L = lib()
    cc = CConfig.of(cfg)
    p = L.vit_synth_images(C.byref(cc), n, seed)
    out = np.stack([np.ctypeslib.as_array(p[i].data, shape=(cfg.in_chans, cfg.img_size, cfg.img_size)).copy()
                    for i in range(n)])
    L.free_image_data(p)
    return out


def write_results(path: str, probs: np.ndarray, fix_argmax: bool = True) -> int:
    probs = _as_f32(probs)
    n, classes = probs.shape
    ptrs = (f32p * n)(*[probs[i].ctypes.data_as(f32p) for i in range(n)])
    L = lib()
    L.vit_write_results_file.argtypes = [C.c_char_p, C.POINTER(f32p), C.c_int, C.c_int, C.c_int]
    return L.vit_write_results_file(path.encode(), ptrs, n, classes, 1 if fix_argmax else 0)


def compare_results(result_path: str, answer_path: str, lines: int, tol: float = 0.01) -> int:
    return lib().vit_compare_results(result_path.encode(), answer_path.encode(), lines, tol)
