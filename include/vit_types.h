/*
 * include/vit_types.h -- data model shared by the loaders and the forward entry points.
 *
 * These two structs ARE the reference's (Network.h:7-13 and Network.h:18-21, duplicated at
 * Network.c:9-20): a caller written against the reference passes them unchanged.
 *
 *   ImageData: load_image_data() returns an ARRAY of n structs; every element carries the
 *              total count in .n and owns a separately malloc'd CHW fp32 image in .data
 *              (Network.c:66-93).  The forward entry reads image[0].n images.
 *   Network:   one weight tensor; .size is the ELEMENT count; {NULL,0} when the file was
 *              absent (Network.c:127-130,190-191).
 */
#ifndef VIT_TYPES_H
#define VIT_TYPES_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int n;        /* total number of images in the array this element belongs to */
    int c;        /* channels */
    int h;        /* height   */
    int w;        /* width    */
    float *data;  /* this image, CHW fp32, separately allocated */
} ImageData;

typedef struct {
    float *data;  /* raw fp32 tensor in PyTorch layout (Linear.weight = [out][in]) */
    size_t size;  /* number of floats */
} Network;

/*
 * Model dimensions.  The reference fixes them with macros (ViT_seq.c:10-21,
 * ViT_opencl.c:12-23); here they are a runtime struct so that the same engine serves
 * ViT-B/16-224 (the default), reduced test models and ViT-L/16-384.
 * Constraints of the HIP path: head_dim = embed_dim / num_heads is 64 or a multiple of 8 from 72 to 128 (80: ViT-H/14, 88: ViT-g-14,
 * 104: ViT-bigG-14; vithip_qscale(head_dim) != 0), embed_dim % 32 == 0 (bf16 engines and the LayerNorm fold: % 64), embed_dim <= 2048,
 * hidden_dim % 32 == 0 (bf16 engines: % 64; under VIT_MLP_SWIGLU the 2 * hidden_dim rows of fc1 inherit it), patch_size and img_size even (patch 14 included; the 8-bit and decoded-image
 * input calls also need img_size % 4 == 0).
 */
typedef struct {
    int img_size;     /* 224 */
    int patch_size;   /* 16; bits 24..30 hold the count of register tokens (0: a plain patch size is a model without): VIT_PATCH_SIZE_OF() */
    int in_chans;     /* 3   */
    int num_classes;  /* 1000 */
    int embed_dim;    /* 768 */
    int depth;        /* 12  */
    int num_heads;    /* 12  */
    int hidden_dim;   /* 3072 = (int)(embed_dim * mlp_ratio), ViT_seq.c:254: the width of the hidden layer that fc2 reads, below 2^24;
                       * bits 24..30 hold the MLP kind (0 = VIT_MLP_GELU, so a plain width is a GELU model): VIT_HIDDEN_DIM_OF() */
} vit_config;

/*
 * The MLP kind.  VIT_MLP_GELU: fc1 -> erf-GELU -> fc2.  VIT_MLP_SWIGLU: fc1 is the fused [2 * H][embed_dim] "w12" (gate rows first,
 * value rows behind) and the hidden layer is silu(gate) * value.  VIT_MLP_QUICKGELU (CLIP): fc1 -> y * sigmoid(1.702 y) -> fc2, the
 * layout of a GELU model.  The struct keeps its eight ints -- compiled callers, positional
 * initialisers and the cache file's eight header words stay as they are -- so the kind travels in the top bits of hidden_dim:
 *     vit_config g14 = {224, 14, 3, 1000, 1536, 40, 24, VIT_HIDDEN_DIM_OF(4096, VIT_MLP_SWIGLU)};
 * Read the two parts with VIT_HIDDEN_DIM(cfg) and VIT_MLP_KIND(cfg), never hidden_dim itself.
 */
enum { VIT_MLP_GELU = 0, VIT_MLP_SWIGLU = 1, VIT_MLP_QUICKGELU = 3 /* 2 stays unassigned: callers know it as a refused kind */ };
#define VIT_MLP_SHIFT 24
#define VIT_HIDDEN_DIM_OF(width, mlp) ((int)(width) | ((int)(mlp) << VIT_MLP_SHIFT))
#define VIT_HIDDEN_DIM(cfg) ((cfg)->hidden_dim & ((1 << VIT_MLP_SHIFT) - 1))
#define VIT_MLP_KIND(cfg) ((cfg)->hidden_dim >> VIT_MLP_SHIFT)
/* output rows of the fc1 weight (tensors 8 and 9 of a layer hold VIT_FC1_ROWS * embed_dim and VIT_FC1_ROWS floats) */
#define VIT_FC1_ROWS(cfg) (VIT_MLP_KIND(cfg) == VIT_MLP_SWIGLU ? 2 * VIT_HIDDEN_DIM(cfg) : VIT_HIDDEN_DIM(cfg))

/*
 * Register tokens (DINOv2 `_reg4`, "Vision Transformers Need Registers"): R learned rows between the class token and the patch
 * tokens, T = 1 + R + (img_size / patch_size)^2 token rows in that order.  They take no position embedding, and no output counts
 * them among "the patch tokens".  As with the MLP kind, the struct keeps its eight ints and the count travels in the top bits of
 * patch_size:
 *     vit_config reg = {224, VIT_PATCH_SIZE_OF(14, 4), 3, 1000, 768, 12, 12, 3072};
 * Read the two parts with VIT_PATCH_SIZE(cfg) and VIT_REGISTER_TOKENS(cfg), never patch_size itself.  Weight tensor 0 of such a
 * model is the prefix [(1 + R)][embed_dim]: the class token, then the checkpoint's register_tokens in their order; tensor 3, the
 * position embedding, stays [(g * g + 1)][embed_dim].
 */
#define VIT_REG_SHIFT 24
#define VIT_PATCH_SIZE_OF(patch, regs) ((int)(patch) | ((int)(regs) << VIT_REG_SHIFT))
#define VIT_PATCH_SIZE(cfg) ((cfg)->patch_size & ((1 << VIT_REG_SHIFT) - 1))
#define VIT_REGISTER_TOKENS(cfg) ((cfg)->patch_size >> VIT_REG_SHIFT)
#define VIT_MAX_REGISTER_TOKENS 16

#define VIT_WEIGHTS_PER_LAYER 12
/* number of Network entries: cls (the prefix: class token + register tokens), conv w/b, pos, 12 per layer, ln w/b, head w/b (Main.c:29-30 => 152) */
#define VIT_WEIGHT_COUNT(depth) (4 + VIT_WEIGHTS_PER_LAYER * (depth) + 4)

#ifdef __cplusplus
}
#endif
#endif /* VIT_TYPES_H */
