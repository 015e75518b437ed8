/*
 * include/vit_engine.h -- the batched ViT forward engine (host side, plain C).
 *
 * This is the re-entrant object underneath the reference-shaped facade of ViT_hip.h.  It owns
 * what the reference's OpenCL path re-creates on every call (ViT_opencl.c:126-883: buffers,
 * weight uploads, per-op blocking reads): device-resident weights uploaded ONCE, a workspace
 * sized for a whole batch, one in-order HIP stream, and the layer loop that enqueues the
 * kernels of vit_hip_kernels.h.  The forward is ViT_seq.c:337-439 for a batch of images
 * (the reference loops `for i < image->n`, ViT_seq.c:354; here the batch is the GEMM M dimension).
 *
 * All functions return VIT_OK or an error code; vit_engine_last_error() gives the message.
 * Nothing here prints or exits -- that convention belongs to the facade (ViT_hip.h).
 */
#ifndef VIT_ENGINE_H
#define VIT_ENGINE_H

#include "vit_io.h"
#include "vit_types.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    VIT_OK = 0,
    VIT_ERR_ARG = 1,      /* bad argument / unsupported configuration */
    VIT_ERR_WEIGHTS = 2,  /* missing or mis-sized weight tensor */
    VIT_ERR_HIP = 3,      /* a HIP call failed (message carries the hipError string) */
    VIT_ERR_NOMEM = 4,
    VIT_ERR_STATE = 5     /* e.g. forward before weights were loaded */
};

typedef struct vit_engine vit_engine;

typedef struct {
    int device;      /* HIP device ordinal */
    int max_batch;   /* images per forward chunk (workspace is sized for it); default 256 */
    int profile;     /* 1: bracket every stage with events and accumulate vit_stage_times */
    int lanes;       /* sub-batches of a chunk run concurrently on separate streams (1..4); default 1 */
    int dtype;       /* VIT_DTYPE_F32 (default: the reference's arithmetic) or VIT_DTYPE_BF16 (bf16 MFMA GEMMs) */
    int prune_last_layer; /* 1: in the LAST encoder layer compute only what the class token needs (default 0).  Only row
                           * 0 of the encoder output feeds the classifier (ViT_seq.c:429-435), so after the last layer's
                           * K/V projections every token-wise operation runs on the n class rows instead of n*tokens:
                           * the probabilities are bit-identical, 7 % of the reference's arithmetic is not executed
                           * (vit_config_macs_per_image_pruned).  Off by default: bench.py's metric counts the
                           * reference's full work.  tokens <= 224. */
    int use_graph;   /* 1: vit_engine_forward_device() captures its launch sequence into a hipGraph the first time it sees
                      * an (n, pointers, stream-kind) combination and replays the graph afterwards (default 0).  For
                      * small batches the ~150 launches of a forward are a visible share of the latency.  Ignored
                      * while profiling, with lanes > 1 and on the NULL stream (not capturable). */
    int gemm_tile;   /* tuning: vithip_gemm_args.tile for every fp32 GEMM of this engine (0 = auto, the default) */
    int ln_fold;     /* fold the encoder LayerNorms into the GEMMs behind them (vit_hip_kernels.h, "LayerNorm folding"): in_proj and
                      * fc1 multiply the un-normalised rows with gamma-folded weights and rescale in their epilogues, a LayerNorm
                      * is then one pass that reads x and writes 8 bytes per row (fp32) or nothing at all (bf16: the residual
                      * GEMM in front produces the row sums).  0 = auto (fp32: on when embed_dim % 64 == 0 and <= 2048; bf16: on
                      * when embed_dim and hidden_dim >= 128), 1 = on (error when the shapes do not allow it), -1 = off: a
                      * LayerNorm kernel per LayerNorm, i.e. the reference's operation order (ViT_seq.c:103-147) -- both orders
                      * meet the 1e-4 bar against ViT_seq.c, the folded one is not the same bits as the unfolded one. */
    int gemm_handover_test; /* testing: vithip_gemm_args.handover_test for every fp32 GEMM (1 = helper pieces arrive too late and
                             * every owner computes its whole tile; results must not change) */
    int host_first_piece;   /* vit_engine_forward_host(): images in the FIRST piece of a call (nothing overlaps its gather and upload,
                             * so it is a small one; the rest follows behind its compute in pieces of max_batch).  0 = auto (the
                             * measured choice, host/vit_engine.c), otherwise clamped to [1, max_batch].  Rows are bit-identical
                             * whatever the cut. */
    int fp32_split;  /* fp32 engines: the encoder GEMMs (QKV, out_proj, fc1, fc2 of every layer) on the bf16 matrix pipe through the
                      * three-piece operand split (vithip_gemm_args.arith = 1); the patch embedding and the head
                      * stay on fp32 MFMA.  0 = auto (on: every fp32 model shape allows it), 1 = on, -1 = off (fp32 MFMA throughout,
                      * the arithmetic of earlier versions bit for bit).  Ignored by bf16 engines. */
} vit_engine_options;

enum { VIT_DTYPE_F32 = 0, VIT_DTYPE_BF16 = 1 };

/* Per-stage device time of the profiled forwards (ms, summed) and launch counts. */
enum {
    VIT_STAGE_EMBED = 0, VIT_STAGE_LN, VIT_STAGE_QKV, VIT_STAGE_ATTN, VIT_STAGE_OUTPROJ,
    VIT_STAGE_FC1, VIT_STAGE_FC2, VIT_STAGE_HEAD, VIT_STAGE_SOFTMAX, VIT_STAGE_COUNT
};
typedef struct {
    double ms[VIT_STAGE_COUNT];
    long launches[VIT_STAGE_COUNT];
    long images;  /* images covered by the profiled forwards */
} vit_stage_times;

/* ViT-B/16-224: the reference's macros (ViT_seq.c:10-21). */
vit_config vit_config_b16(void);
/* patches = g * g, g = img_size / VIT_PATCH_SIZE; tokens T = 1 + VIT_REGISTER_TOKENS + patches, the rows of an image in the order the
 * model keeps them: class token, register tokens (none unless vit_config.patch_size carries a count), patch tokens.
 *
 * What every output does with R = VIT_REGISTER_TOKENS register tokens (R = 0: everything as it was):
 *   probabilities, top-k, VIT_FEAT_CLS, VIT_FEAT_HEAD, VIT_TAP_CLS      row 0
 *   VIT_FEAT_MEAN, pooled heads (VIT_HEAD_POOL_AVG, _AVG_FCNORM)        the mean over the g * g patch tokens, rows 1 + R .. T - 1
 *                                                                       (transformers' Dinov2WithRegistersForImageClassification)
 *   VIT_FEAT_TOKENS, VIT_TAP_TOKENS                                     all T rows (hidden_states; x_norm_regtokens = rows 1 .. R)
 *   VIT_TAP_PATCHES, VIT_TAP_MAP, dense heads                           the g * g patch rows, [P][D] / [D][g][g]
 *                                                                       (Dinov2WithRegistersBackbone's feature maps)
 *   class-token attention                                               rows of T weights in stored order, summing to 1 over all
 *                                                                       T: the patches are entries 1 + R ..; registers are neither
 *                                                                       dropped nor renormalised away
 * Below, P = g * g is the count of patch tokens and F = 1 + R the row of the first of them (F = 1 without registers).
 * vit_engine_copy_weights* need equal R; the resampled loads work on tensor 3 unchanged. */
int vit_config_patches(const vit_config *cfg);
int vit_config_tokens(const vit_config *cfg);
/* Expected element count of weight tensor `index` (reference index map); 0 if out of range.  Tensor 0 is the
 * prefix [(1 + R)][D] (class token, then register tokens), tensor 3 the position embedding [(g * g + 1)][D] at every R. */
size_t vit_config_weight_size(const vit_config *cfg, int index);
/* Algorithmic MACs of one image (17,563,828,224 for ViT-B/16-224). */
unsigned long long vit_config_macs_per_image(const vit_config *cfg);
/* MACs actually executed per image with vit_engine_options.prune_last_layer = 1. */
unsigned long long vit_config_macs_per_image_pruned(const vit_config *cfg);

void vit_engine_default_options(vit_engine_options *opt);
int vit_engine_create(vit_engine **out, const vit_config *cfg, const vit_engine_options *opt);
void vit_engine_destroy(vit_engine *e);
const char *vit_engine_last_error(const vit_engine *e);
const vit_config *vit_engine_config(const vit_engine *e);

/*
 * Validate (non-NULL, exact element count -- the reference's loader validates nothing,
 * Network.c:147) and upload all `count` = VIT_WEIGHT_COUNT(depth) tensors once.
 * The host arrays are only borrowed during the call.
 */
int vit_engine_load_weights(vit_engine *e, const Network *weights, int count);
/*
 * The same from a device-layout weight image (vit_io.h: built once, or read from the cache file): ONE host-to-device
 * copy of [fp32 tensors | bf16 GEMM operands]; an image without a bf16 section is converted on the device (one launch).
 */
int vit_engine_load_weight_image(vit_engine *e, const vit_weight_image *img);
/* Replicate the resident weights of `src` into `dst` (same model and dtype, any two devices of the process) with one
 * device-to-device copy -- over xGMI between GPUs, instead of another upload from the host. */
int vit_engine_copy_weights(vit_engine *dst, vit_engine *src);
/* Read the resident weights back as an image (bf16 section = the device's own conversion), e.g. to write the cache. */
int vit_engine_read_weight_image(vit_engine *e, vit_weight_image *img);

/*
 * A checkpoint at another input size than the one it was trained at: cfg.img_size is the size the engine runs at, and the one tensor
 * tied to it -- tensor 3, the position embedding [tokens][D] -- is resampled on the device from the checkpoint's own grid
 * (vithip_pos_resample_f32 in vit_hip_kernels.h states the arithmetic; DESIGN.md the agreement with PyTorch).  Row 0, the class
 * token's embedding, is copied; the g_src x g_src patch part becomes g_dst x g_dst, g = img_size / patch_size.
 *   VIT_POS_BICUBIC     torch.nn.functional.interpolate(mode="bicubic", align_corners=False): DINO, DeiT, DINOv2 given a size
 *   VIT_POS_BICUBIC_AA  the same with antialias=True: the default of timm's resample_abs_pos_embed
 * Everything else of the forward does not depend on the token count and runs on the same kernels at every size.
 *
 * vit_engine_load_weights_resampled: vit_engine_load_weights, except that tensor 3 must have ((src_img_size / patch_size)^2 + 1) * D
 * floats.  The other tensors take the usual path (one image, one upload); the checkpoint's position embedding goes to a temporary
 * device buffer and is resampled into the resident tensor 3 in front of the LayerNorm fold and the weight split; the temporary is
 * freed before the call returns.  fp32 and bf16 engines alike: the position embedding is an fp32 tensor in both.  The resampled
 * values are NOT rounded to 1e-6: that rounding is the file loader's and the checkpoint has been through it.
 * With src_img_size == cfg.img_size nothing is resampled and the result is vit_engine_load_weights bit for bit.
 * vit_engine_read_weight_image afterwards gives an image for the engine's own cfg that holds the resampled tensor, so the cache file
 * of vit_io.h can store a checkpoint at its serving resolution.
 * Every check comes before anything is changed: a refused call leaves the resident weights, and a captured graph, in working order.
 * VIT_ERR_ARG: NULL rs, reserved != 0, an unknown mode, src_img_size not a positive multiple of cfg.patch_size, a grid of more than
 * 256 patches per side.  VIT_ERR_WEIGHTS: what vit_engine_load_weights refuses, and a tensor 3 of the wrong size (the message names
 * both grids and both sizes).
 *
 * vit_engine_copy_weights_resampled: vit_engine_copy_weights between engines of the same dtype whose configurations are equal in every
 * field except img_size (anything else: VIT_ERR_ARG).  Every tensor but the position embedding is copied device to device (the
 * layouts differ behind tensor 3: two ranges and the bf16 section); dst's position embedding is resampled from the one RESIDENT in
 * src, then the fold and the split are recomputed.  The source is whatever src holds: if src was itself loaded or copied with a
 * resampling, this is a second resampling of already resampled values, not one from the checkpoint's grid -- copy from the engine
 * that holds the checkpoint's own embedding.  With equal img_size it is vit_engine_copy_weights (the mode is still checked).
 */
enum { VIT_POS_BICUBIC = 0, VIT_POS_BICUBIC_AA = 1 };
typedef struct {
    int src_img_size;   /* the checkpoint's input size; its grid is src_img_size / cfg.patch_size */
    int mode;           /* VIT_POS_* */
    int reserved;       /* must be 0 */
} vit_pos_resample;
int vit_engine_load_weights_resampled(vit_engine *e, const Network *weights, int count, const vit_pos_resample *rs);
int vit_engine_copy_weights_resampled(vit_engine *dst, vit_engine *src, int mode);

/*
 * Device-resident forward: d_images [n][C][S][S] fp32 -> d_probs [n][classes] fp32, both in
 * HBM, n arbitrary (processed in chunks of max_batch).  Asynchronous on `stream`
 * (a hipStream_t; NULL = the engine's own stream, then call vit_engine_sync()).
 * d_top1_label / d_top1_prob (device, n entries each) may be NULL.
 */
int vit_engine_forward_device(vit_engine *e, const float *d_images, int n, float *d_probs,
                              int *d_top1_label, float *d_top1_prob, void *stream);
int vit_engine_sync(vit_engine *e);

/*
 * Host-pointer forward with the reference's ownership rules (ViT_opencl.h:18): images[i] are
 * separately allocated CHW buffers, probs[i] caller-allocated [classes] rows.  Stages through
 * pinned buffers; blocking.
 */
int vit_engine_forward_host(vit_engine *e, const float *const *images, int n, float *const *probs);

/*
 * The same two forwards from 8-bit pixels, as image decoders produce them: images [S][S][C] uint8, channels interleaved.  The
 * engine normalises them on the device, in front of the patch embedding of each lane:
 *     x[c][h][w] = ((float)img[h][w][c] / 255.0f - mean[c]) / std[c]
 * (torchvision's ToTensor() + Normalize(mean, std); vithip_images_u8_to_f32), so the probabilities are bit-identical to the fp32
 * forward of the image normalised by that formula on the host, for every option and dtype.  A quarter of the fp32 bytes cross the
 * host gather and PCIe.  mean / std: HOST arrays of cfg.in_chans floats, read during the call.  VIT_ERR_ARG (the engine stays
 * usable) for NULL pointers, n <= 0, a non-finite mean or std, a zero std, in_chans > 4 or, device path, d_images not 4-byte
 * aligned -- and, checked before anything is enqueued, for an engine whose img_size is no multiple of 4 (even patch geometries
 * such as 518 = 37 x 14 or 42: the 8-bit and decoded-image kernels write 16 bytes of a pixel row at a time; the message names
 * img_size).  That holds for every _u8 and _images call below; the fp32-input calls take any even img_size.
 *
 * Device path: d_images [n][S][S][C] in HBM, asynchronous on `stream` like vit_engine_forward_device (a graph of use_graph is
 * keyed on the input kind and the mean / std values too).  The fp32 images live in the engine's staging until the call's
 * kernels have run.
 * Host path: images[i] separately allocated [S][S][C] buffers, uploaded as bytes through the pipeline of
 * vit_engine_forward_host (the first u8 call allocates 2 x max_batch images of byte staging on the device); blocking.
 */
int vit_engine_forward_device_u8(vit_engine *e, const unsigned char *d_images, int n, const float *mean, const float *std,
                                 float *d_probs, int *d_top1_label, float *d_top1_prob, void *stream);
int vit_engine_forward_host_u8(vit_engine *e, const unsigned char *const *images, int n, const float *mean, const float *std,
                               float *const *probs);

/*
 * Embedding outputs instead of probabilities.  With x the encoder output (the fp32 residual stream behind the last layer, T =
 * tokens rows of D = embed_dim per image) and y[i][t] = LayerNorm_final(x[i][t]) (the encoder_ln weights, vithip_layernorm_f32):
 *
 *   VIT_FEAT_CLS     out[i] = y[i][0]                                  [n][D]     the operand the classifier head reads
 *   VIT_FEAT_MEAN    out[i] = 1/P * sum_{t=F}^{T-1} y[i][t]            [n][D]     mean of the P patch tokens, rows F = 1 + R .. (timm global_pool='avg')
 *   VIT_FEAT_TOKENS  out[i][t] = y[i][t], class row first              [n][T][D]  all tokens (timm forward_features)
 *   VIT_FEAT_HEAD    out[i] = head(operand[i])                         [n][num_classes]  the head in force -- the checkpoint's or one
 *                    from vit_engine_set_head -- applied to its operand, no softmax: CLIP's projected image embedding when the head
 *                    slot holds visual_projection with a zero bias.  Without l2_normalize the rows are the bits
 *                    vit_engine_read_logits() returns for the chunk; read_logits after the call works and returns the un-normalised
 *                    rows.  A prune_last_layer engine prunes exactly when a probabilities call would; accounted to VIT_STAGE_HEAD.
 *
 * Rows are fp32 for both engine dtypes.  Except for HEAD, the head GEMM is not launched; the softmax never is.  CLS is the bits the head of a forward
 * call reads.  MEAN is one pass over x (vithip_layernorm_pool_f32): the normalised tokens are never stored, and an image's row
 * has the same bits wherever the image sits in whatever batch.  l2_normalize = 1 (CLS, MEAN and HEAD) divides each output row by
 * max(||row||_2, 1e-12) (torch.nn.functional.normalize).
 *
 * The four calls mirror the four forwards: the same images, chunking, lanes, stream rules and blocking behaviour; `out` takes the
 * place of the probabilities, rows of vit_engine_feature_row_elems() floats (device: one [n][row] array; host: caller-allocated
 * rows out[i]).  The host calls (re)allocate the pinned output staging for the widest row seen so far: a TOKENS call holds
 * 2 x max_batch x T x D floats of pinned and of device memory from then on.  If that does not fit, the call returns VIT_ERR_NOMEM,
 * the staging is back at its classes-sized start and the engine stays usable.
 * prune_last_layer engines: a CLS call uses the pruned last layer (same bits as unpruned); a MEAN or TOKENS call needs every token
 * of the last layer and runs it unpruned -- for that call only, not an error.  use_graph: the graph is keyed on the kind of output
 * too, so forwards and feature calls on the same n and pointers never replay each other's graph.  Profiling: the launches are
 * accounted to VIT_STAGE_LN.  vit_engine_read_logits() after a CLS, MEAN or TOKENS call is an error: nothing wrote logits.
 * VIT_ERR_ARG (the engine stays usable): NULL pointers, n <= 0, unknown kind, l2_normalize other than 0 / 1, l2_normalize with
 * TOKENS, and what the matching forward refuses.
 */
enum { VIT_FEAT_CLS = 0, VIT_FEAT_MEAN = 1, VIT_FEAT_TOKENS = 2, VIT_FEAT_HEAD = 4 /* 3 stays unassigned: callers know it as an unknown kind (VIT_ERR_ARG) */ };
typedef struct {
    int kind;          /* VIT_FEAT_* */
    int l2_normalize;  /* 0 / 1; not with TOKENS */
} vit_feature_spec;

/* floats per output row: D, D, tokens * D or (HEAD) num_classes; 0 on a bad spec */
size_t vit_engine_feature_row_elems(const vit_engine *e, const vit_feature_spec *spec);
int vit_engine_features_device(vit_engine *e, const float *d_images, int n, const vit_feature_spec *spec, float *d_out, void *stream);
int vit_engine_features_host(vit_engine *e, const float *const *images, int n, const vit_feature_spec *spec, float *const *out);
int vit_engine_features_device_u8(vit_engine *e, const unsigned char *d_images, int n, const float *mean, const float *std,
                                  const vit_feature_spec *spec, float *d_out, void *stream);
int vit_engine_features_host_u8(vit_engine *e, const unsigned char *const *images, int n, const float *mean, const float *std,
                                const vit_feature_spec *spec, float *const *out);

/*
 * The same four calls from decoded images of any size: the engine runs the whole evaluation transform of a ViT checkpoint
 *     Resize(resize_shorter) -> CenterCrop(cfg.img_size) -> ToTensor() -> Normalize(mean, std)
 * on the device, in one kernel in front of the patch embedding of each lane (vithip_images_u8_resize_crop_to_f32 in
 * vit_hip_kernels.h states the arithmetic: Pillow's 8-bit bilinear resize as torchvision runs it, bit for bit; bicubic instead after
 * vit_engine_set_resize_filter, below).  The outputs are bit-identical to the matching _u8 call on the bytes that torchvision's
 * Resize + CenterCrop give, for every option and dtype.
 *
 * images: a HOST array of n records in all four calls, read during the call only; pixels [height][width][cfg.in_chans] uint8, rows
 * packed, any address: DEVICE pointers in the _device_ calls, HOST pointers in the _host_ ones.  Everything else mirrors the _u8
 * calls: chunking, lanes, stream rules, blocking behaviour, outputs, prune_last_layer rules for features; the preprocessing
 * launches (one per 64 images of a lane) are accounted to VIT_STAGE_EMBED.
 * use_graph: these calls always run eagerly and leave a captured graph of the other calls alone, neither replayed nor destroyed --
 * its key would have to hold every pointer and size.
 * Host path: a piece of the pipeline of vit_engine_forward_host ends at the usual image count or where the next image's
 * height * width * in_chans bytes (each image's start rounded up to 16) would overflow a staging slot, whichever comes first.  A
 * slot holds max_batch * in_chans * img_size^2 * 4 bytes (the pinned fp32 staging, and as many bytes of device memory per slot that the
 * first such call allocates; VIT_ERR_NOMEM if it cannot, and the engine and its other calls go on working): sources that average up to
 * 4 x the pixels of the crop pass at full max_batch, larger ones in shorter pieces.  Rows are bit-identical whatever the cut.
 * VIT_ERR_ARG (the engine stays usable, nothing was enqueued): NULL images / pp / outputs, n <= 0, in_chans > 4, a non-finite mean or
 * std, a zero std, resize_shorter < cfg.img_size (torchvision would pad) or > 4096, a record with NULL pixels, a height or width
 * outside 1..16384 or a shorter side above 64 x resize_shorter, and (host path) an image that does not fit a slot alone; the message
 * names the record.
 */
typedef struct {
    const unsigned char *pixels; /* [height][width][in_chans], packed */
    int height, width;
} vit_image_u8;
typedef struct {
    int resize_shorter;          /* the crop is cfg.img_size */
    float mean[4], std[4];       /* the first cfg.in_chans are read */
} vit_preproc;
int vit_engine_forward_device_images(vit_engine *e, const vit_image_u8 *images, int n, const vit_preproc *pp, float *d_probs,
                                     int *d_top1_label, float *d_top1_prob, void *stream);
int vit_engine_forward_host_images(vit_engine *e, const vit_image_u8 *images, int n, const vit_preproc *pp, float *const *probs);
int vit_engine_features_device_images(vit_engine *e, const vit_image_u8 *images, int n, const vit_preproc *pp, const vit_feature_spec *spec,
                                      float *d_out, void *stream);
int vit_engine_features_host_images(vit_engine *e, const vit_image_u8 *images, int n, const vit_preproc *pp, const vit_feature_spec *spec,
                                    float *const *out);

/*
 * The resize filter of every _images call of this engine (the eight above and below: forward, features, cls_attention, intermediate,
 * host and device).  It belongs to a checkpoint's evaluation transform, so it is engine state: VIT_RESIZE_BILINEAR, the default, is
 * torchvision's own ViT transform; VIT_RESIZE_BICUBIC is Resize(R, interpolation=BICUBIC) on PIL images -- DINOv2, DINO, DeiT, MAE,
 * timm's vit_* configs -- bit for bit like the bilinear one (vithip_images_u8_resize_crop_to_f32_filter in vit_hip_kernels.h states
 * the arithmetic).  The outputs are then bit-identical to the matching _u8 call on the bytes that transform gives.
 * The setter takes effect from the next _images call.  The filter is read on the host when a call enqueues its work (the record check
 * of the call uses it too) and travels in that call's launches, so changing it between calls needs no synchronisation with work that
 * is still running; like every other call on an engine it must not run concurrently with another call on the same engine.  The
 * size limits are those of the bilinear filter.  Every engine has its own filter.  VIT_ERR_ARG for an unknown value (or a NULL
 * engine): the filter stays what it was.
 */
enum { VIT_RESIZE_BILINEAR = 0, VIT_RESIZE_BICUBIC = 1 };
int vit_engine_set_resize_filter(vit_engine *e, int filter);
int vit_engine_get_resize_filter(const vit_engine *e);  /* -1 for a NULL engine */

/*
 * The class token's attention over the tokens, in the LAST encoder layer, instead of probabilities: the DINO-style saliency map of a
 * ViT.  With q[i][h] the class row's query of image i and head h in that layer and k[i][h][t] the key of token t (T = tokens, the
 * class token's own key first, head_dim = embed_dim / num_heads: 64, or 72 .. 128 through vithip_cls_attention_*_hd):
 *
 *     s_t = (q . k_t) / sqrtf(head_dim);   p[i][h][t] = expf(s_t - max_t s) / sum_t expf(s_t - max)          (ViT_seq.c:156-190, query row 0)
 *
 *   VIT_ATTN_HEADS      out[i][h][t] = p[i][h][t]                                       [n][heads][T]  every row sums to 1
 *   VIT_ATTN_HEAD_MEAN  out[i][t] = (p[i][0][t] + p[i][1][t] + ...) / (float)heads      [n][T]         heads added in order, in fp32:
 *                                                                                       the HEADS bits of the same engine, reduced
 *
 * Rows are fp32 for both engine dtypes; the patch tokens are columns 1 + R..T-1 in raster order (register tokens, if any, columns 1..R).  The last layer runs its LayerNorm (or
 * the fold's statistics) and its QKV GEMM; then each lane runs vithip_cls_attention_* (vit_hip_kernels.h states the arithmetic) on
 * the Q and K it left.  Nothing else of that layer is launched, nor the final LayerNorm, the head or the softmax.  The map is the
 * softmax the forward itself uses for the class row: fp32 engines compute it in fp32, bf16 engines from the bf16 q and k of their
 * forward, with fp32 scores and softmax.  ln_fold and fp32_split select other arithmetic, as they do for probabilities.
 * An image's rows have the same bits whatever prune_last_layer and lanes are set to, wherever the image sits in whatever batch and
 * whichever of the six calls delivers the same pixels.  No atomics: calls are reproducible bit for bit.
 *
 * The six calls mirror the six features calls: the same images, chunking, lanes, stream rules and blocking behaviour; `out` takes
 * the place of the feature rows, rows of vit_engine_attention_row_elems() floats (device: one [n][row] array; host: caller-allocated
 * rows out[i]).  The host calls share the pinned output staging of the features calls and its rule: it is (re)allocated for the
 * widest row seen so far (HEADS: heads * T floats, wider than the classes-sized start for ViT-B/16); if that does not fit, the call
 * returns VIT_ERR_NOMEM, the staging is back at its classes-sized start and the engine stays usable.
 * use_graph: the graph is keyed on the kind of output and the attention kind too, so forwards, feature calls and attention calls
 * on the same n and pointers never replay each other's graph.  Profiling: the new launches (one per lane and chunk) are accounted
 * to VIT_STAGE_ATTN.  vit_engine_read_logits() after an attention call is an error: nothing wrote logits.
 * VIT_ERR_ARG (the engine stays usable, nothing was enqueued): NULL pointers, n <= 0, an unknown kind, reserved != 0, and what the
 * matching forward refuses.
 */
enum { VIT_ATTN_HEADS = 0, VIT_ATTN_HEAD_MEAN = 1 };
typedef struct {
    int kind;      /* VIT_ATTN_* */
    int reserved;  /* must be 0 */
} vit_attention_spec;

/* floats per output row: heads * tokens or tokens; 0 on a bad spec */
size_t vit_engine_attention_row_elems(const vit_engine *e, const vit_attention_spec *spec);
int vit_engine_cls_attention_device(vit_engine *e, const float *d_images, int n, const vit_attention_spec *spec, float *d_out, void *stream);
int vit_engine_cls_attention_host(vit_engine *e, const float *const *images, int n, const vit_attention_spec *spec, float *const *out);
int vit_engine_cls_attention_device_u8(vit_engine *e, const unsigned char *d_images, int n, const float *mean, const float *std,
                                       const vit_attention_spec *spec, float *d_out, void *stream);
int vit_engine_cls_attention_host_u8(vit_engine *e, const unsigned char *const *images, int n, const float *mean, const float *std,
                                     const vit_attention_spec *spec, float *const *out);
int vit_engine_cls_attention_device_images(vit_engine *e, const vit_image_u8 *images, int n, const vit_preproc *pp,
                                           const vit_attention_spec *spec, float *d_out, void *stream);
int vit_engine_cls_attention_host_images(vit_engine *e, const vit_image_u8 *images, int n, const vit_preproc *pp,
                                         const vit_attention_spec *spec, float *const *out);

/*
 * Intermediate-layer outputs instead of probabilities: the residual stream behind chosen encoder layers (DINOv2
 * get_intermediate_layers, timm forward_intermediates).  With x_l the fp32 residual stream behind encoder layer l (T = tokens rows of
 * D = embed_dim per image; layer 0 is the first layer, so x_l is what the oracle calls stages[l + 1]), f = the FINAL LayerNorm
 * (encoder_ln, as DINOv2 norm=True applies it to every tapped layer) when norm = 1 and the identity when norm = 0, P = g * g patch tokens at rows F = 1 + R .. and
 * K = num_layers, the row of image i is K blocks, block j for layer layers[j]:
 *
 *   VIT_TAP_CLS      block = f(x_l[i][0])                        [n][K][D]        = [n][K*D], the operand of a linear probe
 *   VIT_TAP_TOKENS   block[t] = f(x_l[i][t]), class row first,   [n][K][T][D]
 *                    then the register rows, then the patches
 *   VIT_TAP_PATCHES  block[p] = f(x_l[i][F + p]), p = 0..P-1     [n][K][P][D]
 *   VIT_TAP_MAP      block[d][p] = f(x_l[i][F + p])[d]           [n][K][D][g][g]  = [n][K*D][g][g], g = img_size / patch_size, patches in
 *                                                                                 raster order: the channel concatenation of a dense head
 *
 * Rows are fp32 for both engine dtypes.  Behind each tapped layer every lane launches vithip_tap_f32_prefix_eps (vit_hip_kernels.h; prefix = F) once, on
 * its own stream, from its rows of x into its images' blocks; normalised values are the bits vithip_layernorm_f32 gives, so a tap of
 * the last layer with norm = 1 is the bits of the matching features call (TOKENS, CLS), MAP is the transpose of PATCHES bit for bit,
 * and block j does not depend on which other layers are tapped.  Layers behind the deepest tap are not launched, nor the final
 * LayerNorm of the forward, the head or the softmax.  An image's row has the same bits whatever prune_last_layer and lanes are set to,
 * wherever the image sits in whatever batch and whichever of the six calls delivers the same pixels.  No atomics.
 *
 * The six calls mirror the six features calls: the same images, chunking, lanes, stream rules and blocking behaviour; `out` takes the
 * place of the feature rows, rows of vit_engine_intermediate_row_elems() floats (device: one [n][row] array; host: caller-allocated
 * rows out[i]).  The host calls share the pinned output staging of the features calls and its rule: it is (re)allocated for the widest
 * row seen so far (K * T * D floats for TOKENS); if that does not fit, the call returns VIT_ERR_NOMEM, the staging is back at its
 * classes-sized start and the engine stays usable.
 * prune_last_layer engines: the last layer runs pruned only when it is tapped and kind = VIT_TAP_CLS (same bits as unpruned); any other
 * kind that taps it runs it unpruned -- for that call only, not an error.  use_graph: the graph is keyed on the whole spec, so two calls
 * that differ in one layer never replay each other's graph; the _images calls run eagerly.  Profiling: the tap launches (one per lane,
 * chunk and tapped layer) are accounted to VIT_STAGE_LN.  vit_engine_read_logits() after an intermediate call is an error: nothing wrote
 * logits.
 * VIT_ERR_ARG (the engine stays usable, nothing was enqueued): NULL pointers, n <= 0, an unknown kind, norm other than 0 / 1, num_layers
 * outside 1..VIT_MAX_TAPS, a layer outside 0..depth-1 or not above the one before it (the message names the entry), reserved != 0, MAP
 * when img_size / patch_size does not give a square grid of P patches, and what the matching forward refuses.
 */
enum { VIT_TAP_CLS = 0, VIT_TAP_TOKENS = 1, VIT_TAP_PATCHES = 2, VIT_TAP_MAP = 3 };
#define VIT_MAX_TAPS 32
typedef struct {
    int kind;                  /* VIT_TAP_* */
    int norm;                  /* 1: the final LayerNorm (encoder_ln) applied to every tap, as DINOv2 norm=True; 0: the raw residual stream */
    int num_layers;            /* 1..VIT_MAX_TAPS */
    int layers[VIT_MAX_TAPS];  /* strictly increasing, 0 <= l < depth: the output of encoder layer l (oracle stages[l + 1]) */
    int reserved;              /* must be 0 */
} vit_intermediate_spec;

/* floats per output row: K * D, K * T * D, K * P * D or K * D * P; 0 on a bad spec */
size_t vit_engine_intermediate_row_elems(const vit_engine *e, const vit_intermediate_spec *spec);
int vit_engine_intermediate_device(vit_engine *e, const float *d_images, int n, const vit_intermediate_spec *spec, float *d_out, void *stream);
int vit_engine_intermediate_host(vit_engine *e, const float *const *images, int n, const vit_intermediate_spec *spec, float *const *out);
int vit_engine_intermediate_device_u8(vit_engine *e, const unsigned char *d_images, int n, const float *mean, const float *std,
                                      const vit_intermediate_spec *spec, float *d_out, void *stream);
int vit_engine_intermediate_host_u8(vit_engine *e, const unsigned char *const *images, int n, const float *mean, const float *std,
                                    const vit_intermediate_spec *spec, float *const *out);
int vit_engine_intermediate_device_images(vit_engine *e, const vit_image_u8 *images, int n, const vit_preproc *pp,
                                          const vit_intermediate_spec *spec, float *d_out, void *stream);
int vit_engine_intermediate_host_images(vit_engine *e, const vit_image_u8 *images, int n, const vit_preproc *pp,
                                        const vit_intermediate_spec *spec, float *const *out);

/*
 * Top-k class records instead of probabilities: the k most likely classes of every image (ImageNet top-5, "the five best guesses").
 * The row of image i is 2k 32-bit words,
 *
 *     row[0 .. k-1]   the labels (int32), best first
 *     row[k .. 2k-1]  their scores as fp32 bit patterns
 *
 * labels first, then bit patterns, as in the 8-byte records of vit_dp.h.  The score of a class is its probability (VIT_SCORE_PROB: the
 * bits the matching forward call of the same engine returns, and slot 0 is that call's top-1 record) or its logit (VIT_SCORE_LOGIT);
 * for both engine dtypes the fp32 logits are read.  Order: higher score first, among equal scores (==) the lower label first.  A
 * class whose score is NaN is not a candidate; slots left over when fewer than k candidates exist hold label 0x7fffffff and score
 * -1.0f (PROB) or -INFINITY (LOGIT) -- with PROB, one non-finite logit makes every probability of that image NaN and its whole row
 * empty slots, exactly the top-1 record a forward gives it; the other images of the batch are untouched.
 * (vithip_softmax_topk_f32 in vit_hip_kernels.h states the arithmetic.)
 *
 * The whole forward runs, the final LayerNorm and the head GEMM included; then each lane launches vithip_softmax_topk_f32 on its rows
 * of the logits in place of vithip_softmax_top1_f32: no [n][classes] array is written anywhere.  An image's row has the same bits
 * whatever prune_last_layer and lanes are set to, wherever the image sits in whatever batch and whichever of the six calls delivers the
 * same pixels.  prune_last_layer engines use the pruned last layer: only the class row is needed.  No atomics.
 *
 * The six calls mirror the six features calls: the same images, chunking, lanes, stream rules, blocking behaviour and _images eager
 * rule; `out` takes the place of the feature rows (device: one [n][2k] array of 32-bit words; host: caller-allocated rows out[i] of
 * 2k words).  On the host path only the records cross PCIe, 8k bytes per image instead of 4 * classes.  The host calls share the
 * pinned output staging of the features calls and its rule: it is (re)allocated for the widest row seen so far (2k words can exceed
 * the classes-sized start on a small head); if that does not fit, the call returns VIT_ERR_NOMEM, the staging is back at its
 * classes-sized start and the engine stays usable.
 * use_graph: the graph is keyed on the kind of output, k and score too, so forwards and top-k calls on the same n and pointers, or two
 * top-k calls that differ in k or score, never replay each other's graph.  Profiling: the launch (one per lane and chunk) is accounted
 * to VIT_STAGE_SOFTMAX.  vit_engine_read_logits() after a top-k call works: the head ran, and these are the logits the records of the
 * last chunk were taken from.
 * VIT_ERR_ARG (the engine stays usable, nothing was enqueued): NULL pointers, n <= 0, k outside 1..min(VIT_MAX_TOPK, num_classes)
 * (the message names both), an unknown score, reserved != 0, and what the matching forward refuses.
 */
enum { VIT_SCORE_PROB = 0, VIT_SCORE_LOGIT = 1 };
#define VIT_MAX_TOPK 64
typedef struct {
    int k;         /* 1..min(VIT_MAX_TOPK, num_classes) */
    int score;     /* VIT_SCORE_* */
    int reserved;  /* must be 0 */
} vit_topk_spec;

/* 32-bit words per output row: 2k; 0 on a bad spec */
size_t vit_engine_topk_row_elems(const vit_engine *e, const vit_topk_spec *spec);
int vit_engine_topk_device(vit_engine *e, const float *d_images, int n, const vit_topk_spec *spec, int *d_out, void *stream);
int vit_engine_topk_host(vit_engine *e, const float *const *images, int n, const vit_topk_spec *spec, int *const *out);
int vit_engine_topk_device_u8(vit_engine *e, const unsigned char *d_images, int n, const float *mean, const float *std,
                              const vit_topk_spec *spec, int *d_out, void *stream);
int vit_engine_topk_host_u8(vit_engine *e, const unsigned char *const *images, int n, const float *mean, const float *std,
                            const vit_topk_spec *spec, int *const *out);
int vit_engine_topk_device_images(vit_engine *e, const vit_image_u8 *images, int n, const vit_preproc *pp, const vit_topk_spec *spec,
                                  int *d_out, void *stream);
int vit_engine_topk_host_images(vit_engine *e, const vit_image_u8 *images, int n, const vit_preproc *pp, const vit_topk_spec *spec,
                                int *const *out);

/*
 * Pooled and multi-layer classifier heads: another operand for the head GEMM, as engine state.  The checkpoint's own head (tensors
 * base+2, base+3 of the Network) reads LayerNorm_final(x[i][0]); the published classifiers of DINOv2 and of timm's average-pooled
 * ViTs read something else.  With f the final LayerNorm (tensors base, base+1), x_l the residual stream behind encoder layer l (layer
 * l = oracle stages[l + 1], as in vit_intermediate_spec), P = g * g patch tokens at rows F = 1 + R .. and K = num_cls_layers, the operand row of image i is
 *
 *     [ f(x_{l_0}[i][0]) | ... | f(x_{l_{K-1}}[i][0]) | pooled ]          in_features = (K + (pool != NONE)) * D floats
 *
 *     VIT_HEAD_POOL_NONE        no pooled block
 *     VIT_HEAD_POOL_AVG         pooled = 1/P * sum_{t=1..P} f(x_last[i][t])       norm, then mean (DINOv2 linear heads; timm avg pool)
 *     VIT_HEAD_POOL_AVG_FCNORM  pooled = f(1/P * sum_{t=1..P} x_last[i][t])       mean, then norm (timm fc_norm, MAE fine-tuned ViTs:
 *                                                                                 the caller puts fc_norm.weight / .bias into base, base+1)
 *
 * over the patch tokens of the LAST layer, and logits = operand . weight^T + bias: weight [num_classes][in_features] row-major
 * (nn.Linear.weight), bias [num_classes], HOST fp32 arrays read during the call and uploaded as they are (no rounding) to an
 * allocation of the head's own.  The Network layout, the weight image and the cache file do not know about it.
 *
 *     DINOv2 linear head, 1 layer    K = 1, cls_layers = {depth-1}, AVG          weight columns [cls | mean of patch tokens]
 *     DINOv2 linear head, 4 layers   K = 4, cls_layers = {depth-4..depth-1}, AVG  weight columns [cls of the four layers, earliest first | mean]
 *     timm global_pool='avg'         K = 0, AVG;   with fc_norm: K = 0, AVG_FCNORM
 *     another linear probe           K = 1, cls_layers = {depth-1}, NONE: swaps probes on one resident backbone
 *
 * Every probability and top-k call, vit_engine_read_logits and the callers built on them use the head in force.  Bits: a class block
 * is the row of an intermediate call (VIT_TAP_CLS, norm = 1) for that layer, an AVG block the row of a VIT_FEAT_MEAN features call
 * without L2 -- the same launches, pointed at the operand; AVG_FCNORM is vithip_pool_layernorm_f32 (vit_hip_kernels.h).  The head GEMM is
 * fp32 on both engine dtypes.  An image's operand, logits and probabilities have the same bits whatever lanes is set to, wherever the
 * image sits in the batch and whichever of the six input paths delivers the pixels.  All `depth` layers always run.  The features,
 * attention and intermediate calls do not see the head.
 * prune_last_layer engines keep pruning with pool = NONE (only class rows are read; same bits); with a pooled block the last layer
 * runs unpruned for that call -- not an error, the rule of MEAN features.
 *
 * vit_engine_set_head: synchronises the device and drops a captured graph, as a weight install does.  spec == NULL (weight and bias
 * must then be NULL) restores the checkpoint's own head -- and so does EVERY weight install (vit_engine_load_weights*,
 * vit_engine_load_weight_image, vit_engine_copy_weights*): set the head again behind it.  A head is not copied by copy_weights: set it
 * per engine.  The new weight, bias and operand rows ([max_batch][in_features]) are allocated before the old ones are freed: on
 * VIT_ERR_NOMEM the previous head stays in force and the engine stays usable.  VIT_ERR_STATE: no weights loaded yet.  VIT_ERR_ARG,
 * nothing changed: a NULL weight or bias with a spec, num_cls_layers outside 0..VIT_MAX_TAPS, a layer outside 0..depth-1 or not above
 * the one before it (the message names the entry), an unknown pool, reserved != 0, an empty operand (K = 0 and NONE).
 * vit_engine_read_head_operand: debug/test tap beside vit_engine_read_logits -- the operand rows of the most recent chunk (rows of
 * in_features floats; with the checkpoint's own head, of D floats); an error where read_logits is one.
 */
enum { VIT_HEAD_POOL_NONE = 0, VIT_HEAD_POOL_AVG = 1, VIT_HEAD_POOL_AVG_FCNORM = 2 };
typedef struct {
    int num_cls_layers;            /* 0..VIT_MAX_TAPS */
    int cls_layers[VIT_MAX_TAPS];  /* strictly increasing, 0 <= l < depth (layer l = oracle stages[l + 1], as in vit_intermediate_spec) */
    int pool;                      /* VIT_HEAD_POOL_*: over the patch tokens (rows 1 + R..T-1) of the LAST layer */
    int reserved;                  /* must be 0 */
} vit_head_spec;
/* (num_cls_layers + (pool != NONE)) * D; 0 on a bad spec */
size_t vit_engine_head_in_features(const vit_engine *e, const vit_head_spec *spec);
int vit_engine_set_head(vit_engine *e, const vit_head_spec *spec, const float *weight, const float *bias);
int vit_engine_read_head_operand(vit_engine *e, float *dst, int rows);

/*
 * Dense linear heads: a class per pixel from the patch tokens, on the device -- the published segmentation heads of DINOv2 (mmseg
 * BNHead, `linear` on one layer and `ms` on four): BatchNorm + 1x1 conv over the channel concatenation of the tapped layers' patch
 * tokens, the logits resized bilinearly to the image, then the argmax.  The head is engine state, beside and independent of the
 * classifier head: setting or removing one never disturbs the other.
 *
 * With K = num_layers, D = embed_dim, P = g * g patches (g = img_size / patch_size; rows 1 + R..T-1) and A_j the [P][D] rows of an
 * intermediate call of VIT_TAP_PATCHES with the head's norm for layer layers[j], an image's logits [P][num_classes] are
 *     logits = bias + sum_j A_j . weight[:, j*D .. (j+1)*D]^T
 * weight [num_classes][K * D] row-major: the 1x1 conv's weight, the earliest layer's columns first (a BatchNorm in front of it is
 * folded on the host: vit_dense_head_fold_batchnorm, vit_io.h); bias [num_classes]; HOST fp32 arrays read during the call and uploaded
 * as they are.  Bits: a chain of vithip_gemm_f32 launches with arith = 0 (fp32 MFMA, as the classifier head uses, on both engine
 * dtypes: the residual stream is fp32 on both), in layer order -- the first with VITHIP_EPI_BIAS, W = weight, ldw = K * D, the later
 * ones with VITHIP_EPI_BIAS_RESIDUAL, a zero bias, W = weight + j * D and residual = C.  Each tap and its GEMM run directly behind
 * their layer (the next layer overwrites the stream): the head holds one [max_batch][P][D] scratch and the logits
 * [max_batch][P][num_classes], allocated by vit_engine_set_dense_head.
 *
 * vit_engine_set_dense_head: the rules of vit_engine_set_head.  It synchronises the device and drops a captured graph; the new
 * allocations are made before the old ones are freed, on VIT_ERR_NOMEM the previous dense head stays in force; spec == NULL (weight
 * and bias must then be NULL) removes the head; EVERY weight install removes it, and the copy calls do not carry it: set it again
 * behind them, per engine.  VIT_ERR_STATE: no weights loaded yet.  VIT_ERR_ARG, nothing changed: a NULL weight or bias with a spec,
 * num_layers outside 1..VIT_MAX_TAPS, a layer outside 0..depth-1 or not above the one before it (the message names the entry), norm
 * other than 0 / 1, num_classes outside 1..255, reserved != 0, an img_size / patch_size that does not give a square grid of P
 * patches.
 *
 * The six calls mirror the six intermediate calls argument for argument (`out` is untyped: labels are bytes): the same images,
 * chunking, lanes, stream rules, blocking behaviour, pinned output staging (sized in bytes; VIT_ERR_NOMEM puts it back at its
 * classes-sized start), graph keying on the whole spec and eager _images calls.  Output rows, vit_engine_dense_row_bytes() bytes each
 * (device: one [n][row] array, any alignment for LABELS, 4-byte aligned for GRID; host: caller-allocated rows out[i]):
 *
 *   VIT_DENSE_GRID    fp32 [num_classes][g][g]: entry [c][p] the logit of patch p in raster order, the transpose of the chain above
 *   VIT_DENSE_LABELS  uint8 [out_h][out_w]: the argmax over the classes of F.interpolate(grid, (out_h, out_w), mode="bilinear",
 *                     align_corners=False) -- vithip_dense_upsample_argmax_f32 (vit_hip_kernels.h) states the arithmetic and the order:
 *                     higher wins, among equal values the lower label, a NaN value is no candidate, a pixel without one gets 255.  The
 *                     full-resolution logits are never stored.  out_h = out_w = 0 means img_size x img_size.
 *
 * Layers behind the deepest tap are not launched, nor the final LayerNorm of the forward, the classifier head or the softmax;
 * prune_last_layer engines run a tapped last layer unpruned for that call.  An image's row has the same bits whatever lanes and
 * prune_last_layer are set to, wherever the image sits in whatever batch and whichever of the six calls delivers the same pixels.
 * Non-finite values in one image reach only that image's row.  Profiling: the taps are accounted to VIT_STAGE_LN, the GEMMs to
 * VIT_STAGE_HEAD, the upsampling (or the transpose) to VIT_STAGE_SOFTMAX.  vit_engine_read_logits() after a dense call is an error:
 * nothing wrote the classifier's logits.
 * VIT_ERR_STATE: no dense head set.  VIT_ERR_ARG (the engine stays usable, nothing was enqueued): NULL pointers, n <= 0, an unknown
 * kind, reserved != 0, an out_h or out_w that is not 0 (GRID) or, with 0 standing for img_size, each on its own, outside 1..4096
 * (LABELS), and what the matching forward refuses.
 * Not covered: depth heads (class-token concatenation and bins), sliding-window inference, mapping the labels back through
 * Resize / CenterCrop -- the labels are those of the img_size x img_size crop the engine saw.
 */
typedef struct {
    int num_layers;            /* 1..VIT_MAX_TAPS */
    int layers[VIT_MAX_TAPS];  /* strictly increasing, 0 <= l < depth, as in vit_intermediate_spec */
    int norm;                  /* 1: final LayerNorm on every tapped layer (DINOv2), 0: raw stream */
    int num_classes;           /* 1..255 */
    int reserved;              /* must be 0 */
} vit_dense_head_spec;
int vit_engine_set_dense_head(vit_engine *e, const vit_dense_head_spec *spec, const float *weight, const float *bias);

enum { VIT_DENSE_LABELS = 0, VIT_DENSE_GRID = 1 };
typedef struct {
    int kind;          /* VIT_DENSE_* */
    int out_h, out_w;  /* LABELS: 0 = img_size, else 1..4096; GRID: must be 0 */
    int reserved;      /* must be 0 */
} vit_dense_spec;

/* bytes per output row: out_h * out_w (LABELS) or num_classes * g * g * 4 (GRID); 0 on a bad spec or without a dense head */
size_t vit_engine_dense_row_bytes(const vit_engine *e, const vit_dense_spec *spec);
int vit_engine_dense_device(vit_engine *e, const float *d_images, int n, const vit_dense_spec *spec, void *d_out, void *stream);
int vit_engine_dense_host(vit_engine *e, const float *const *images, int n, const vit_dense_spec *spec, void *const *out);
int vit_engine_dense_device_u8(vit_engine *e, const unsigned char *d_images, int n, const float *mean, const float *std,
                               const vit_dense_spec *spec, void *d_out, void *stream);
int vit_engine_dense_host_u8(vit_engine *e, const unsigned char *const *images, int n, const float *mean, const float *std,
                             const vit_dense_spec *spec, void *const *out);
int vit_engine_dense_device_images(vit_engine *e, const vit_image_u8 *images, int n, const vit_preproc *pp, const vit_dense_spec *spec,
                                   void *d_out, void *stream);
int vit_engine_dense_host_images(vit_engine *e, const vit_image_u8 *images, int n, const vit_preproc *pp, const vit_dense_spec *spec,
                                 void *const *out);

/*
 * CLIP image towers (OpenAI / OpenCLIP ViT-B/32, B/16, L/14): VIT_MLP_QUICKGELU (or VIT_MLP_GELU for OpenCLIP checkpoints trained with
 * plain GELU) in vit_config, and the three pieces below; the projected embedding is a features call of VIT_FEAT_HEAD with the head
 * slot holding visual_projection (num_classes = projection_dim, zero bias).  INTEGRATION.md has the checkpoint mapping.
 *
 * vit_engine_set_layernorm_eps: the epsilon of EVERY LayerNorm the engine runs -- the encoder's, the fold's statistics passes and the
 * finalise launch behind the stats-producing GEMMs, the final LayerNorm, the pooled blocks, the normalised taps and the pre-norm.  A
 * DOUBLE, added to the variance in double before the cast; the default is exactly the double 1e-6 (VITHIP_LN_EPS; CLIP: 1e-5, HF
 * ViTModel: 1e-12).  Architecture, not checkpoint data: it PERSISTS across weight installs, and the copy calls do not carry it.
 * Synchronises the device and drops a captured graph, as vit_engine_set_head does.  VIT_ERR_ARG, nothing changed: eps not finite or
 * not > 0.  (The gamma/beta weight fold does not depend on it.)
 *
 * vit_engine_set_pre_norm: a LayerNorm in front of layer 0 (CLIP's ln_pre, transformers' pre_layrnorm), applied to [cls | patches] +
 * pos; its output IS the residual stream.  gamma and beta are HOST arrays of embed_dim floats, uploaded as they are to an allocation
 * of the engine's own.  NULL, NULL removes it; one NULL alone is VIT_ERR_ARG.  Behind the embedding each lane runs one LayerNorm in
 * place on its n * T rows of the fp32 residual stream (both engine dtypes), with the engine's epsilon, accounted to VIT_STAGE_LN.
 * Intermediate calls (norm = 0) return the stream behind each layer as ever (hidden_states[l + 1] of transformers); nothing returns
 * the pre-norm's own output.  The rules of vit_engine_set_head: it synchronises the device and drops a captured graph; EVERY weight
 * install (vit_engine_load_weights*, vit_engine_load_weight_image, vit_engine_copy_weights*) removes it: set it again behind it; it
 * is not copied by copy_weights: set it per engine.  The new allocation is made before the old one is freed: on VIT_ERR_NOMEM the
 * previous pre-norm stays in force and the engine stays usable.  VIT_ERR_STATE: no weights loaded yet.
 */
int vit_engine_set_layernorm_eps(vit_engine *e, double eps);
double vit_engine_get_layernorm_eps(const vit_engine *e);
int vit_engine_set_pre_norm(vit_engine *e, const float *gamma, const float *beta);

/*
 * The fp32 GEMMs' helper-piece hand-over (csrc/vit_gemm_persistent.hip) since the last call, summed over the lanes: tiles whose
 * first K-steps came from a helper workgroup / tiles whose owner found no piece when it looked and computed all of it.  The
 * second number is lost time, never a wrong result (nothing in the hand-over waits or gives up).  Synchronises the device.
 */
int vit_engine_handover_stats(vit_engine *e, long *taken, long *recomputed);

/* Debug/test taps: copy the logits of the most recent chunk (rows = images of that chunk; an error after a features, attention or
 * intermediate call, which write none; after a top-k call the logits its records were taken from). */
int vit_engine_read_logits(vit_engine *e, float *dst, int rows);
/* Where a MEAN features chunk of nb <= max_batch images would put things inside the engine's y allocation (max_batch * tokens *
 * embed_dim floats), for lane `lane` under the current lane setting; launches nothing.  Byte offsets from the allocation's start:
 * range[0..1] the lane's pooling scratch, [2..3] the lane's rows of y, [4..5] the lane's bf16 copy of x (0, 0 when it has none
 * there).  Lanes run on independent streams, so a lane's scratch must lie inside its own y rows and clear of every other lane's
 * ranges (tests/test_gpu_features.py).  Returns the number of lanes the chunk uses, -1 on bad arguments. */
int vit_engine_debug_pool_scratch(vit_engine *e, int nb, int lane, size_t range[6]);

int vit_engine_get_stage_times(vit_engine *e, vit_stage_times *out);  /* syncs, then reports */
void vit_engine_reset_stage_times(vit_engine *e);
int vit_engine_set_profile(vit_engine *e, int on);
int vit_engine_set_lanes(vit_engine *e, int lanes);

#ifdef __cplusplus
}
#endif
#endif /* VIT_ENGINE_H */
