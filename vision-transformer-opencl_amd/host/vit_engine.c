/*
 * host/vit_engine.c -- batched ViT forward, host orchestration in C over the HIP C-ABI.
 *
 * Follows the stage order of the reference's forward (ViT_seq.c:337-439 / ViT_opencl.c:785-883)
 * with the whole chunk of images as the GEMM M dimension:
 *
 *   patch_embed (conv_proj + flatten_transpose + class_token + pos_emb, one implicit GEMM)
 *   depth x { LN1 -> QKV GEMM -> fused attention -> out_proj GEMM (+bias +residual, in place)
 *             LN2 -> fc1 GEMM (+bias +GELU) -> fc2 GEMM (+bias +residual, in place) }
 *   LN on the class-token rows only -> head GEMM -> softmax + top-1
 *   (one head, vit_head: the checkpoint's own is the instance {class block of the last layer} over z; every kind of final block --
 *    class, pooled, tap -- has one writer, whoever asks for it;
 *    a features call ends instead in the final LN of the rows it returns, or in the fused LN + mean over the patch tokens;
 *    an attention call stops the last layer behind its QKV GEMM and stores the class token's softmax row;
 *    an intermediate call copies rows of x out behind the layers it taps and stops behind the deepest of them;
 *    a dense call walks the layers of the dense head the same way, with a tap and a GEMM into per-patch logits behind each, and ends in
 *    the upsample + argmax launch that turns them into a label per pixel)
 *
 * Weights are validated and uploaded once (the reference re-uploads them per op per image, e.g. ViT_opencl.c:136,630-631); every
 * install route ends in finish_install, which derives the folded and pre-split operands and resolves, per layer, what each GEMM and
 * LayerNorm reads (vit_layer_ops): the stages index no tensor.  Activations never leave HBM between stages (the reference reads
 * every stage back to the host).
 */
#include "vit_engine.h"

#include <limits.h>
#include <math.h>
#include <stdarg.h>
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <omp.h>
#include <string.h>

#include "vit_hip_kernels.h"
#include "vit_io.h"

#define VIT_MAX_LANES 4
#define MAX_EVENTS 4096   /* stage brackets kept in flight before they are read back */
#define VIT_MAX_U8_CHANS 4 /* vithip_images_u8_to_f32 */

/* What a forward reads, besides where: fp32 images [C][S][S] as the model takes them, 8-bit pixels [S][S][C] that stage_embed
 * normalises into fp32 staging in front of the patch embedding, or records of decoded 8-bit images of any size that it resizes,
 * crops and normalises into the same staging (vithip_images_u8_resize_crop_to_f32).  Zero-filled before use: the graph cache
 * compares it bytewise. */
enum { VIT_IN_F32 = 0, VIT_IN_U8 = 1, VIT_IN_IMAGES = 2 };
typedef struct {
    int kind;           /* VIT_IN_* */
    int resize_shorter; /* VIT_IN_IMAGES */
    int resize_filter;  /* VIT_IN_IMAGES: the engine's filter when the call began (VIT_RESIZE_* = VITHIP_RESIZE_*) */
    float mean[VIT_MAX_U8_CHANS], std[VIT_MAX_U8_CHANS];
} vit_input;
_Static_assert(VIT_RESIZE_BILINEAR == VITHIP_RESIZE_BILINEAR && VIT_RESIZE_BICUBIC == VITHIP_RESIZE_BICUBIC, "one numbering of the filters");
_Static_assert(sizeof(vit_image_u8) == sizeof(vithip_image_u8) && offsetof(vit_image_u8, pixels) == offsetof(vithip_image_u8, pixels) &&
                   offsetof(vit_image_u8, height) == offsetof(vithip_image_u8, height) &&
                   offsetof(vit_image_u8, width) == offsetof(vithip_image_u8, width),
               "the engine hands its callers' records to the kernel launcher as they are");

/* What a forward writes, besides where: probabilities [n][classes] and the optional top-1 records, the embedding rows `spec`
 * asks for (stage_features), the class token's attention over the tokens in the last layer (stage_cls_attention), or the residual
 * stream behind the layers `tap` names (stage_tap), [n][row] floats -- or, behind the head, the k best classes as records in
 * place of the probabilities (stage_head; 32-bit words, as many bytes as a float each) -- or the rows of a dense call
 * (stage_dense_out: labels, a byte each, or the fp32 grid).  What the engine knows of each kind, the bytes of its row among it, is
 * the kind's row of OUT_KINDS.  Zero-filled before use (output_fault): the graph cache compares it bytewise.  The pointers are those
 * of the call's (or chunk's) first image. */
enum { VIT_OUT_PROBS = 0, VIT_OUT_FEATURES = 1, VIT_OUT_ATTENTION = 2, VIT_OUT_INTERMEDIATE = 3, VIT_OUT_TOPK = 4, VIT_OUT_DENSE = 5, VIT_OUT_KINDS };
typedef struct {
    int kind;              /* VIT_OUT_*: which member of the union is in use (_PROBS: none), and what dst holds */
    int zero;              /* always 0: with it the struct has no padding, which a bytewise comparison would read */
    union {                /* the kind's checked spec; the bytes behind it stay zero */
        vit_feature_spec spec;     /* _FEATURES */
        int attn_kind;             /* _ATTENTION: VIT_ATTN_* */
        vit_intermediate_spec tap; /* _INTERMEDIATE: layers[num_layers..] zero */
        vit_topk_spec topk;        /* _TOPK: dst = the records, [n][2k] 32-bit words */
        vit_dense_spec dense;      /* _DENSE: out_h / out_w resolved; the head is engine state */
    };
    float *dst;
    int *label;            /* _PROBS: top-1 (may be NULL) */
    float *prob;
} vit_output;
_Static_assert(sizeof(vit_output) == 2 * sizeof(int) + sizeof(vit_intermediate_spec) + 3 * sizeof(void *) &&
                   sizeof(vit_intermediate_spec) == (4 + VIT_MAX_TAPS) * sizeof(int) && sizeof(vit_intermediate_spec) % sizeof(void *) == 0,
               "vit_output must stay free of padding: the graph cache compares it bytewise");
_Static_assert(VIT_SCORE_PROB == VITHIP_SCORE_PROB && VIT_SCORE_LOGIT == VITHIP_SCORE_LOGIT && VIT_MAX_TOPK == VITHIP_MAX_TOPK,
               "one numbering of the scores, one bound on k");

/* The resolved operands of the forward.  A GEMM's: W [N][K] in the engine's GEMM dtype, fp32 bias [N], the column sums of W where
 * the LayerNorm fold's epilogue subtracts mean * colsum (else NULL), W's pre-split image on split engines (else NULL). */
typedef struct { const void *W; const float *bias, *colsum; const void *w_split; } vit_gemm_ops;
typedef struct { const float *ln1_g, *ln1_b, *ln2_g, *ln2_b; vit_gemm_ops qkv, out, fc1, fc2; } vit_layer_ops;
typedef struct { const float *cls, *conv_w, *conv_b, *pos; const unsigned short *conv_w16; /* bf16 engines */ } vit_embed_ops;
typedef struct { const float *ln_g, *ln_b; vit_gemm_ops head; } vit_final_ops;
/* The classifier head in force: the checked spec (cls_layers behind num_cls_layers zero), the operand's width `in` =
 * (num_cls_layers + (pool != NONE)) * D, the head GEMM's W [num_classes][in] and bias, the operand rows [max_batch][in].  owned: the
 * three are allocations of the head's own (W with a zeroed tail pad behind it, as wblob has), which go with it. */
typedef struct { vit_head_spec spec; size_t in; vit_gemm_ops ops; float *operand; int owned; } vit_head;
/* The dense head in force (vit_engine_set_dense_head; num_layers == 0: none): the checked spec (layers behind num_layers zero), the
 * 1x1 conv's W [num_classes][num_layers * D] (a zeroed tail pad behind it) and bias, a zero bias for the chain's later GEMMs, the
 * patch rows of the layer just tapped [max_batch][P][D] and the logits [max_batch][P][num_classes]: five allocations of its own. */
typedef struct { vit_dense_head_spec spec; float *W, *bias, *zero_bias, *rows, *logits; } vit_dense_head;

struct vit_engine {
    vit_config cfg;
    vit_engine_options opt;
    int tokens;                  /* T = prefix + patches rows per image: class token, register tokens, patch tokens */
    int prefix, patches;         /* 1 + VIT_REGISTER_TOKENS: the row of the first patch token; vit_config_patches */
    int n_weights;
    char err[512];

    vithip_stream_t stream;      /* engine-owned in-order stream */
    vithip_stream_t aux_stream[VIT_MAX_LANES - 1]; /* extra lanes of a chunk (forward_chunk) */
    vithip_event_t ev_fork, ev_join[VIT_MAX_LANES - 1];
    float *wblob;                /* all weights, ONE allocation: [fp32 section | bf16 GEMM operands] (vit_weight_image) */
    size_t wblob_bytes;          /* bytes of it that carry data (the allocation has a read-only tail pad behind) */
    float **w;                   /* device pointer per weight index */
    unsigned short *wblob16;     /* the bf16 section inside wblob (dtype bf16 only) */
    int fold;                    /* LayerNorm fold active (vit_engine_options.ln_fold) */
    int split;                   /* encoder GEMMs on the three-piece split (vit_engine_options.fp32_split; fp32 engines) */
    /* the operands derived from the weights by every install (finish_install); their layout: "derived operands" below */
    void *wfold;                 /* folded in_proj and fc1: bf16 (bf16 engines) or the fp32 products gamma * W (fp32 engines) */
    float *wfoldf;               /* their column sums and folded biases */
    unsigned char *wsplit;       /* split engines: the pre-split images (vithip_split3_weights_f32) of the four encoder GEMM weights */
    size_t wsplit_off[4], wsplit_layer; /* byte offset of each image inside a layer's, and a layer's bytes */
    /* what every GEMM and LayerNorm of the forward reads, resolved by every install (resolve_operands): pointers into the above */
    vit_embed_ops embed;
    vit_layer_ops *layer;        /* [depth] */
    vit_final_ops final;
    float *ln_rows32;            /* fp32 engines: (rstd, mean) per token row [max_batch * tokens][2], then per class row [max_batch][2] */
    float *ln_part32;            /* ... and the residual GEMMs' scratch for them: [embed_dim / 64][rows][2] per lane (vithip_gemm_args.stats_partials) */
    int lane_cap;                /* most images one lane may hold (32-bit buffer offsets of the fp32 kernels) */
    void *gemm_ws[VIT_MAX_LANES]; /* per lane in use (= per stream): vithip_gemm_args.workspace handles */
    long handover_taken, handover_recomputed;
    int n_cus;                   /* compute units of the device */
    /* use_graph: the captured forward and what it was captured for */
    vithip_graph_t graph;
    const void *g_images; vit_input g_in; vit_output g_out; int g_n;
    unsigned short **w16;        /* per weight index; NULL for tensors that stay fp32 */
    int weights_loaded;
    int resize_filter;           /* VIT_RESIZE_*: the filter of the _images calls (vit_engine_set_resize_filter) */
    double ln_eps;               /* the epsilon of every LayerNorm the engine runs (vit_engine_set_layernorm_eps): architecture, kept across installs */
    float *pre_g, *pre_b;        /* the LayerNorm in front of layer 0 (vit_engine_set_pre_norm), the engine's own allocation; NULL: none */

    /* workspace for max_batch images */
    float *x, *y, *qkv, *hbuf, *z, *logits;
    /* the one classifier head: the checkpoint's own (restore_own_head) or a caller's (vit_engine_set_head); no stage tells them apart */
    vit_head head;
    vit_dense_head dense;
    /* host-pointer path: double-buffered staging so that gather + H2D of piece i+1 overlap compute of piece i */
    float *in_stage[2], *out_stage[2];   /* device */
    float *pin_in[2], *pin_out[2];       /* pinned host */
    size_t out_row_cap;                  /* BYTES per image out_stage / pin_out hold: classes floats, or the widest row seen */
    vithip_stream_t copy_stream;
    vithip_event_t ev_h2d[2], ev_done[2];
    /* 8-bit input: the host path's byte staging (allocated by the first u8 host call); the device path normalises into
     * in_stage[0], and ev_in_stage (recorded behind it on the caller's stream) keeps the next host call's uploads behind it */
    unsigned char *in8_stage[2];
    /* decoded images of any size (the _images calls): the host path's byte staging, as many bytes per slot as pin_in holds
     * (allocated by the first such host call); the records of the piece in front of the kernel; the pieces' first images */
    unsigned char *img_stage[2];
    vithip_image_u8 *img_recs;   /* max_batch */
    size_t *img_off;             /* max_batch + 1: byte offsets of a piece's images inside a slot */
    int *piece_lo; int piece_cap;
    vithip_event_t ev_in_stage;
    int in_stage_pending;
    int last_rows;

    /* stage profiling */
    vithip_event_t ev[2 * MAX_EVENTS];
    int ev_stage[MAX_EVENTS];
    int ev_used;
    int ev_ready;
    long pending_images;         /* images whose brackets are still in the pool */
    vit_stage_times times;
};

/* element i of an array of esz-byte elements */
static void *at(const void *p, size_t i, size_t esz) { return (char *)p + i * esz; }

/* The weight order (ViT_seq.c:366-426): w[0..3] below, then VIT_WEIGHTS_PER_LAYER tensors per layer in the order of LW_*, then the
 * final LayerNorm's gamma and beta and the head's weight and bias. */
enum { W_CLS, W_CONV_W, W_CONV_B, W_POS, W_LAYER0 };
enum { LW_LN1_G, LW_LN1_B, LW_QKV_W, LW_QKV_B, LW_OUT_W, LW_OUT_B, LW_LN2_G, LW_LN2_B, LW_FC1_W, LW_FC1_B, LW_FC2_W, LW_FC2_B };
_Static_assert(LW_FC2_B + 1 == VIT_WEIGHTS_PER_LAYER, "LW_* names every tensor of a layer");

/* The derived operands' layout, per layer (resolve_operands fills them, and names the slots):
 *   wfold   [gamma1-folded in_proj 3D x D | gamma2-folded fc1 H1 x D], elements of the engine's GEMM dtype
 *   wfoldf  [colsum qkv 3D | bias qkv 3D | colsum fc1 H1 | bias fc1 H1]        (H1 = VIT_FC1_ROWS: H, or 2H under SwiGLU)
 *   wsplit  the images of [qkv | out_proj | fc1 | fc2] at wsplit_off[0..3], wsplit_layer bytes (vit_engine_create) */
static size_t fold_w_elems(const vit_config *c) { return (3 * (size_t)c->embed_dim + (size_t)VIT_FC1_ROWS(c)) * (size_t)c->embed_dim; }
static size_t fold_f_elems(const vit_config *c) { return 6 * (size_t)c->embed_dim + 2 * (size_t)VIT_FC1_ROWS(c); }

/* ------------------------------------------------------------------------------------------ */

vit_config vit_config_b16(void) {
    vit_config c = {224, 16, 3, 1000, 768, 12, 12, 3072};
    return c;
}

int vit_config_patches(const vit_config *cfg) {
    int g = cfg->img_size / VIT_PATCH_SIZE(cfg);
    return g * g;
}

/* class token, register tokens, patch tokens: the order of the rows */
int vit_config_tokens(const vit_config *cfg) { return 1 + VIT_REGISTER_TOKENS(cfg) + vit_config_patches(cfg); }

size_t vit_config_weight_size(const vit_config *cfg, int index) {
    const size_t D = (size_t)cfg->embed_dim, H = (size_t)VIT_HIDDEN_DIM(cfg), H1 = (size_t)VIT_FC1_ROWS(cfg);
    const size_t P = (size_t)vit_config_patches(cfg), R = (size_t)VIT_REGISTER_TOKENS(cfg);
    const size_t PK = (size_t)cfg->in_chans * VIT_PATCH_SIZE(cfg) * VIT_PATCH_SIZE(cfg);
    const int base = 4 + VIT_WEIGHTS_PER_LAYER * cfg->depth;
    if (index < 0 || index >= base + 4) return 0;
    if (index < 4) {
        const size_t s[4] = {(1 + R) * D, D * PK, D, (P + 1) * D}; /* the prefix rows; registers take no position embedding */
        return s[index];
    }
    if (index >= base) {
        const size_t s[4] = {D, D, (size_t)cfg->num_classes * D, (size_t)cfg->num_classes};
        return s[index - base];
    }
    {
        /* ln1 w,b | in_proj w,b | out_proj w,b | ln2 w,b | fc1 w,b | fc2 w,b  (ViT_seq.c:366-426); SwiGLU: fc1 = w12, 2H rows */
        const size_t s[12] = {D, D, 3 * D * D, 3 * D, D * D, D, D, D, H1 * D, H1, D * H, D};
        return s[(index - 4) % VIT_WEIGHTS_PER_LAYER];
    }
}

unsigned long long vit_config_macs_per_image(const vit_config *cfg) {
    const unsigned long long T = (unsigned long long)vit_config_tokens(cfg), D = cfg->embed_dim,
                             H = VIT_HIDDEN_DIM(cfg), H1 = (unsigned long long)VIT_FC1_ROWS(cfg), hd = D / cfg->num_heads,
                             PK = (unsigned long long)cfg->in_chans * VIT_PATCH_SIZE(cfg) * VIT_PATCH_SIZE(cfg);
    const unsigned long long layer = T * D * 3 * D + 2 * cfg->num_heads * T * T * hd + T * D * D + T * D * H1 + T * H * D;
    return (unsigned long long)vit_config_patches(cfg) * PK * D + cfg->depth * layer + D * cfg->num_classes;
}

unsigned long long vit_config_macs_per_image_pruned(const vit_config *cfg) {
    const unsigned long long T = (unsigned long long)vit_config_tokens(cfg), D = cfg->embed_dim, H = VIT_HIDDEN_DIM(cfg),
                             H1 = (unsigned long long)VIT_FC1_ROWS(cfg), hd = D / cfg->num_heads;
    /* last layer: Q projection, both attention products, out_proj, fc1, fc2 for one row instead of T */
    const unsigned long long saved = (T - 1) * (D * D + 2 * cfg->num_heads * T * hd + D * D + D * H1 + H * D);
    return vit_config_macs_per_image(cfg) - saved;
}

void vit_engine_default_options(vit_engine_options *opt) {
    opt->device = 0;
    opt->max_batch = 256;
    opt->profile = 0;
    opt->lanes = 1;
    opt->dtype = VIT_DTYPE_F32;
    opt->prune_last_layer = 0;
    opt->use_graph = 0;
    opt->gemm_tile = 0;
    opt->ln_fold = 0;
    opt->gemm_handover_test = 0;
    opt->host_first_piece = 0;
    opt->fp32_split = 0;
}

static int fail(vit_engine *e, int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(e->err, sizeof(e->err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(e, call)                                                                     \
    do {                                                                                     \
        int rc_ = (call);                                                                    \
        if (rc_ != 0)                                                                        \
            return fail((e), VIT_ERR_HIP, "[%s:%d] HIP error %d (%s) in %s", __FILE__, __LINE__, \
                        rc_, vithip_error_string(rc_), #call);                               \
    } while (0)

const char *vit_engine_last_error(const vit_engine *e) { return e ? e->err : "null engine"; }
const vit_config *vit_engine_config(const vit_engine *e) { return &e->cfg; }

#define WEIGHT_TAIL_PAD (1u << 20) /* GEMM loaders read (never use) up to a tile of rows past the last tensor */

static int check_config(vit_engine *e) {
    const vit_config *c = &e->cfg;
    if (c->img_size <= 0 || c->patch_size <= 0 || VIT_PATCH_SIZE(c) == 0 || c->in_chans <= 0 || c->num_classes <= 0 ||
        c->embed_dim <= 0 || c->depth <= 0 || c->num_heads <= 0 || c->hidden_dim <= 0 || VIT_HIDDEN_DIM(c) == 0)
        return fail(e, VIT_ERR_ARG, "vit_config: all dimensions must be positive");
    if (VIT_MLP_KIND(c) != VIT_MLP_GELU && VIT_MLP_KIND(c) != VIT_MLP_SWIGLU && VIT_MLP_KIND(c) != VIT_MLP_QUICKGELU)
        return fail(e, VIT_ERR_ARG, "vit_config.hidden_dim: MLP kind %d (VIT_MLP_KIND, bits 24..30): VIT_MLP_GELU (%d), VIT_MLP_SWIGLU (%d) or VIT_MLP_QUICKGELU (%d)",
                    VIT_MLP_KIND(c), VIT_MLP_GELU, VIT_MLP_SWIGLU, VIT_MLP_QUICKGELU);
    if (VIT_REGISTER_TOKENS(c) > VIT_MAX_REGISTER_TOKENS)
        return fail(e, VIT_ERR_ARG, "vit_config.patch_size: %d register tokens (VIT_REGISTER_TOKENS, bits 24..30): 0..%d", VIT_REGISTER_TOKENS(c),
                    VIT_MAX_REGISTER_TOKENS);
    if (c->img_size % VIT_PATCH_SIZE(c)) return fail(e, VIT_ERR_ARG, "img_size must be a multiple of patch_size");
    if (c->embed_dim % c->num_heads || vithip_qscale(c->embed_dim / c->num_heads) == 0.0f) /* what the attention kernels take */
        return fail(e, VIT_ERR_ARG, "HIP attention kernels need head_dim 64 or a multiple of 8 from 72 to 128 (got %d/%d)", c->embed_dim,
                    c->num_heads);
    if (c->embed_dim % 32 || VIT_HIDDEN_DIM(c) % 32)
        return fail(e, VIT_ERR_ARG, "embed_dim and hidden_dim must be multiples of 32");
    /* what vithip_patch_embed_f32 takes: the 16-byte gather or, for every other even geometry (patch 14), the general kernel */
    if (VIT_PATCH_SIZE(c) % 2 || c->img_size % 2)
        return fail(e, VIT_ERR_ARG, "patch geometry unsupported: patch_size %d and img_size %d must both be even", VIT_PATCH_SIZE(c),
                    c->img_size);
    if (c->embed_dim > 2048) return fail(e, VIT_ERR_ARG, "embed_dim > 2048 unsupported by the LayerNorm kernel");
    return VIT_OK;
}

/* One hand-over workspace per lane in use (fp32 engines; 32 MB of uncached device memory each on a 256-CU device). */
static int ensure_gemm_workspaces(vit_engine *e) {
    if (e->opt.dtype != VIT_DTYPE_F32) return VIT_OK;
    for (int j = 0; j < e->opt.lanes && j < VIT_MAX_LANES; ++j)
        if (!e->gemm_ws[j]) HIP_TRY(e, vithip_gemm_f32_workspace_create(&e->gemm_ws[j]));
    return VIT_OK;
}

int vit_engine_create(vit_engine **out, const vit_config *cfg, const vit_engine_options *opt) {
    static vit_engine scratch;  /* error text holder when allocation itself fails */
    if (!out) return VIT_ERR_ARG;
    *out = NULL;
    vit_engine *e = (vit_engine *)calloc(1, sizeof(*e));
    if (!e) return fail(&scratch, VIT_ERR_NOMEM, "out of host memory");
    *out = e; /* returned even on failure so the caller can read the message, then destroy */
    e->cfg = cfg ? *cfg : vit_config_b16();
    if (opt) e->opt = *opt; else vit_engine_default_options(&e->opt);
    e->ln_eps = VITHIP_LN_EPS;
    if (e->opt.max_batch <= 0) e->opt.max_batch = 256;
    if (e->opt.lanes < 1) e->opt.lanes = 1;
    int rc = check_config(e);
    if (rc) return rc;
    e->tokens = vit_config_tokens(&e->cfg);
    e->patches = vit_config_patches(&e->cfg);
    e->prefix = e->tokens - e->patches;
    e->n_weights = VIT_WEIGHT_COUNT(e->cfg.depth);
    {
        /* The fp32 GEMMs (and the patch gather) address an A operand through a buffer descriptor with 32-bit byte
         * offsets (csrc/vit_gemm.hip): one launch may span < 2 GiB of images, LN output, attention output or MLP hidden
         * rows.  That bounds the images of one LANE; larger chunks are cut down in forward_device/forward_host. */
        const size_t T_ = (size_t)e->tokens, per[3] = {T_ * (size_t)VIT_FC1_ROWS(&e->cfg), T_ * (size_t)e->cfg.embed_dim,
                                                         (size_t)e->cfg.in_chans * e->cfg.img_size * e->cfg.img_size};
        size_t worst = per[0] > per[1] ? per[0] : per[1];
        if (per[2] > worst) worst = per[2];
        const size_t cap = ((size_t)0x7fffffff - 4096) / (worst * sizeof(float));
        if (cap < 1) return fail(e, VIT_ERR_ARG, "model too large: one image needs %zu bytes of fp32 rows, the fp32 kernels "
                                                 "address < 2 GiB per launch", worst * sizeof(float));
        e->lane_cap = cap > (size_t)INT_MAX ? INT_MAX : (int)cap;
    }

    int ndev = 0;
    HIP_TRY(e, vithip_device_count(&ndev));
    if (e->opt.device < 0 || e->opt.device >= ndev)
        return fail(e, VIT_ERR_ARG, "device %d not available (%d HIP devices)", e->opt.device, ndev);
    HIP_TRY(e, vithip_set_device(e->opt.device));
    {
        vithip_device_info di;
        HIP_TRY(e, vithip_get_device_info(e->opt.device, &di));
        e->n_cus = di.compute_units;
    }
    HIP_TRY(e, vithip_stream_create(&e->stream));
    for (int j = 0; j < VIT_MAX_LANES - 1; ++j) {
        HIP_TRY(e, vithip_stream_create(&e->aux_stream[j]));
        HIP_TRY(e, vithip_event_create(&e->ev_join[j]));
    }
    HIP_TRY(e, vithip_event_create(&e->ev_fork));

    const size_t B = (size_t)e->opt.max_batch, T = (size_t)e->tokens, D = (size_t)e->cfg.embed_dim,
                 H = (size_t)VIT_HIDDEN_DIM(&e->cfg), H1 = (size_t)VIT_FC1_ROWS(&e->cfg), NC = (size_t)e->cfg.num_classes;
    const size_t img = (size_t)e->cfg.in_chans * e->cfg.img_size * e->cfg.img_size;
    HIP_TRY(e, vithip_malloc((void **)&e->x, B * T * D * sizeof(float)));
    HIP_TRY(e, vithip_malloc((void **)&e->y, B * T * D * sizeof(float)));
    HIP_TRY(e, vithip_malloc((void **)&e->qkv, B * T * 3 * D * sizeof(float)));
    /* the MLP's rows: the hidden layer or, under SwiGLU, fc1's [gate | value] rows, whose gate half becomes the hidden layer in
     * place (encoder_layer) */
    HIP_TRY(e, vithip_malloc((void **)&e->hbuf, B * T * H1 * sizeof(float)));
    HIP_TRY(e, vithip_malloc((void **)&e->z, B * D * sizeof(float)));
    HIP_TRY(e, vithip_malloc((void **)&e->logits, B * NC * sizeof(float)));
    if (e->opt.lanes > VIT_MAX_LANES) e->opt.lanes = VIT_MAX_LANES;
    {
        int rc_ws = ensure_gemm_workspaces(e);
        if (rc_ws) return rc_ws;
    }
    const int bf16 = e->opt.dtype == VIT_DTYPE_BF16, f32 = e->opt.dtype == VIT_DTYPE_F32;
    /* the split runs at every K of the model (K % 32 == 0 is checked for every fp32 GEMM anyway) and every M: whether it is on
     * depends on the options alone, never on the batch */
    e->split = f32 && e->opt.fp32_split >= 0;
    if ((bf16 || f32) && e->opt.ln_fold >= 0) {
        /* bf16: the fold lives in the ping-pong GEMM (two K steps at least); its scratch (bf16 copy of x, row sums) uses the idle
         * halves of the y and qkv allocations, which bf16 activations only half fill.  fp32: the consumer epilogue exists in every
         * fp32 GEMM kernel; the row statistics kernel wants whole 64-column strips */
        const int ok = bf16 ? D >= 128 && H >= 128 && D % 64 == 0 && H % 64 == 0 : D % 64 == 0 && D <= 2048;
        if (!ok && e->opt.ln_fold > 0)
            return fail(e, VIT_ERR_ARG, bf16 ? "ln_fold needs embed_dim and hidden_dim >= 128 and multiples of 64"
                                             : "ln_fold (fp32) needs embed_dim to be a multiple of 64, at most 2048");
        e->fold = ok;
        if (e->fold) {
            const size_t wbytes = (size_t)e->cfg.depth * fold_w_elems(&e->cfg) * (bf16 ? sizeof(unsigned short) : sizeof(float));
            HIP_TRY(e, vithip_malloc(&e->wfold, wbytes + WEIGHT_TAIL_PAD));
            HIP_TRY(e, vithip_memset((char *)e->wfold + wbytes, 0, WEIGHT_TAIL_PAD, e->stream));
            HIP_TRY(e, vithip_malloc((void **)&e->wfoldf, (size_t)e->cfg.depth * fold_f_elems(&e->cfg) * sizeof(float)));
            if (f32) {
                HIP_TRY(e, vithip_malloc((void **)&e->ln_rows32, (B * T + B) * 2 * sizeof(float)));
                HIP_TRY(e, vithip_malloc((void **)&e->ln_part32, (D / 64) * B * T * 2 * sizeof(float)));
            }
        }
    }
    if (e->split) {
        /* W's pieces, made once per upload (resolve_operands): the persistent split walk then splits only A.  6 bytes per weight of
         * the four encoder GEMMs; without the image (K not a multiple of 32) every GEMM splits W on the fly, with the same bits */
        const size_t b[4] = {vithip_split3_weights_bytes((int)(3 * D), (int)D), vithip_split3_weights_bytes((int)D, (int)D),
                             vithip_split3_weights_bytes((int)H1, (int)D), vithip_split3_weights_bytes((int)D, (int)H)};
        if (b[0] && b[1] && b[2] && b[3]) {
            e->wsplit_layer = 0;
            for (int i = 0; i < 4; ++i) { e->wsplit_off[i] = e->wsplit_layer; e->wsplit_layer += b[i]; }
            HIP_TRY(e, vithip_malloc((void **)&e->wsplit, (size_t)e->cfg.depth * e->wsplit_layer));
        }
    }
    HIP_TRY(e, vithip_stream_create(&e->copy_stream));
    e->out_row_cap = NC * sizeof(float);
    for (int b = 0; b < 2; ++b) {
        HIP_TRY(e, vithip_malloc((void **)&e->in_stage[b], B * img * sizeof(float)));
        HIP_TRY(e, vithip_malloc((void **)&e->out_stage[b], B * NC * sizeof(float)));
        HIP_TRY(e, vithip_host_alloc((void **)&e->pin_in[b], B * img * sizeof(float)));
        HIP_TRY(e, vithip_host_alloc((void **)&e->pin_out[b], B * NC * sizeof(float)));
        HIP_TRY(e, vithip_event_create(&e->ev_h2d[b]));
        HIP_TRY(e, vithip_event_create(&e->ev_done[b]));
    }

    e->w = (float **)calloc((size_t)e->n_weights, sizeof(float *));
    e->w16 = (unsigned short **)calloc((size_t)e->n_weights, sizeof(unsigned short *));
    e->layer = (vit_layer_ops *)calloc((size_t)e->cfg.depth, sizeof(vit_layer_ops));
    e->img_recs = (vithip_image_u8 *)calloc(B, sizeof(vithip_image_u8));
    e->img_off = (size_t *)calloc(B + 1, sizeof(size_t));
    if (!e->w || !e->w16 || !e->layer || !e->img_recs || !e->img_off) return fail(e, VIT_ERR_NOMEM, "out of host memory");
    if (e->opt.dtype != VIT_DTYPE_F32 && e->opt.dtype != VIT_DTYPE_BF16)
        return fail(e, VIT_ERR_ARG, "dtype must be VIT_DTYPE_F32 or VIT_DTYPE_BF16");
    if (e->opt.dtype == VIT_DTYPE_BF16 && (e->cfg.embed_dim % 64 || VIT_HIDDEN_DIM(&e->cfg) % 64))
        return fail(e, VIT_ERR_ARG, "bf16 path needs embed_dim and hidden_dim to be multiples of 64");
    if (e->opt.profile) return vit_engine_set_profile(e, 1);
    return VIT_OK;
}

/* a caller's head owns its weight, bias and operand rows; the checkpoint's own points into wblob and z */
static void release_head(vit_head *h) {
    if (!h->owned) return;
    vithip_free((void *)h->ops.W); vithip_free((void *)h->ops.bias); vithip_free(h->operand);
}

/* the dense head's allocations go with it; nothing may be in flight */
static void release_dense_head(vit_dense_head *h) {
    vithip_free(h->W); vithip_free(h->bias); vithip_free(h->zero_bias); vithip_free(h->rows); vithip_free(h->logits);
    memset(h, 0, sizeof(*h));
}

void vit_engine_destroy(vit_engine *e) {
    if (!e) return;
    vithip_set_device(e->opt.device);
    if (e->stream) vithip_stream_sync(e->stream);
    if (e->ev_ready)
        for (int i = 0; i < 2 * MAX_EVENTS; ++i) vithip_event_destroy(e->ev[i]);
    if (e->graph) vithip_graph_destroy(e->graph);
    vithip_free(e->x); vithip_free(e->y); vithip_free(e->qkv); vithip_free(e->hbuf);
    vithip_free(e->z); vithip_free(e->logits);
    release_head(&e->head);
    release_dense_head(&e->dense);
    vithip_free(e->pre_g); /* one allocation: gamma, beta behind it */
    for (int j = 0; j < VIT_MAX_LANES; ++j) vithip_gemm_f32_workspace_destroy(e->gemm_ws[j]);
    if (e->copy_stream) { vithip_stream_sync(e->copy_stream); vithip_stream_destroy(e->copy_stream); }
    if (e->ev_in_stage) vithip_event_destroy(e->ev_in_stage);
    for (int b = 0; b < 2; ++b) {
        vithip_free(e->in_stage[b]); vithip_free(e->out_stage[b]); vithip_free(e->in8_stage[b]); vithip_free(e->img_stage[b]);
        if (e->pin_in[b]) vithip_host_free(e->pin_in[b]);
        if (e->pin_out[b]) vithip_host_free(e->pin_out[b]);
        if (e->ev_h2d[b]) vithip_event_destroy(e->ev_h2d[b]);
        if (e->ev_done[b]) vithip_event_destroy(e->ev_done[b]);
    }
    vithip_free(e->wblob);
    vithip_free(e->wfold);
    vithip_free(e->wsplit);
    vithip_free(e->ln_rows32);
    vithip_free(e->ln_part32);
    vithip_free(e->wfoldf);
    free(e->w16); free(e->layer);
    free(e->img_recs); free(e->img_off); free(e->piece_lo);
    for (int j = 0; j < VIT_MAX_LANES - 1; ++j) {
        if (e->aux_stream[j]) { vithip_stream_sync(e->aux_stream[j]); vithip_stream_destroy(e->aux_stream[j]); }
        if (e->ev_join[j]) vithip_event_destroy(e->ev_join[j]);
    }
    if (e->ev_fork) vithip_event_destroy(e->ev_fork);
    if (e->stream) vithip_stream_destroy(e->stream);
    free(e->w);
    free(e);
}

int vit_engine_set_lanes(vit_engine *e, int lanes) {
    if (!e) return VIT_ERR_ARG;
    if (lanes < 1 || lanes > VIT_MAX_LANES) return fail(e, VIT_ERR_ARG, "lanes must be 1..%d", VIT_MAX_LANES);
    e->opt.lanes = lanes;
    HIP_TRY(e, vithip_set_device(e->opt.device));
    return ensure_gemm_workspaces(e);
}

int vit_engine_set_resize_filter(vit_engine *e, int filter) {
    if (!e) return VIT_ERR_ARG;
    if (filter != VIT_RESIZE_BILINEAR && filter != VIT_RESIZE_BICUBIC)
        return fail(e, VIT_ERR_ARG, "resize filter %d: VIT_RESIZE_BILINEAR (%d) or VIT_RESIZE_BICUBIC (%d)", filter, VIT_RESIZE_BILINEAR,
                    VIT_RESIZE_BICUBIC);
    e->resize_filter = filter;
    return VIT_OK;
}

int vit_engine_get_resize_filter(const vit_engine *e) { return e ? e->resize_filter : -1; }

static void drop_graph(vit_engine *e);

int vit_engine_set_layernorm_eps(vit_engine *e, double eps) {
    if (!e) return VIT_ERR_ARG;
    if (!(eps > 0.0) || !isfinite(eps)) return fail(e, VIT_ERR_ARG, "set_layernorm_eps: eps = %g must be finite and > 0", eps);
    HIP_TRY(e, vithip_set_device(e->opt.device));
    HIP_TRY(e, vithip_device_sync()); /* a captured forward holds the old value in its launches */
    drop_graph(e);
    e->ln_eps = eps;
    return VIT_OK;
}

double vit_engine_get_layernorm_eps(const vit_engine *e) { return e ? e->ln_eps : 0.0; }

/* Nothing may be in flight (the callers have synchronised). */
static void release_pre_norm(vit_engine *e) {
    vithip_free(e->pre_g);
    e->pre_g = e->pre_b = NULL;
}

int vit_engine_set_pre_norm(vit_engine *e, const float *gamma, const float *beta) {
    if (!e) return VIT_ERR_ARG;
    if (!gamma != !beta) return fail(e, VIT_ERR_ARG, "set_pre_norm: gamma and beta come together (both NULL removes the pre-norm)");
    if (!e->weights_loaded) return fail(e, VIT_ERR_STATE, "set_pre_norm before vit_engine_load_weights()");
    HIP_TRY(e, vithip_set_device(e->opt.device));
    if (!gamma) { /* as an install: nothing in flight, no graph with the old launch list */
        HIP_TRY(e, vithip_device_sync());
        drop_graph(e);
        release_pre_norm(e);
        return VIT_OK;
    }
    /* the new pair first, whole; only then the old one goes */
    const size_t D = (size_t)e->cfg.embed_dim;
    float *g = NULL;
    int hrc = vithip_malloc((void **)&g, 2 * D * sizeof(float));
    if (hrc)
        return fail(e, VIT_ERR_NOMEM, "set_pre_norm: no memory for 2 x %zu floats (HIP error %d: %s); the previous pre-norm stays", D, hrc,
                    vithip_error_string(hrc));
    hrc = vithip_memcpy_h2d(g, gamma, D * sizeof(float), e->stream);
    if (!hrc) hrc = vithip_memcpy_h2d(g + D, beta, D * sizeof(float), e->stream);
    if (!hrc) hrc = vithip_device_sync(); /* the uploads, and every forward that still reads the old pair, on whatever stream */
    if (hrc) {
        vithip_free(g);
        return fail(e, VIT_ERR_HIP, "set_pre_norm: HIP error %d (%s) uploading; the previous pre-norm stays", hrc, vithip_error_string(hrc));
    }
    drop_graph(e);
    release_pre_norm(e);
    e->pre_g = g; e->pre_b = g + D; /* D % 32 == 0: beta is 16-byte aligned too */
    return VIT_OK;
}

int vit_engine_set_profile(vit_engine *e, int on) {
    if (on && !e->ev_ready) {
        for (int i = 0; i < 2 * MAX_EVENTS; ++i) HIP_TRY(e, vithip_event_create(&e->ev[i]));
        e->ev_ready = 1;
    }
    e->opt.profile = on ? 1 : 0;
    return VIT_OK;
}

/* ------------------------------------------------------------------------------------------ */

/* A captured forward holds the old weight addresses in its kernel arguments: drop it with them. */
static void drop_graph(vit_engine *e) {
    if (e->graph) { vithip_graph_destroy(e->graph); e->graph = NULL; }
    e->g_n = 0; e->g_images = NULL;
    memset(&e->g_in, 0, sizeof(e->g_in));
    memset(&e->g_out, 0, sizeof(e->g_out));
}

/* (Re)allocate the device blob for this model and point w[] / w16[] into it (no data yet). */
static int alloc_weight_blob(vit_engine *e, const size_t *off, size_t f32_floats, size_t gemm_floats) {
    const int bf16 = e->opt.dtype == VIT_DTYPE_BF16;
    const size_t bytes = f32_floats * sizeof(float) + (bf16 ? gemm_floats * sizeof(unsigned short) : 0);
    HIP_TRY(e, vithip_set_device(e->opt.device));
    if (e->stream) HIP_TRY(e, vithip_stream_sync(e->stream));
    drop_graph(e);
    e->weights_loaded = 0;
    if (e->wblob && e->wblob_bytes != bytes) { vithip_free(e->wblob); e->wblob = NULL; }
    if (!e->wblob) {
        HIP_TRY(e, vithip_malloc((void **)&e->wblob, bytes + WEIGHT_TAIL_PAD));
        HIP_TRY(e, vithip_memset((char *)e->wblob + bytes, 0, WEIGHT_TAIL_PAD, e->stream));
    }
    e->wblob_bytes = bytes;
    e->wblob16 = bf16 ? (unsigned short *)(e->wblob + f32_floats) : NULL;
    for (int i = 0; i < e->n_weights; ++i) {
        e->w[i] = e->wblob + off[i];
        e->w16[i] = (bf16 && off[i] < gemm_floats) ? e->wblob16 + off[i] : NULL;
    }
    return VIT_OK;
}

/* Every GEMM's and LayerNorm's operands as the stages read them: the only place that knows where a tensor lies.  bf16 engines read
 * the encoder GEMM weights (and the conv weight) from w16[].  The derived operands are made here, where they enter the table:
 *   fold   2 launches per layer, from the resident fp32 tensors: Wf = gamma * W (bf16 engines: rounded to bf16), its column sums
 *          and the beta-folded biases of in_proj (LN1) and fc1 (LN2), which then stand in for the raw operands;
 *   split  fp32 engines: W's pieces, 4 launches per layer.
 * The table points into wblob, which alloc_weight_blob may move: it is rebuilt by every install, never patched. */
static int resolve_operands(vit_engine *e) {
    const int bf16 = e->opt.dtype == VIT_DTYPE_BF16, D = e->cfg.embed_dim, H = VIT_HIDDEN_DIM(&e->cfg), H1 = VIT_FC1_ROWS(&e->cfg);
    const size_t esz = bf16 ? sizeof(unsigned short) : sizeof(float);
    float **tail = e->w + W_LAYER0 + VIT_WEIGHTS_PER_LAYER * e->cfg.depth;
    e->embed = (vit_embed_ops){e->w[W_CLS], e->w[W_CONV_W], e->w[W_CONV_B], e->w[W_POS], e->w16[W_CONV_W]};
    e->final = (vit_final_ops){tail[0], tail[1], {.W = tail[2], .bias = tail[3]}};
    for (int l = 0; l < e->cfg.depth; ++l) {
        float **lw = e->w + W_LAYER0 + VIT_WEIGHTS_PER_LAYER * l;
        unsigned short **lw16 = e->w16 + W_LAYER0 + VIT_WEIGHTS_PER_LAYER * l;
#define GEMM_OPS(k) {bf16 ? (const void *)lw16[k] : (const void *)lw[k], lw[(k) + 1], NULL, NULL} /* a weight, its bias behind it */
        vit_layer_ops o = {lw[LW_LN1_G], lw[LW_LN1_B], lw[LW_LN2_G], lw[LW_LN2_B],
                           GEMM_OPS(LW_QKV_W), GEMM_OPS(LW_OUT_W), GEMM_OPS(LW_FC1_W), GEMM_OPS(LW_FC2_W)};
#undef GEMM_OPS
        if (e->fold) {
            void *w_qkv = at(e->wfold, (size_t)l * fold_w_elems(&e->cfg), esz), *w_fc1 = at(w_qkv, 3 * (size_t)D * D, esz);
            float *cs_qkv = e->wfoldf + (size_t)l * fold_f_elems(&e->cfg), *b_qkv = cs_qkv + 3 * D, *cs_fc1 = b_qkv + 3 * D, *b_fc1 = cs_fc1 + H1;
            if (bf16) { /* in_proj: the Q rows also carry the factor of the scores' exponent (the attention kernels are told: _qscaled) */
                HIP_TRY(e, vithip_ln_fold_weights_scaled(e->stream, lw[LW_QKV_W], lw[LW_QKV_B], o.ln1_g, o.ln1_b, w_qkv, cs_qkv, b_qkv, 3 * D, D, D, vithip_qscale(D / e->cfg.num_heads)));
                HIP_TRY(e, vithip_ln_fold_weights(e->stream, lw[LW_FC1_W], lw[LW_FC1_B], o.ln2_g, o.ln2_b, w_fc1, cs_fc1, b_fc1, H1, D));
            } else { /* fp32 products, sums in double, rounded once; centred weights (vit_hip_kernels.h): the GEMMs deliver
                      * x . (gamma W)^T - mean * colsum themselves and their epilogues only scale, so no column sums are passed on:
                      * their slots receive what the weights' rounding left of the sums and are not read again */
                HIP_TRY(e, vithip_ln_fold_weights_f32_centered(e->stream, lw[LW_QKV_W], lw[LW_QKV_B], o.ln1_g, o.ln1_b, w_qkv, cs_qkv, b_qkv, 3 * D, D));
                HIP_TRY(e, vithip_ln_fold_weights_f32_centered(e->stream, lw[LW_FC1_W], lw[LW_FC1_B], o.ln2_g, o.ln2_b, w_fc1, cs_fc1, b_fc1, H1, D));
                cs_qkv = cs_fc1 = NULL;
            }
            o.qkv.W = w_qkv; o.qkv.bias = b_qkv; o.qkv.colsum = cs_qkv;
            o.fc1.W = w_fc1; o.fc1.bias = b_fc1; o.fc1.colsum = cs_fc1;
        }
        if (e->wsplit) { /* 4 launches: the image of every encoder GEMM weight as its GEMM reads it, folded (centred) or raw */
            vit_gemm_ops *g[4] = {&o.qkv, &o.out, &o.fc1, &o.fc2}; /* the order of wsplit_off[] */
            const int N[4] = {3 * D, D, H1, D}, K[4] = {D, D, D, H};
            for (int i = 0; i < 4; ++i) {
                void *img = e->wsplit + (size_t)l * e->wsplit_layer + e->wsplit_off[i];
                HIP_TRY(e, vithip_split3_weights_f32(e->stream, g[i]->W, K[i], N[i], K[i], img));
                g[i]->w_split = img;
            }
        }
        e->layer[l] = o;
    }
    return VIT_OK;
}

/* Back to the checkpoint's own head: a caller's head (vit_engine_set_head) and its allocations go.  Nothing may be in flight.  The
 * own head is an instance like any other: the class block of the last layer alone, final.head (as installed: wblob may move) over z. */
static void restore_own_head(vit_engine *e) {
    if (e->head.owned) e->last_rows = 0;
    release_head(&e->head);
    e->head = (vit_head){.spec = {.num_cls_layers = 1, .cls_layers = {e->cfg.depth - 1}, .pool = VIT_HEAD_POOL_NONE},
                         .in = (size_t)e->cfg.embed_dim, .ops = e->final.head, .operand = e->z, .owned = 0};
}

/* The tail of every install, behind the last write to wblob: the fold, the split images and the operand table, then the sync.
 * Every install also puts the checkpoint's own head back in force (alloc_weight_blob has synchronised and dropped the graph),
 * whatever became of the derived operands' launches: final.head is set before the first of them. */
static int finish_install(vit_engine *e) {
    const int rc = resolve_operands(e);
    restore_own_head(e);
    release_dense_head(&e->dense); /* a caller's head like the classifier's: every install removes it */
    release_pre_norm(e); /* checkpoint data like a caller's head: every install removes it (the epsilon, architecture, stays) */
    if (rc) return rc;
    HIP_TRY(e, vithip_stream_sync(e->stream));
    e->weights_loaded = 1;
    return VIT_OK;
}

static int pos_mode_ok(int mode) { return mode == VIT_POS_BICUBIC || mode == VIT_POS_BICUBIC_AA; }
/* patches per side the resampling kernel takes (vithip_pos_resample_f32) */
static int pos_grid_ok(int g) { return g >= 1 && g <= 256; }

/* Upload an image; with d_pos_src (device, [1 + g_src^2][D], the checkpoint's position embedding) the resident position embedding
 * is resampled from it to the engine's own grid, in front of finish_install. */
static int load_image(vit_engine *e, const vit_weight_image *img, const float *d_pos_src, int g_src, int mode) {
    if (!e || !img || !img->f32) return e ? fail(e, VIT_ERR_ARG, "null weight image") : VIT_ERR_ARG;
    if (memcmp(&img->cfg, &e->cfg, sizeof(vit_config)) != 0 || img->count != e->n_weights)
        return fail(e, VIT_ERR_WEIGHTS, "weight image was built for another model configuration");
    int rc = alloc_weight_blob(e, img->off, img->f32_floats, img->gemm_floats);
    if (rc) return rc;
    const int bf16 = e->opt.dtype == VIT_DTYPE_BF16;
    /* ONE host-to-device copy: the image is the device layout ([fp32 | bf16] adjacent on both sides) */
    const size_t up = img->f32_floats * sizeof(float) + ((bf16 && img->bf16_elems) ? img->bf16_elems * sizeof(unsigned short) : 0);
    HIP_TRY(e, vithip_memcpy_h2d(e->wblob, img->f32, up, e->stream));
    if (bf16 && !img->bf16_elems) /* image without a bf16 section: convert the GEMM-operand region on the device, one launch */
        HIP_TRY(e, vithip_f32_to_bf16(e->stream, e->wblob, e->wblob16, img->gemm_floats));
    if (d_pos_src) /* fp32 only: the position embedding is no GEMM operand and has no bf16 copy */
        HIP_TRY(e, vithip_pos_resample_f32(e->stream, d_pos_src, g_src, e->w[W_POS], e->cfg.img_size / VIT_PATCH_SIZE(&e->cfg), e->cfg.embed_dim, mode));
    return finish_install(e);
}

int vit_engine_load_weight_image(vit_engine *e, const vit_weight_image *img) { return load_image(e, img, NULL, 0, 0); }

/* A caller's Network[] against the model: the count, then every tensor present and of its size; the position embedding holds
 * pos_floats (the checkpoint's grid, which need not be the engine's), pos_note says which grid that is (may be NULL). */
static int check_network(vit_engine *e, const Network *weights, int count, size_t pos_floats, const char *pos_note) {
    if (count != e->n_weights)
        return fail(e, VIT_ERR_WEIGHTS, "expected %d weight tensors for depth %d, got %d", e->n_weights, e->cfg.depth, count);
    for (int i = 0; i < count; ++i) {
        const size_t want = i == W_POS ? pos_floats : vit_config_weight_size(&e->cfg, i);
        if (!weights[i].data)
            return fail(e, VIT_ERR_WEIGHTS, "weight %d is missing (Network[%d].data == NULL; expected %zu floats)", i, i, want);
        if (weights[i].size != want && i == W_POS && pos_note)
            return fail(e, VIT_ERR_WEIGHTS, "weight 3 (position embedding) has %zu floats, expected %zu %s", weights[i].size, want, pos_note);
        if (weights[i].size != want)
            return fail(e, VIT_ERR_WEIGHTS, "weight %d has %zu floats, expected %zu", i, weights[i].size, want);
    }
    return VIT_OK;
}

/* The separately malloc'd tensors of the reference's Network[] (Network.c:147-191), checked, are packed into the device layout on
 * the host (8 threads), then uploaded with one copy (load_image); bf16 operands are converted on the device */
static int load_network(vit_engine *e, const Network *weights, int count, const float *d_pos_src, int g_src, int mode) {
    vit_weight_image img;
    if (vit_weight_image_build(&img, &e->cfg, weights, count, 0) != 0) return fail(e, VIT_ERR_NOMEM, "out of host memory packing the weights");
    const int rc = load_image(e, &img, d_pos_src, g_src, mode);
    vit_weight_image_free(&img);
    return rc;
}

int vit_engine_load_weights(vit_engine *e, const Network *weights, int count) {
    if (!e || !weights) return e ? fail(e, VIT_ERR_ARG, "null weights") : VIT_ERR_ARG;
    const int rc = check_network(e, weights, count, vit_config_weight_size(&e->cfg, W_POS), NULL);
    return rc ? rc : load_network(e, weights, count, NULL, 0, 0);
}

int vit_engine_load_weights_resampled(vit_engine *e, const Network *weights, int count, const vit_pos_resample *rs) {
    if (!e || !weights) return e ? fail(e, VIT_ERR_ARG, "null weights") : VIT_ERR_ARG;
    if (!rs) return fail(e, VIT_ERR_ARG, "load_weights_resampled: null vit_pos_resample");
    if (rs->reserved != 0) return fail(e, VIT_ERR_ARG, "load_weights_resampled: reserved must be 0 (got %d)", rs->reserved);
    if (!pos_mode_ok(rs->mode)) return fail(e, VIT_ERR_ARG, "load_weights_resampled: unknown mode %d", rs->mode);
    const int patch = VIT_PATCH_SIZE(&e->cfg);
    if (rs->src_img_size <= 0 || rs->src_img_size % patch)
        return fail(e, VIT_ERR_ARG, "load_weights_resampled: src_img_size %d is not a positive multiple of patch_size %d", rs->src_img_size,
                    patch);
    const int g_src = rs->src_img_size / patch, g_dst = e->cfg.img_size / patch;
    if (!pos_grid_ok(g_src) || !pos_grid_ok(g_dst))
        return fail(e, VIT_ERR_ARG, "load_weights_resampled: grids of %d and %d patches per side, the resampling takes 1..256", g_src, g_dst);
    const size_t D = (size_t)e->cfg.embed_dim, pos_src = ((size_t)g_src * g_src + 1) * D, pos_dst = ((size_t)g_dst * g_dst + 1) * D;
    char note[128];
    snprintf(note, sizeof(note), "for the checkpoint's %d x %d grid (the engine's own %d x %d grid holds %zu)", g_src, g_src, g_dst, g_dst, pos_dst);
    int rc = check_network(e, weights, count, pos_src, note);
    if (rc) return rc;
    if (g_src == g_dst) return vit_engine_load_weights(e, weights, count); /* nothing to resample: the plain load, bit for bit */
    /* the image is the engine's own layout; its tensor 3 is a placeholder that the kernel overwrites on the device */
    Network *tmp = (Network *)malloc(sizeof(Network) * (size_t)count);
    float *blank = (float *)calloc(pos_dst, sizeof(float));
    float *d_pos = NULL;
    rc = (tmp && blank) ? VIT_OK : fail(e, VIT_ERR_NOMEM, "out of host memory");
    if (!rc) {
        memcpy(tmp, weights, sizeof(Network) * (size_t)count);
        tmp[W_POS].data = blank; tmp[W_POS].size = pos_dst;
        int hrc = vithip_set_device(e->opt.device);
        if (!hrc) hrc = vithip_malloc((void **)&d_pos, pos_src * sizeof(float));
        if (!hrc) hrc = vithip_memcpy_h2d(d_pos, weights[W_POS].data, pos_src * sizeof(float), e->stream);
        rc = hrc ? fail(e, VIT_ERR_HIP, "load_weights_resampled: HIP error %d (%s) staging the checkpoint's position embedding", hrc,
                        vithip_error_string(hrc))
                 : load_network(e, tmp, count, d_pos, g_src, rs->mode);
        if (e->stream) vithip_stream_sync(e->stream); /* the staging copy reads the caller's array: not behind this call, whatever failed */
        vithip_free(d_pos);
    }
    free(tmp); free(blank);
    return rc;
}

/* dst's weights from src's, device to device: on a multi-GPU node this crosses xGMI once per replica instead of PCIe (the
 * in-process form of "upload to GPU 0 + broadcast").  Equal grids: ONE peer copy of the whole blob.  Otherwise the
 * two layouts differ behind the position embedding only, which is staged on dst's device and resampled into dst's own. */
static int replicate_weights(vit_engine *dst, vit_engine *src, int mode) {
    const int g_src = src->cfg.img_size / VIT_PATCH_SIZE(&src->cfg), g_dst = dst->cfg.img_size / VIT_PATCH_SIZE(&dst->cfg), same = g_src == g_dst;
    if (!same && (!pos_grid_ok(g_src) || !pos_grid_ok(g_dst)))
        return fail(dst, VIT_ERR_ARG, "copy_weights_resampled: grids of %d and %d patches per side, the resampling takes 1..256", g_src, g_dst);
    const size_t n = (size_t)dst->n_weights;
    size_t *off = (size_t *)malloc(sizeof(size_t) * 4 * n);
    if (!off) return fail(dst, VIT_ERR_NOMEM, "out of host memory");
    size_t *size = off + n, *soff = off + 2 * n, *ssize = off + 3 * n;
    size_t gemm_floats = 0, sgemm = 0;
    const size_t f32_floats = vit_weight_layout(&dst->cfg, off, size, &gemm_floats);
    const size_t sf32 = vit_weight_layout(&src->cfg, soff, ssize, &sgemm);
    /* [0, off[W_POS]) | the position embedding's slots | an equally long rest | the bf16 section */
    const size_t head = off[W_POS], spos_floats = ssize[W_POS];
    size_t rest = f32_floats, srest = sf32; /* where the tensor laid out behind the position embedding starts */
    for (size_t i = 0; i < n; ++i) {
        if (off[i] > head && off[i] < rest) rest = off[i];
        if (soff[i] > head && soff[i] < srest) srest = soff[i];
    }
    const int ok = same || (soff[W_POS] == head && sgemm == gemm_floats && gemm_floats <= head && f32_floats - rest == sf32 - srest);
    int rc = ok ? alloc_weight_blob(dst, off, f32_floats, gemm_floats) : fail(dst, VIT_ERR_STATE, "copy_weights_resampled: the weight layouts do not line up");
    free(off);
    if (rc) return rc;
    const int dd = dst->opt.device, sd = src->opt.device;
    if (same) {
        HIP_TRY(dst, vithip_memcpy_peer(dst->wblob, dd, src->wblob, sd, dst->wblob_bytes, dst->stream));
        return finish_install(dst); /* the derived operands are recomputed from the replica's own tensors */
    }
    float *d_pos = NULL; /* src's position embedding on dst's device: the kernel reads local memory whatever the pair of devices */
    HIP_TRY(dst, vithip_malloc((void **)&d_pos, spos_floats * sizeof(float)));
    int hrc = vithip_memcpy_peer(dst->wblob, dd, src->wblob, sd, head * sizeof(float), dst->stream);
    if (!hrc) hrc = vithip_memset(dst->wblob + head, 0, (rest - head) * sizeof(float), dst->stream); /* slot padding stays zero */
    if (!hrc) hrc = vithip_memcpy_peer(dst->wblob + rest, dd, src->wblob + srest, sd, (f32_floats - rest) * sizeof(float), dst->stream);
    if (!hrc && dst->wblob16) hrc = vithip_memcpy_peer(dst->wblob16, dd, src->wblob16, sd, gemm_floats * sizeof(unsigned short), dst->stream);
    if (!hrc) hrc = vithip_memcpy_peer(d_pos, dd, src->w[W_POS], sd, spos_floats * sizeof(float), dst->stream);
    if (!hrc) hrc = vithip_pos_resample_f32(dst->stream, d_pos, g_src, dst->w[W_POS], g_dst, dst->cfg.embed_dim, mode);
    if (dst->stream) vithip_stream_sync(dst->stream);
    vithip_free(d_pos);
    if (hrc) return fail(dst, VIT_ERR_HIP, "copy_weights_resampled: HIP error %d (%s)", hrc, vithip_error_string(hrc));
    return finish_install(dst);
}

int vit_engine_copy_weights(vit_engine *dst, vit_engine *src) {
    if (!dst || !src) return VIT_ERR_ARG;
    if (!src->weights_loaded) return fail(dst, VIT_ERR_STATE, "copy_weights: the source engine has no weights");
    if (memcmp(&dst->cfg, &src->cfg, sizeof(vit_config)) != 0 || dst->opt.dtype != src->opt.dtype)
        return fail(dst, VIT_ERR_ARG, "copy_weights: engines differ in model configuration or dtype");
    return replicate_weights(dst, src, 0);
}

int vit_engine_copy_weights_resampled(vit_engine *dst, vit_engine *src, int mode) {
    if (!dst || !src) return VIT_ERR_ARG;
    if (!pos_mode_ok(mode)) return fail(dst, VIT_ERR_ARG, "copy_weights_resampled: unknown mode %d", mode);
    if (!src->weights_loaded) return fail(dst, VIT_ERR_STATE, "copy_weights: the source engine has no weights");
    vit_config same = src->cfg;
    same.img_size = dst->cfg.img_size;
    if (memcmp(&dst->cfg, &same, sizeof(vit_config)) != 0 || dst->opt.dtype != src->opt.dtype)
        return fail(dst, VIT_ERR_ARG, "copy_weights_resampled: engines differ in more than img_size, or in dtype");
    return replicate_weights(dst, src, mode);
}

int vit_engine_read_weight_image(vit_engine *e, vit_weight_image *img) {
    if (!e || !img) return VIT_ERR_ARG;
    if (!e->weights_loaded) return fail(e, VIT_ERR_STATE, "read_weight_image: no weights loaded");
    /* an empty image of the right shape (built from a zero-filled model would be wasteful: allocate through the loader) */
    Network *tmp = (Network *)calloc((size_t)e->n_weights, sizeof(Network));
    if (!tmp) return fail(e, VIT_ERR_NOMEM, "out of host memory");
    size_t gemm_floats = 0;
    const size_t f32_floats = vit_weight_layout(&e->cfg, NULL, NULL, &gemm_floats);
    float *host = (float *)malloc(e->wblob_bytes);
    int rc = host ? VIT_OK : fail(e, VIT_ERR_NOMEM, "out of host memory");
    if (!rc) {
        rc = vithip_set_device(e->opt.device) || vithip_memcpy_d2h(host, e->wblob, e->wblob_bytes, e->stream) ||
             vithip_stream_sync(e->stream);
        if (rc) rc = fail(e, VIT_ERR_HIP, "read_weight_image: device-to-host copy failed");
    }
    if (!rc) {
        for (int i = 0; i < e->n_weights; ++i) { tmp[i].data = host + (e->w[i] - e->wblob); tmp[i].size = vit_config_weight_size(&e->cfg, i); }
        const int bf16 = e->opt.dtype == VIT_DTYPE_BF16;
        if (vit_weight_image_build(img, &e->cfg, tmp, e->n_weights, bf16) != 0) rc = fail(e, VIT_ERR_NOMEM, "out of host memory");
        /* the bf16 section is taken from the DEVICE (its own conversion), not re-derived on the host */
        if (!rc && bf16) memcpy(img->bf16, host + f32_floats, gemm_floats * sizeof(unsigned short));
    }
    free(host); free(tmp);
    return rc;
}

/* ---- stage launch helpers -------------------------------------------------------------------- */

static int stage_begin(vit_engine *e, vithip_stream_t s, int stage) {
    if (!e->opt.profile || e->ev_used >= MAX_EVENTS) return 0;
    e->ev_stage[e->ev_used] = stage;
    return vithip_event_record(e->ev[2 * e->ev_used], s);
}
static int stage_end(vit_engine *e, vithip_stream_t s) {
    if (!e->opt.profile || e->ev_used >= MAX_EVENTS) return 0;
    int rc = vithip_event_record(e->ev[2 * e->ev_used + 1], s);
    e->ev_used++;
    return rc;
}

/* One GEMM of the forward: fp32 operands, or bf16 ones (the encoder layers of a bf16 engine; C of the residual role stays fp32).
 * The residual role adds in place: C += A . W^T + bias.  ln_rows makes it the consumer of the LayerNorm fold: A holds the
 * un-normalised rows, W / bias the folded operands, ln_rows a pair per row of A -- fp32 (rstd, mean), bf16 (rstd, mean*rstd).
 * stats_rows makes a residual GEMM the producer, which leaves the pairs of the rows it stored in stats_rows:
 *   bf16: always -- its epilogue stores bf16(C) to x16 and the row sums to stats_part, and one small launch (accounted to the
 *         LayerNorm stage) turns them into the pairs;
 *   fp32: when its kernel can take the sums in its epilogue (the persistent walk: large batches); otherwise the caller runs the
 *         statistics pass, so that small batches keep their launch list and the stage profile its meaning.
 * *stats_ready (optional) says whether it left them. */
typedef struct {
    int stage, bf16;
    const void *A; int lda;
    vit_gemm_ops ops;                  /* W [N][K], bias; colsum and w_split: the fold's consumers and split engines */
    int ldw;                           /* fp32 GEMMs: floats from one row of W to the next; 0 = K (a column block of a wider W: the dense head) */
    void *C; int ldc;
    int M, N, K;
    int role;                          /* VITHIP_EPI_BIAS, VITHIP_EPI_BIAS_GELU, VITHIP_EPI_BIAS_QGELU or VITHIP_EPI_BIAS_RESIDUAL */
    const float *ln_rows;              /* consumer */
    float *stats_rows, *stats_part;    /* producer */
    unsigned short *x16;               /* bf16 producer: the bf16 copy of C, leading dimension ldc */
} gemm_desc;

static int gemm(vit_engine *e, vithip_stream_t s, const gemm_desc *g, int *stats_ready) {
    const float *res = g->role == VITHIP_EPI_BIAS_RESIDUAL ? (const float *)g->C : NULL;
    const int ldr = g->ln_rows ? 0 : g->ldc; /* read by the residual epilogue only; the fold's consumers pass 0 */
    int ready;
    HIP_TRY(e, stage_begin(e, s, g->stage));
    if (g->bf16) {
        static const int epi16[] = {[VITHIP_EPI_BIAS] = VITHIP_BF16_EPI_BF16, [VITHIP_EPI_BIAS_GELU] = VITHIP_BF16_EPI_BF16_GELU,
                                    [VITHIP_EPI_BIAS_RESIDUAL] = VITHIP_BF16_EPI_F32_RESIDUAL, [VITHIP_EPI_BIAS_QGELU] = VITHIP_BF16_EPI_BF16_QGELU};
        vithip_gemm_bf16_args a;
        memset(&a, 0, sizeof(a));
        a.A = g->A; a.lda = g->lda; a.W = g->ops.W; a.ldw = g->K; a.bias = g->ops.bias; a.residual = res; a.ldr = ldr;
        a.C = g->C; a.ldc = g->ldc; a.M = g->M; a.N = g->N; a.K = g->K; a.epilogue = epi16[g->role];
        a.ln_rows = g->ln_rows; a.ln_colsum = g->ops.colsum;
        if ((ready = g->stats_rows != NULL)) { a.x16 = g->x16; a.ldx16 = g->ldc; a.row_partials = g->stats_part; }
        HIP_TRY(e, vithip_gemm_bf16(s, &a));
    } else {
        vithip_gemm_args a;
        memset(&a, 0, sizeof(a));
        /* the lane's workspace: launches on one stream are ordered, which is what sharing it needs.  Lane 0 runs on the caller's
         * stream (whatever it is), lane j on aux_stream[j - 1]. */
        a.workspace = e->gemm_ws[0];
        for (int j = 0; j < VIT_MAX_LANES - 1; ++j)
            if (s == e->aux_stream[j]) a.workspace = e->gemm_ws[j + 1];
        a.handover_test = e->opt.gemm_handover_test; a.tile = e->opt.gemm_tile;
        a.arith = e->split && g->stage != VIT_STAGE_HEAD; /* every encoder GEMM (the embedding does not come through here) */
        a.w_split = a.arith ? g->ops.w_split : NULL;
        a.A = g->A; a.lda = g->lda; a.W = g->ops.W; a.ldw = g->ldw ? g->ldw : g->K; a.bias = g->ops.bias; a.residual = res; a.ldr = ldr;
        a.C = g->C; a.ldc = g->ldc; a.M = g->M; a.N = g->N; a.K = g->K; a.epilogue = g->role;
        a.ln_rows = g->ln_rows; a.ln_colsum = g->ops.colsum;
        a.stats_out = g->stats_rows; a.stats_partials = g->stats_part; a.stats_eps = e->ln_eps;
        if (!(ready = vithip_gemm_f32_stats_in_epilogue(&a))) a.stats_out = a.stats_partials = NULL;
        HIP_TRY(e, vithip_gemm_f32(s, &a));
    }
    HIP_TRY(e, stage_end(e, s));
    if (g->bf16 && ready) {
        HIP_TRY(e, stage_begin(e, s, VIT_STAGE_LN));
        HIP_TRY(e, vithip_rowstats_finalize_eps(s, g->stats_part, vithip_ln_strips(g->N), g->M, g->N, g->stats_rows, e->ln_eps));
        HIP_TRY(e, stage_end(e, s));
    }
    if (stats_ready) *stats_ready = ready;
    return VIT_OK;
}

static int collect_profile(vit_engine *e) {
    if (e->ev_used == 0) return VIT_OK;
    HIP_TRY(e, vithip_device_sync()); /* brackets may sit on several lane streams */
    for (int i = 0; i < e->ev_used; ++i) {
        float ms = 0.f;
        HIP_TRY(e, vithip_event_elapsed_ms(&ms, e->ev[2 * i], e->ev[2 * i + 1]));
        e->times.ms[e->ev_stage[i]] += ms;
        e->times.launches[e->ev_stage[i]]++;
    }
    e->times.images += e->pending_images;
    e->pending_images = 0;
    e->ev_used = 0;
    return VIT_OK;
}

/*
 * One chunk of nb <= max_batch images, everything device resident.
 *
 * With opt.lanes > 1 the chunk is cut into that many sub-batches that run the same stage sequence
 * on their own HIP streams (lane 0 on the caller's stream, which forks and joins the others with
 * events).  The sub-batches are independent -- images never interact -- so this adds no
 * synchronisation to the data path; what it buys is that the low-occupancy and HBM-bound kernels of
 * one lane run beside the other lane's GEMMs.  Launches are issued stage by stage across the lanes so
 * that the queues advance together.
 *
 * Every encoder layer runs the one step sequence of encoder_layer(), whatever the dtype, the LayerNorm
 * fold and the class-rows-only "pruned last layer"; each step is issued for every lane.
 */
typedef struct {
    vithip_stream_t s;
    int off, n; /* first image of the lane inside the chunk, image count */
    int stats_ready; /* fold: the residual GEMM in front has left the pairs of the lane's token rows (see gemm()) */
    /* the lane's rows of the activation buffers, from its first token row (off * T) on; bf16 activations fill the fp32-sized
     * allocations of y, qkv and hbuf from their start */
    float *x;
    void *y, *qkv, *h;
    /* LayerNorm fold (NULL without it): the rows in_proj and fc1 read (x itself, or its bf16 copy), the pairs of the token rows
     * and of the class rows, the residual GEMMs' partial sums */
    void *xa;
    float *tok_pairs, *cls_pairs, *partials;
} vit_lane;

typedef struct {
    vit_engine *e;
    vit_lane lane[VIT_MAX_LANES];
    int L;                       /* lanes in use for this chunk */
    int T, D, H, NC;
    int H1;                      /* columns of a row of the lanes' h: VIT_FC1_ROWS (H; 2H under SwiGLU, [gate -> hidden | value]) */
    size_t esz;                  /* bytes of an element of the lanes' y, qkv and h: 4, or 2 on bf16 engines */
    int pruned;                  /* the last layer computes the class rows only: prune_last_layer, where the chunk's output reads no others (class_rows_only) */
    int qkv_only;                /* the last layer stops behind its QKV GEMM: the chunk's output is read from its Q and K (attention calls) */
    size_t row;                  /* bytes per image of the chunk's output rows (the kind's row_bytes) */
} chunk_ctx;

#define RUN(call) do { int rc_ = (call); if (rc_) return rc_; } while (0)

/* conv_proj + flatten_transpose + class_token + pos_emb (ViT_seq.c:25-101).  8-bit input: each lane first normalises its own
 * images into the same rows of f32_stage (one more launch of the embed stage) and embeds from there; decoded images of any size
 * (d_images = the chunk's records): the lane's slice of the records is resized, cropped and normalised into those rows (one launch
 * of the embed stage per 64 images). */
static int stage_embed(chunk_ctx *c, const void *d_images, const vit_input *in, float *f32_stage) {
    vit_engine *e = c->e;
    const vit_config *cfg = &e->cfg;
    const vit_embed_ops *w = &e->embed;
    const size_t img = (size_t)cfg->in_chans * cfg->img_size * cfg->img_size;
    /* bf16 patch embedding needs K = chans*patch^2 to be a multiple of 64 (two K steps at least) and patch % 8 == 0;
     * its bf16 patch rows live in the (still unused) hidden-layer buffer */
    const int patch = VIT_PATCH_SIZE(cfg), regs = e->prefix - 1, pk = cfg->in_chans * patch * patch;
    const int embed16 = e->opt.dtype == VIT_DTYPE_BF16 && pk % 64 == 0 && pk >= 128 && patch % 8 == 0 &&
                        (size_t)pk <= 2 * (size_t)c->H;
    for (int j = 0; j < c->L; ++j) {
        const vit_lane *ln = &c->lane[j];
        const float *images = in->kind != VIT_IN_F32 ? f32_stage + ln->off * img : (const float *)d_images + ln->off * img;
        if (in->kind != VIT_IN_F32) {
            HIP_TRY(e, stage_begin(e, ln->s, VIT_STAGE_EMBED));
            if (in->kind == VIT_IN_IMAGES)
                HIP_TRY(e, vithip_images_u8_resize_crop_to_f32_filter(ln->s, (const vithip_image_u8 *)d_images + ln->off, ln->n,
                                                                      f32_stage + ln->off * img, cfg->img_size, cfg->in_chans,
                                                                      in->resize_shorter, in->resize_filter, in->mean, in->std));
            else
                HIP_TRY(e, vithip_images_u8_to_f32(ln->s, (const unsigned char *)d_images + ln->off * img, f32_stage + ln->off * img,
                                                   ln->n, cfg->img_size, cfg->in_chans, in->mean, in->std));
            HIP_TRY(e, stage_end(e, ln->s));
        }
        HIP_TRY(e, stage_begin(e, ln->s, VIT_STAGE_EMBED));
        if (embed16)
            HIP_TRY(e, vithip_patch_embed_bf16_reg(ln->s, images, w->conv_w16, w->conv_b, w->cls, w->pos, ln->x,
                                                   (unsigned short *)e->hbuf + (size_t)ln->off * (size_t)e->patches * pk,
                                                   ln->n, cfg->img_size, patch, cfg->in_chans, c->D, regs));
        else
            HIP_TRY(e, vithip_patch_embed_f32_reg(ln->s, images, w->conv_w, w->conv_b, w->cls, w->pos, ln->x, ln->n,
                                                  cfg->img_size, patch, cfg->in_chans, c->D, regs));
        HIP_TRY(e, stage_end(e, ln->s));
    }
    return VIT_OK;
}

/* LayerNorm (ViT_seq.c:103-121) of `rows` rows of x into y (bf16 on bf16 engines) */
static int layernorm(chunk_ctx *c, vithip_stream_t s, const float *x, size_t ldx, void *y, size_t ldy, const float *gamma,
                     const float *beta, int rows) {
    vit_engine *e = c->e;
    HIP_TRY(e, stage_begin(e, s, VIT_STAGE_LN));
    if (e->opt.dtype == VIT_DTYPE_BF16) HIP_TRY(e, vithip_layernorm_f32_bf16out_eps(s, x, ldx, y, ldy, gamma, beta, rows, c->D, e->ln_eps));
    else HIP_TRY(e, vithip_layernorm_f32_eps(s, x, ldx, y, ldy, gamma, beta, rows, c->D, e->ln_eps));
    HIP_TRY(e, stage_end(e, s));
    return VIT_OK;
}

/* the fold's statistics pass over `rows` rows of the lane's x (leading dimension ldx): a pair per row into `pairs`; bf16 engines
 * also write the bf16 copy of the rows, which the consumers read */
static int row_stats(chunk_ctx *c, const vit_lane *ln, size_t ldx, float *pairs, int rows) {
    vit_engine *e = c->e;
    HIP_TRY(e, stage_begin(e, ln->s, VIT_STAGE_LN));
    if (e->opt.dtype == VIT_DTYPE_BF16) HIP_TRY(e, vithip_rowstats_bf16_eps(ln->s, ln->x, ldx, ln->xa, ldx, pairs, rows, c->D, e->ln_eps));
    else HIP_TRY(e, vithip_rowstats_f32_eps(ln->s, ln->x, ldx, pairs, rows, c->D, e->ln_eps));
    HIP_TRY(e, stage_end(e, ln->s));
    return VIT_OK;
}

/*
 * Encoder layer l (ViT_seq.c:276-300): LN1 -> QKV in_proj -> attention -> out_proj + residual -> LN2 -> fc1 + GELU -> fc2 +
 * residual, each step issued for every lane before the next one starts.  What varies is where rows are and which kernel runs:
 *   mlp     VIT_MLP_SWIGLU: fc1 is the bias-only GEMM of the fused w12, N = 2H, into rows of 2H columns [gate | value]; one launch
 *           (vithip_swiglu_*, still the fc1 stage) turns the gate half into the hidden layer silu(gate) * value in place; fc2 reads it
 *           there, lda = 2H.  The GEMMs know nothing of it, and a GELU engine's launches are the ones they were.
 *           VIT_MLP_QUICKGELU: the launches of a GELU engine with fc1's epilogue role VITHIP_EPI_BIAS_QGELU in VITHIP_EPI_BIAS_GELU's place.
 *   dtype   bf16 engines keep the LN output, qkv, the attention output and the MLP hidden layer in bf16; the residual stream x,
 *           the LayerNorm statistics, softmax and every accumulation stay fp32.
 *   fold    the LayerNorm fold (vit_hip_kernels.h, "LayerNorm folding"): in_proj and fc1 read the raw rows (x, or its bf16 copy)
 *           with the gamma/beta-folded operands (vit_layer_ops) and a pair per row; a LayerNorm becomes a statistics pass,
 *           or nothing where the residual GEMM in front has left the pairs.  The bf16 Q rows carry the scores' exponent factor.
 *   pruned  prune_last_layer, for chunks whose output reads the class rows only (class_rows_only: probabilities, CLS features and CLS taps;
 *           MEAN and TOKENS run the layer in full): K and V of every token, everything else for the class rows only.  The class rows of a [n*T][w]
 *           buffer are rows 0, T, 2T, ... = a matrix with leading dimension T*w, which every operator takes as it is.
 *   qkv_only  attention calls: the last layer ends behind in_proj, with K of every token and Q of (at least) the class rows in the
 *           lanes' qkv rows, where stage_cls_attention reads them; pruned or not, those are the same bits.
 */
static int encoder_layer(chunk_ctx *c, int l) {
    vit_engine *e = c->e;
    const int T = c->T, D = c->D, H = c->H, H1 = c->H1, heads = e->cfg.num_heads, swiglu = VIT_MLP_KIND(&e->cfg) == VIT_MLP_SWIGLU;
    /* fc1's epilogue by MLP kind: the activation of a GELU or QuickGELU model is part of the GEMM; SwiGLU's gate is a launch behind it */
    const int fc1_role = swiglu ? VITHIP_EPI_BIAS : VIT_MLP_KIND(&e->cfg) == VIT_MLP_QUICKGELU ? VITHIP_EPI_BIAS_QGELU : VITHIP_EPI_BIAS_GELU;
    const int bf16 = e->opt.dtype == VIT_DTYPE_BF16, fold = e->fold, feeds_next = l + 1 < e->cfg.depth;
    const int pruned = c->pruned && !feeds_next;
    const vit_layer_ops *o = &e->layer[l];
    /* the rows the layer computes past K and V: every token row, or the class rows (row step T); and their pairs (fold) */
    const int r = pruned ? T : 1;
    int rows[VIT_MAX_LANES], ln2_ready[VIT_MAX_LANES];
    float *pairs[VIT_MAX_LANES];
    for (int j = 0; j < c->L; ++j) {
        rows[j] = pruned ? c->lane[j].n : c->lane[j].n * T;
        pairs[j] = pruned ? c->lane[j].cls_pairs : c->lane[j].tok_pairs;
    }

    for (int j = 0; j < c->L; ++j) { /* LN1 (ViT_seq.c:281); folded: its statistics, unless the fc2 in front has left them */
        vit_lane *ln = &c->lane[j];
        if (!fold) RUN(layernorm(c, ln->s, ln->x, D, ln->y, D, o->ln1_g, o->ln1_b, ln->n * T));
        else if (!ln->stats_ready) RUN(row_stats(c, ln, D, ln->tok_pairs, ln->n * T));
    }
    for (int j = 0; j < c->L; ++j) { /* QKV in_proj (ViT_seq.c:134-147) */
        vit_lane *ln = &c->lane[j];
        gemm_desc g = {.stage = VIT_STAGE_QKV, .bf16 = bf16, .A = fold ? ln->xa : ln->y, .lda = D, .ops = o->qkv, .C = ln->qkv,
                       .ldc = 3 * D, .M = ln->n * T, .N = 3 * D, .K = D, .role = VITHIP_EPI_BIAS, .ln_rows = ln->tok_pairs};
        if (pruned) { /* K and V of every token (in_proj rows D..3D), then Q of the class rows, whose pairs are gathered first */
            gemm_desc kv = g;
            kv.ops.W = at(g.ops.W, (size_t)D * D, c->esz); kv.ops.bias = g.ops.bias + D; kv.C = at(ln->qkv, D, c->esz); kv.N = 2 * D;
            kv.ops.colsum = g.ops.colsum ? g.ops.colsum + D : NULL;
            /* the image of rows D.. starts at a panel boundary only when D is a multiple of 128 (panel = 128 rows x K x 6 bytes) */
            kv.ops.w_split = g.ops.w_split && D % 128 == 0 ? at(g.ops.w_split, (size_t)D * D * 6, 1) : NULL;
            RUN(gemm(e, ln->s, &kv, NULL));
            if (fold) {
                HIP_TRY(e, stage_begin(e, ln->s, VIT_STAGE_LN));
                HIP_TRY(e, vithip_gather_rows_f32(ln->s, ln->tok_pairs, (size_t)2 * T, ln->cls_pairs, 2, ln->n, 2));
                HIP_TRY(e, stage_end(e, ln->s));
            }
            g.lda = r * D; g.ldc = r * 3 * D; g.M = rows[j]; g.N = D; g.ln_rows = pairs[j];
        }
        RUN(gemm(e, ln->s, &g, NULL));
    }
    if (c->qkv_only && !feeds_next) return VIT_OK;
    for (int j = 0; j < c->L; ++j) { /* scores, softmax, P.V (ViT_seq.c:156-215) -> y; pruned: for the class rows */
        const vit_lane *ln = &c->lane[j];
        HIP_TRY(e, stage_begin(e, ln->s, VIT_STAGE_ATTN));
        /* head_dim 64: the entries these generalise (_f32 / _f32_rows, _bf16io / _rows / _qscaled), their launches and their bits */
        /* fp32 with the split on (fp32_split >= 0), head_dim 64: both products on the bf16 matrix pipe, like the GEMMs around them */
        if (!bf16 && e->split && D / heads == 64)
            HIP_TRY(e, vithip_attention_f32_split(ln->s, ln->qkv, ln->y, ln->n, T, heads, 64, pruned ? 1 : T));
        else if (!bf16) HIP_TRY(e, vithip_attention_f32_hd(ln->s, ln->qkv, ln->y, ln->n, T, heads, D / heads, pruned ? 1 : T));
        else HIP_TRY(e, vithip_attention_bf16io_hd(ln->s, ln->qkv, ln->y, ln->n, T, heads, D / heads, pruned ? 1 : T, fold));
        HIP_TRY(e, stage_end(e, ln->s));
    }
    for (int j = 0; j < c->L; ++j) { /* out_proj + residual (ViT_seq.c:219-227,286-288): x += y . Wo^T + bo; folded, it also
                                      * leaves the pairs of LN2 -- except in the pruned fp32 layer, which takes them in a pass */
        vit_lane *ln = &c->lane[j];
        gemm_desc g = {.stage = VIT_STAGE_OUTPROJ, .bf16 = bf16, .A = ln->y, .lda = r * D, .ops = o->out, .C = ln->x,
                       .ldc = r * D, .M = rows[j], .N = D, .K = D, .role = VITHIP_EPI_BIAS_RESIDUAL};
        if (fold && (bf16 || !pruned)) { g.stats_rows = pairs[j]; g.stats_part = ln->partials; g.x16 = bf16 ? ln->xa : NULL; }
        RUN(gemm(e, ln->s, &g, &ln2_ready[j]));
    }
    for (int j = 0; j < c->L; ++j) { /* LN2 (ViT_seq.c:291); pruned: of the class rows, into a compact [n][D] at the head of y */
        const vit_lane *ln = &c->lane[j];
        if (!fold) RUN(layernorm(c, ln->s, ln->x, (size_t)r * D, ln->y, D, o->ln2_g, o->ln2_b, rows[j]));
        else if (!ln2_ready[j]) RUN(row_stats(c, ln, (size_t)r * D, pairs[j], rows[j]));
    }
    for (int j = 0; j < c->L; ++j) { /* fc1 + GELU (ViT_seq.c:258-264); SwiGLU: w12 + bias, then the gate */
        const vit_lane *ln = &c->lane[j];
        gemm_desc g = {.stage = VIT_STAGE_FC1, .bf16 = bf16, .A = ln->y, .lda = D, .ops = o->fc1, .C = ln->h, .ldc = H1,
                       .M = rows[j], .N = H1, .K = D, .role = fc1_role};
        if (fold) { g.A = ln->xa; g.lda = r * D; g.ln_rows = pairs[j]; }
        RUN(gemm(e, ln->s, &g, NULL));
        if (swiglu) {
            HIP_TRY(e, stage_begin(e, ln->s, VIT_STAGE_FC1));
            if (bf16) HIP_TRY(e, vithip_swiglu_bf16(ln->s, ln->h, (size_t)H1, ln->h, (size_t)H1, rows[j], H));
            else HIP_TRY(e, vithip_swiglu_f32(ln->s, ln->h, (size_t)H1, ln->h, (size_t)H1, rows[j], H));
            HIP_TRY(e, stage_end(e, ln->s));
        }
    }
    for (int j = 0; j < c->L; ++j) { /* fc2 + residual (ViT_seq.c:266,297-299): x += h . W2^T + b2; folded, it also leaves the
                                      * pairs of the next layer's LN1 when there is one */
        vit_lane *ln = &c->lane[j];
        gemm_desc g = {.stage = VIT_STAGE_FC2, .bf16 = bf16, .A = ln->h, .lda = H1, .ops = o->fc2, .C = ln->x, .ldc = r * D,
                       .M = rows[j], .N = D, .K = H, .role = VITHIP_EPI_BIAS_RESIDUAL};
        if (fold && feeds_next) { g.stats_rows = ln->tok_pairs; g.stats_part = ln->partials; g.x16 = bf16 ? ln->xa : NULL; }
        RUN(gemm(e, ln->s, &g, &ln->stats_ready));
    }
    return VIT_OK;
}

/* The final blocks: what a chunk returns from the residual stream (the head's operand, embedding rows, tapped layers) is made of
 * three kinds of block with one writer each.  A writer serves one lane inside the bracket its caller has opened and writes the block
 * of each of the lane's images at dst, dst + ld, ..: ld is an image's whole row, the caller's or the head's operand's.
 * class_block: the final LayerNorm of the class rows (ViT_seq.c:429-433 normalises all rows, uses row 0): row step T*D, exactly the
 * rows a pruned last layer has updated.  Not vithip_tap_f32 with VITHIP_TAP_CLS: the same bits, but another launch. */
static int class_block(chunk_ctx *c, const vit_lane *ln, float *dst, size_t ld) {
    HIP_TRY(c->e, vithip_layernorm_f32_eps(ln->s, ln->x, (size_t)c->T * c->D, dst, ld, c->e->final.ln_g, c->e->final.ln_b, ln->n, c->D, c->e->ln_eps));
    return VIT_OK;
}

/* The pooling scratch is the head of the lane's OWN rows of y (ln->y: n * T * D elements of 4 or, bf16 engines, 2 bytes), which the
 * lane's own stream has finished with behind its last layer.  Nothing of another lane may be touched: lanes run on independent
 * streams and the others may still be in their last layer, reading their y and (fold) the bf16 copy of x in y's upper half.  The
 * scratch is one [D] fp32 row per 16 tokens, at most n * T * D * 2 bytes for every T >= 2; checked by pooled_block all the same. */
static float *pool_scratch(const chunk_ctx *c, const vit_lane *ln, size_t *bytes) {
    *bytes = vithip_layernorm_pool_f32_workspace_floats(ln->n, c->T, c->e->prefix, c->D) * sizeof(float);
    return (float *)ln->y;
}

/* pooled_block: the mean over the patch tokens: normalise, then pool (l2: and L2-normalise the mean) or, fcnorm, pool, then
 * normalise; both kernels keep the same partial rows in the scratch.  who: the caller, for the message. */
static int pooled_block(chunk_ctx *c, const vit_lane *ln, float *dst, size_t ld, int fcnorm, int l2, const char *who) {
    vit_engine *e = c->e;
    const size_t D = (size_t)c->D, own = (size_t)ln->n * c->T * D * c->esz;
    size_t need;
    float *scratch = pool_scratch(c, ln, &need);
    if (need == 0 || need > own || ((size_t)scratch & 15))
        return fail(e, VIT_ERR_STATE, "%s: the pooling scratch (%zu bytes) does not fit the lane's own %zu bytes of y", who, need, own);
    if (fcnorm) HIP_TRY(e, vithip_pool_layernorm_f32_eps(ln->s, ln->x, D, dst, ld, e->final.ln_g, e->final.ln_b, ln->n, c->T, e->prefix, c->D, scratch, e->ln_eps));
    else HIP_TRY(e, vithip_layernorm_pool_f32_eps(ln->s, ln->x, D, dst, ld, e->final.ln_g, e->final.ln_b, ln->n, c->T, e->prefix, c->D, l2, scratch, e->ln_eps));
    return VIT_OK;
}

/* tap_block: the rows `kind` (VITHIP_TAP_*) names of x as the layer in front has just left it; norm: through the final LayerNorm */
static int tap_block(chunk_ctx *c, const vit_lane *ln, float *dst, size_t ld, int norm, int kind) {
    const vit_final_ops *f = &c->e->final;
    HIP_TRY(c->e, vithip_tap_f32_prefix_eps(ln->s, ln->x, (size_t)c->D, dst, ld, norm ? f->ln_g : NULL, norm ? f->ln_b : NULL, ln->n, c->T,
                                            c->e->prefix, c->D, kind, c->e->ln_eps));
    return VIT_OK;
}

/* The head (vit_head): the blocks of the last layer into the operand rows -- the class blocks of earlier layers are in place
 * (stage_head_tap) --, classifier head (ViT_seq.c:435), Softmax (ViT_seq.c:437) + top-1 (Main.c:62-70) -- or, for a top-k call, the k
 * best classes of the same logits as records in the softmax's place: out->dst is then [n][2k] 32-bit words and nothing of
 * [n][classes] is written; or, for a features call of VIT_FEAT_HEAD, the logits rows themselves, copied to the caller's rows (and
 * L2-normalised there when the spec says so).  The checkpoint's own head is the case K = 1, in = D: one class block per lane into z, ld = D. */
static int runs_head(const vit_output *out) {
    return out->kind == VIT_OUT_PROBS || out->kind == VIT_OUT_TOPK || (out->kind == VIT_OUT_FEATURES && out->spec.kind == VIT_FEAT_HEAD);
}
static int stage_head(chunk_ctx *c, const vit_output *out) {
    vit_engine *e = c->e;
    const vit_head *h = &e->head;
    const int NC = c->NC, K = h->spec.num_cls_layers, F = (int)h->in;
    for (int j = 0; j < c->L; ++j) {
        const vit_lane *ln = &c->lane[j];
        float *row = h->operand + (size_t)ln->off * h->in;
        HIP_TRY(e, stage_begin(e, ln->s, VIT_STAGE_LN));
        if (K && h->spec.cls_layers[K - 1] == e->cfg.depth - 1) RUN(class_block(c, ln, row + (size_t)(K - 1) * c->D, h->in));
        if (h->spec.pool != VIT_HEAD_POOL_NONE)
            RUN(pooled_block(c, ln, row + (size_t)K * c->D, h->in, h->spec.pool == VIT_HEAD_POOL_AVG_FCNORM, 0, "head"));
        HIP_TRY(e, stage_end(e, ln->s));
    }
    for (int j = 0; j < c->L; ++j) {
        const vit_lane *ln = &c->lane[j];
        const gemm_desc g = {.stage = VIT_STAGE_HEAD, .A = h->operand + (size_t)ln->off * F, .lda = F, .ops = h->ops,
                             .C = e->logits + (size_t)ln->off * NC, .ldc = NC, .M = ln->n, .N = NC, .K = F, .role = VITHIP_EPI_BIAS};
        RUN(gemm(e, ln->s, &g, NULL));
    }
    for (int j = 0; j < c->L; ++j) {
        const vit_lane *ln = &c->lane[j];
        const size_t o = (size_t)ln->off;
        if (out->kind == VIT_OUT_FEATURES) { /* VIT_FEAT_HEAD: the rows of e->logits as they are (vit_engine_read_logits keeps the
                                              * un-normalised ones), then F.normalize on the caller's copy */
            float *dst = out->dst + o * (c->row / sizeof(float));
            HIP_TRY(e, stage_begin(e, ln->s, VIT_STAGE_HEAD));
            HIP_TRY(e, vithip_gather_rows_f32(ln->s, e->logits + o * NC, (size_t)NC, dst, (size_t)NC, ln->n, NC));
            if (out->spec.l2_normalize) HIP_TRY(e, vithip_l2_normalize_rows_f32(ln->s, dst, (size_t)NC, ln->n, NC));
            HIP_TRY(e, stage_end(e, ln->s));
            continue;
        }
        HIP_TRY(e, stage_begin(e, ln->s, VIT_STAGE_SOFTMAX));
        if (out->kind == VIT_OUT_TOPK)
            HIP_TRY(e, vithip_softmax_topk_f32(ln->s, e->logits + o * NC, NC, (int *)out->dst + o * 2 * (size_t)out->topk.k, 2 * out->topk.k, ln->n, NC,
                                               out->topk.k, out->topk.score));
        else
            HIP_TRY(e, vithip_softmax_top1_f32(ln->s, e->logits + o * NC, NC, out->dst + o * NC, NC, out->label ? out->label + o : NULL, out->prob ? out->prob + o : NULL, ln->n, NC));
        HIP_TRY(e, stage_end(e, ln->s));
    }
    return VIT_OK;
}

/* The embedding rows of the chunk instead of the head: the class block (the checkpoint's own head's operand, in the caller's rows),
 * the final LayerNorm of every row, or the pooled block. */
static int stage_features(chunk_ctx *c, const vit_output *out) {
    vit_engine *e = c->e;
    const size_t D = (size_t)c->D;
    for (int j = 0; j < c->L; ++j) {
        const vit_lane *ln = &c->lane[j];
        float *dst = out->dst + (size_t)ln->off * (c->row / sizeof(float));
        HIP_TRY(e, stage_begin(e, ln->s, VIT_STAGE_LN));
        if (out->spec.kind == VIT_FEAT_CLS) {
            RUN(class_block(c, ln, dst, D));
            if (out->spec.l2_normalize) HIP_TRY(e, vithip_l2_normalize_rows_f32(ln->s, dst, D, ln->n, c->D));
        } else if (out->spec.kind == VIT_FEAT_TOKENS)
            HIP_TRY(e, vithip_layernorm_f32_eps(ln->s, ln->x, D, dst, D, e->final.ln_g, e->final.ln_b, ln->n * c->T, c->D, e->ln_eps));
        else RUN(pooled_block(c, ln, dst, D, 0, out->spec.l2_normalize, "features"));
        HIP_TRY(e, stage_end(e, ln->s));
    }
    return VIT_OK;
}

/* The class token's attention of the last layer instead of everything behind its in_proj: one launch per lane over the lane's qkv
 * rows as encoder_layer (qkv_only) left them -- Q of the class rows at row step T, K of every token; bf16 fold engines keep
 * vithip_qscale(head_dim) * q there.  Nothing has written those rows since: the fold's statistics live in other allocations (fp32) or in the
 * upper half of qkv's (bf16; chunk_setup), and the next writer is the next chunk's first in_proj on the same streams. */
static int stage_cls_attention(chunk_ctx *c, const vit_output *out) {
    vit_engine *e = c->e;
    const int heads = e->cfg.num_heads, hd = c->D / heads, mean = out->attn_kind == VIT_ATTN_HEAD_MEAN;
    const size_t row = c->row / sizeof(float), ld = 3 * (size_t)c->D;
    for (int j = 0; j < c->L; ++j) {
        const vit_lane *ln = &c->lane[j];
        float *dst = out->dst + (size_t)ln->off * row;
        HIP_TRY(e, stage_begin(e, ln->s, VIT_STAGE_ATTN));
        if (e->opt.dtype == VIT_DTYPE_BF16)
            HIP_TRY(e, vithip_cls_attention_bf16_hd(ln->s, (const unsigned short *)ln->qkv, ld, dst, row, ln->n, c->T, heads, hd, mean, e->fold));
        else
            HIP_TRY(e, vithip_cls_attention_f32_hd(ln->s, (const float *)ln->qkv, ld, dst, row, ln->n, c->T, heads, hd, mean));
        HIP_TRY(e, stage_end(e, ln->s));
    }
    return VIT_OK;
}

/* floats of one tapped layer's block of an intermediate row; `kind` is the VIT_TAP_* of a valid spec */
static size_t tap_block_elems(const vit_engine *e, int kind) {
    return (kind == VIT_TAP_CLS ? 1 : kind == VIT_TAP_TOKENS ? (size_t)e->tokens : (size_t)e->patches) * (size_t)e->cfg.embed_dim;
}

/* An intermediate call behind encoder layer l = layers[j] (any other layer: nothing) -- block j of its rows: the residual stream as
 * the layer has just left it, one tap block per lane.  A pruned last layer (CLS only) has updated the class rows of x alone, which
 * is all that CLS reads. */
static int stage_tap(chunk_ctx *c, const vit_output *out, int l) {
    vit_engine *e = c->e;
    const size_t row = c->row / sizeof(float), block = tap_block_elems(e, out->tap.kind);
    int j = 0;
    while (j < out->tap.num_layers && out->tap.layers[j] != l) ++j;
    if (j == out->tap.num_layers) return VIT_OK;
    for (int k = 0; k < c->L; ++k) {
        const vit_lane *ln = &c->lane[k];
        HIP_TRY(e, stage_begin(e, ln->s, VIT_STAGE_LN));
        RUN(tap_block(c, ln, out->dst + (size_t)ln->off * row + (size_t)j * block, row, out->tap.norm, out->tap.kind));
        HIP_TRY(e, stage_end(e, ln->s));
    }
    return VIT_OK;
}

/* A dense call behind encoder layer l = the head's layers[j] (any other layer: nothing): per lane the patch rows of x as the layer
 * has just left them (the tap of an intermediate call of VIT_TAP_PATCHES) into the head's scratch, then the GEMM of the chain over
 * them -- the first writes bias + A_0 . W_0^T, the later ones add A_j . W_j^T in place, W_j the column block j of the head's W.
 * fp32 MFMA on both dtypes.  The spec of the call (out) has no say in it: the layers are the head's. */
static int stage_dense_tap(chunk_ctx *c, const vit_output *out, int l) {
    vit_engine *e = c->e;
    const vit_dense_head *h = &e->dense;
    const size_t P = (size_t)e->patches, D = (size_t)c->D;
    const int NC = h->spec.num_classes, K = h->spec.num_layers;
    int j = 0;
    (void)out;
    while (j < K && h->spec.layers[j] != l) ++j;
    if (j == K) return VIT_OK;
    for (int k = 0; k < c->L; ++k) {
        const vit_lane *ln = &c->lane[k];
        HIP_TRY(e, stage_begin(e, ln->s, VIT_STAGE_LN));
        RUN(tap_block(c, ln, h->rows + (size_t)ln->off * P * D, P * D, h->spec.norm, VITHIP_TAP_PATCHES));
        HIP_TRY(e, stage_end(e, ln->s));
    }
    for (int k = 0; k < c->L; ++k) {
        const vit_lane *ln = &c->lane[k];
        const gemm_desc g = {.stage = VIT_STAGE_HEAD, .A = h->rows + (size_t)ln->off * P * D, .lda = c->D,
                             .ops = {.W = h->W + (size_t)j * D, .bias = j ? h->zero_bias : h->bias}, .ldw = K * c->D,
                             .C = h->logits + (size_t)ln->off * P * NC, .ldc = NC, .M = ln->n * (int)P, .N = NC, .K = c->D,
                             .role = j ? VITHIP_EPI_BIAS_RESIDUAL : VITHIP_EPI_BIAS};
        RUN(gemm(e, ln->s, &g, NULL));
    }
    return VIT_OK;
}

/* ... and behind the deepest of them: the lane's logits [n][P][classes] become its images' rows -- the labels of the upsampled maps
 * (nothing of full resolution but the labels is written) or the channel-major grid. */
static int stage_dense_out(chunk_ctx *c, const vit_output *out) {
    vit_engine *e = c->e;
    const vit_dense_head *h = &e->dense;
    const int g = e->cfg.img_size / VIT_PATCH_SIZE(&e->cfg), NC = h->spec.num_classes;
    const size_t P = (size_t)e->patches, row = c->row;
    for (int k = 0; k < c->L; ++k) {
        const vit_lane *ln = &c->lane[k];
        const float *logits = h->logits + (size_t)ln->off * P * NC;
        unsigned char *dst = (unsigned char *)out->dst + (size_t)ln->off * row;
        HIP_TRY(e, stage_begin(e, ln->s, VIT_STAGE_SOFTMAX));
        if (out->dense.kind == VIT_DENSE_LABELS)
            HIP_TRY(e, vithip_dense_upsample_argmax_f32(ln->s, logits, NC, P * NC, dst, row, ln->n, g, NC, out->dense.out_h, out->dense.out_w));
        else
            HIP_TRY(e, vithip_dense_grid_f32(ln->s, logits, NC, P * NC, (float *)dst, row / sizeof(float), ln->n, g, NC));
        HIP_TRY(e, stage_end(e, ln->s));
    }
    return VIT_OK;
}

/* The head's operand row of an image is [class blocks, in the order of cls_layers | pooled block], head.in floats.  Behind encoder
 * layer l < depth - 1 when cls_layers names it: the class block of that layer, the launch (and so the bits) of an intermediate call
 * with VIT_TAP_CLS, norm = 1.  The blocks of the last layer are stage_head's; the checkpoint's own head names no other layer.
 * Nothing for a features call of plain embedding rows, which runs no head. */
static int stage_head_tap(chunk_ctx *c, const vit_output *out, int l) {
    vit_engine *e = c->e;
    const vit_head *h = &e->head;
    int k = 0;
    while (k < h->spec.num_cls_layers && h->spec.cls_layers[k] != l) ++k;
    if (!runs_head(out) || k == h->spec.num_cls_layers || l == e->cfg.depth - 1) return VIT_OK;
    for (int j = 0; j < c->L; ++j) {
        const vit_lane *ln = &c->lane[j];
        HIP_TRY(e, stage_begin(e, ln->s, VIT_STAGE_LN));
        RUN(tap_block(c, ln, h->operand + (size_t)ln->off * h->in + (size_t)k * c->D, h->in, 1, VITHIP_TAP_CLS));
        HIP_TRY(e, stage_end(e, ln->s));
    }
    return VIT_OK;
}

/* What the engine knows of an output kind, all of it: OUT_KINDS below has one row per VIT_OUT_*, and a new kind is a row and its
 * own functions.  A hook that is absent (NULL) gives the plain answer named with it. */
typedef struct {
    /* The caller's spec, checked against the model and copied into *out (zeroed, its kind set: output_fault): NULL, or what is wrong
     * with it as a format for (who, arg[0], arg[1]) -- the calls and the public row widths ask the same question.  Absent: no spec. */
    const char *(*check)(const vit_engine *e, const void *spec, vit_output *out, int arg[2]);
    size_t (*row_bytes)(const vit_engine *e, const vit_output *out); /* bytes per image of the caller's rows */
    /* Whether the kind reads, of x behind the last layer, the class rows alone, which are all a pruned last layer updates.  Absent:
     * no -- the layer runs in full, so a new output cannot silently return rows of the layer before. */
    int (*class_rows_only)(const vit_engine *e, const vit_output *out);
    int (*last_layer)(const vit_engine *e, const vit_output *out); /* the deepest encoder layer that runs; absent: depth - 1 */
    int (*after_layer)(chunk_ctx *c, const vit_output *out, int l); /* what runs behind encoder layer l; absent: nothing */
    int (*finish)(chunk_ctx *c, const vit_output *out);             /* the stage behind the walk; absent: nothing */
    int qkv_only; /* the last layer stops behind its QKV GEMM (chunk_ctx.qkv_only) */
} vit_out_kind;

/* The forwards, the top-k calls and the features calls share their hooks: a features call of VIT_FEAT_HEAD runs the head as they do
 * (runs_head), one of plain embedding rows stage_features in its place. */
static int head_or_class_rows_only(const vit_engine *e, const vit_output *out) {
    if (runs_head(out)) return e->head.spec.pool == VIT_HEAD_POOL_NONE; /* a pooled block reads every patch row */
    return out->spec.kind == VIT_FEAT_CLS; /* MEAN and TOKENS read every row */
}
static int stage_head_or_features(chunk_ctx *c, const vit_output *out) {
    return runs_head(out) ? stage_head(c, out) : stage_features(c, out);
}

static size_t probs_row_bytes(const vit_engine *e, const vit_output *out) {
    (void)out;
    return (size_t)e->cfg.num_classes * sizeof(float);
}

static const char *features_check(const vit_engine *e, const void *caller, vit_output *out, int arg[2]) {
    const vit_feature_spec *spec = (const vit_feature_spec *)caller;
    if (!spec) return "%s: the feature spec is required";
    arg[0] = spec->kind;
    if (spec->kind != VIT_FEAT_CLS && spec->kind != VIT_FEAT_MEAN && spec->kind != VIT_FEAT_TOKENS && spec->kind != VIT_FEAT_HEAD) return "%s: unknown feature kind %d";
    arg[0] = spec->l2_normalize;
    if (spec->l2_normalize != 0 && spec->l2_normalize != 1) return "%s: l2_normalize must be 0 or 1 (got %d)";
    if (spec->l2_normalize && spec->kind == VIT_FEAT_TOKENS) return "%s: l2_normalize applies to the CLS, MEAN and HEAD rows, not to TOKENS";
    if (spec->kind == VIT_FEAT_MEAN && e->patches < 1) return "%s: MEAN needs at least one patch token";
    out->spec.kind = spec->kind; out->spec.l2_normalize = spec->l2_normalize;
    return NULL;
}
static size_t features_row_bytes(const vit_engine *e, const vit_output *out) {
    if (out->spec.kind == VIT_FEAT_HEAD) return probs_row_bytes(e, out);
    return (out->spec.kind == VIT_FEAT_TOKENS ? (size_t)e->tokens : 1) * (size_t)e->cfg.embed_dim * sizeof(float);
}

static const char *attention_check(const vit_engine *e, const void *caller, vit_output *out, int arg[2]) {
    const vit_attention_spec *spec = (const vit_attention_spec *)caller;
    (void)e;
    if (!spec) return "%s: the attention spec is required";
    arg[0] = spec->kind;
    if (spec->kind != VIT_ATTN_HEADS && spec->kind != VIT_ATTN_HEAD_MEAN) return "%s: unknown attention kind %d";
    arg[0] = spec->reserved;
    if (spec->reserved != 0) return "%s: vit_attention_spec.reserved must be 0 (got %d)";
    out->attn_kind = spec->kind;
    return NULL;
}
static size_t attention_row_bytes(const vit_engine *e, const vit_output *out) {
    return (out->attn_kind == VIT_ATTN_HEADS ? (size_t)e->cfg.num_heads : 1) * (size_t)e->tokens * sizeof(float);
}
static int attention_rows_only(const vit_engine *e, const vit_output *out) { /* Q of the class rows, K of every token (qkv_only) */
    (void)e; (void)out;
    return 1;
}

static const char *intermediate_check(const vit_engine *e, const void *caller, vit_output *out, int arg[2]) {
    const vit_intermediate_spec *spec = (const vit_intermediate_spec *)caller;
    if (!spec) return "%s: the intermediate spec is required";
    arg[0] = spec->kind;
    if (spec->kind != VIT_TAP_CLS && spec->kind != VIT_TAP_TOKENS && spec->kind != VIT_TAP_PATCHES && spec->kind != VIT_TAP_MAP)
        return "%s: unknown intermediate kind %d";
    arg[0] = spec->norm;
    if (spec->norm != 0 && spec->norm != 1) return "%s: norm must be 0 or 1 (got %d)";
    arg[0] = spec->num_layers; arg[1] = VIT_MAX_TAPS;
    if (spec->num_layers < 1 || spec->num_layers > VIT_MAX_TAPS) return "%s: num_layers = %d must be 1..%d";
    arg[0] = spec->reserved;
    if (spec->reserved != 0) return "%s: vit_intermediate_spec.reserved must be 0 (got %d)";
    for (int j = 0; j < spec->num_layers; ++j) {
        arg[0] = j; arg[1] = spec->layers[j];
        if (spec->layers[j] < 0 || spec->layers[j] >= e->cfg.depth) return "%s: layers[%d] = %d is not a layer of the model";
        if (j && spec->layers[j] <= spec->layers[j - 1]) return "%s: layers[%d] = %d is not above the entry before it (strictly increasing)";
    }
    const int g = e->cfg.img_size / VIT_PATCH_SIZE(&e->cfg);
    arg[0] = g; arg[1] = e->patches;
    if (spec->kind == VIT_TAP_MAP && (g < 1 || g * g != e->patches)) return "%s: MAP needs a square grid of patches: (img_size / patch_size = %d)^2 is not the model's %d";
    if (spec->kind == VIT_TAP_PATCHES && e->patches < 1) return "%s: PATCHES needs at least one patch token";
    out->tap.kind = spec->kind; out->tap.norm = spec->norm; out->tap.num_layers = spec->num_layers;
    for (int j = 0; j < spec->num_layers; ++j) out->tap.layers[j] = spec->layers[j]; /* the unused entries stay zero: the graph key compares the whole spec */
    return NULL;
}
static size_t intermediate_row_bytes(const vit_engine *e, const vit_output *out) {
    return (size_t)out->tap.num_layers * tap_block_elems(e, out->tap.kind) * sizeof(float);
}
static int intermediate_rows_only(const vit_engine *e, const vit_output *out) {
    (void)e;
    return out->tap.kind == VIT_TAP_CLS;
}
static int intermediate_last_layer(const vit_engine *e, const vit_output *out) { /* the deepest tap; nothing else */
    (void)e;
    return out->tap.layers[out->tap.num_layers - 1];
}

static const char *topk_check(const vit_engine *e, const void *caller, vit_output *out, int arg[2]) {
    const vit_topk_spec *spec = (const vit_topk_spec *)caller;
    if (!spec) return "%s: the top-k spec is required";
    arg[0] = spec->k; arg[1] = e->cfg.num_classes < VIT_MAX_TOPK ? e->cfg.num_classes : VIT_MAX_TOPK;
    if (spec->k < 1 || spec->k > arg[1]) return "%s: k = %d must be 1..%d (the smaller of VIT_MAX_TOPK and num_classes)";
    arg[0] = spec->score;
    if (spec->score != VIT_SCORE_PROB && spec->score != VIT_SCORE_LOGIT) return "%s: unknown score %d";
    arg[0] = spec->reserved;
    if (spec->reserved != 0) return "%s: vit_topk_spec.reserved must be 0 (got %d)";
    out->topk.k = spec->k; out->topk.score = spec->score;
    return NULL;
}
static size_t topk_row_bytes(const vit_engine *e, const vit_output *out) { /* 2k 32-bit words */
    (void)e;
    return 2 * (size_t)out->topk.k * sizeof(int);
}

/* The one fault that is the engine's state, not the caller's argument: make_output knows it by its address. */
static const char NO_DENSE_HEAD[] = "%s before vit_engine_set_dense_head()";
/* The dense spec is resolved against the model too (out_h / out_w: 0 becomes img_size).  The head itself was checked when it was set. */
static const char *dense_check(const vit_engine *e, const void *caller, vit_output *out, int arg[2]) {
    const vit_dense_spec *spec = (const vit_dense_spec *)caller;
    vit_dense_spec *res = &out->dense;
    if (!spec) return "%s: the dense spec is required";
    if (!e->dense.spec.num_layers) return NO_DENSE_HEAD;
    arg[0] = spec->kind;
    if (spec->kind != VIT_DENSE_LABELS && spec->kind != VIT_DENSE_GRID) return "%s: unknown dense kind %d";
    arg[0] = spec->reserved;
    if (spec->reserved != 0) return "%s: vit_dense_spec.reserved must be 0 (got %d)";
    res->kind = spec->kind;
    arg[0] = spec->out_h; arg[1] = spec->out_w;
    if (spec->kind == VIT_DENSE_GRID) return spec->out_h || spec->out_w ? "%s: GRID takes no output size (out_h = %d, out_w = %d must be 0)" : NULL;
    res->out_h = spec->out_h ? spec->out_h : e->cfg.img_size;
    res->out_w = spec->out_w ? spec->out_w : e->cfg.img_size;
    if (res->out_h < 1 || res->out_h > 4096 || res->out_w < 1 || res->out_w > 4096)
        return "%s: out_h = %d and out_w = %d must be 1..4096 each (0 = img_size, which must then be in that range)";
    return NULL;
}
/* labels are a byte per pixel, the grid classes * P floats: the one kind whose row is not a whole number of floats */
static size_t dense_row_bytes(const vit_engine *e, const vit_output *out) {
    if (out->dense.kind == VIT_DENSE_LABELS) return (size_t)out->dense.out_h * (size_t)out->dense.out_w;
    return (size_t)e->dense.spec.num_classes * (size_t)e->patches * sizeof(float);
}
static int dense_last_layer(const vit_engine *e, const vit_output *out) { /* the deepest layer of the head */
    (void)out;
    return e->dense.spec.layers[e->dense.spec.num_layers - 1];
}

static const vit_out_kind OUT_KINDS[VIT_OUT_KINDS] = {
    [VIT_OUT_PROBS] = {.row_bytes = probs_row_bytes, .class_rows_only = head_or_class_rows_only, .after_layer = stage_head_tap,
                       .finish = stage_head_or_features},
    [VIT_OUT_FEATURES] = {.check = features_check, .row_bytes = features_row_bytes, .class_rows_only = head_or_class_rows_only,
                          .after_layer = stage_head_tap, .finish = stage_head_or_features},
    [VIT_OUT_ATTENTION] = {.check = attention_check, .row_bytes = attention_row_bytes, .class_rows_only = attention_rows_only,
                           .finish = stage_cls_attention, .qkv_only = 1},
    [VIT_OUT_INTERMEDIATE] = {.check = intermediate_check, .row_bytes = intermediate_row_bytes, .class_rows_only = intermediate_rows_only,
                              .last_layer = intermediate_last_layer, .after_layer = stage_tap},
    [VIT_OUT_TOPK] = {.check = topk_check, .row_bytes = topk_row_bytes, .class_rows_only = head_or_class_rows_only,
                      .after_layer = stage_head_tap, .finish = stage_head_or_features},
    /* no class_rows_only: the patch rows of every tapped layer */
    [VIT_OUT_DENSE] = {.check = dense_check, .row_bytes = dense_row_bytes, .last_layer = dense_last_layer, .after_layer = stage_dense_tap,
                       .finish = stage_dense_out},
};

/* The output of a call: *out zeroed in full (the graph key compares it bytewise), then what the kind's check makes of the caller's
 * spec.  NULL, or the fault as a format for (who, arg[0], arg[1]). */
static const char *output_fault(const vit_engine *e, int kind, const void *spec, vit_output *out, int arg[2]) {
    memset(out, 0, sizeof(*out));
    out->kind = kind;
    arg[0] = arg[1] = 0;
    return OUT_KINDS[kind].check ? OUT_KINDS[kind].check(e, spec, out, arg) : NULL;
}
static int make_output(vit_engine *e, const char *who, int kind, const void *spec, float *dst, int *label, float *prob, vit_output *out) {
    int arg[2];
    const char *fault = output_fault(e, kind, spec, out, arg);
    if (fault) return fail(e, fault == NO_DENSE_HEAD ? VIT_ERR_STATE : VIT_ERR_ARG, fault, who, arg[0], arg[1]);
    out->dst = dst; out->label = label; out->prob = prob;
    return VIT_OK;
}
static size_t out_row_bytes(const vit_engine *e, const vit_output *out) { return OUT_KINDS[out->kind].row_bytes(e, out); }

/* The public row widths: the kind's check, then its measure -- 0 for no engine and for a spec the calls would refuse (a dense spec
 * with no dense head set among them). */
static size_t spec_row_bytes(const vit_engine *e, int kind, const void *spec) {
    vit_output out;
    int arg[2];
    return e && !output_fault(e, kind, spec, &out, arg) ? out_row_bytes(e, &out) : 0;
}
size_t vit_engine_feature_row_elems(const vit_engine *e, const vit_feature_spec *spec) {
    return spec_row_bytes(e, VIT_OUT_FEATURES, spec) / sizeof(float);
}
size_t vit_engine_attention_row_elems(const vit_engine *e, const vit_attention_spec *spec) {
    return spec_row_bytes(e, VIT_OUT_ATTENTION, spec) / sizeof(float);
}
size_t vit_engine_intermediate_row_elems(const vit_engine *e, const vit_intermediate_spec *spec) {
    return spec_row_bytes(e, VIT_OUT_INTERMEDIATE, spec) / sizeof(float);
}
size_t vit_engine_topk_row_elems(const vit_engine *e, const vit_topk_spec *spec) {
    return spec_row_bytes(e, VIT_OUT_TOPK, spec) / sizeof(float);
}
size_t vit_engine_dense_row_bytes(const vit_engine *e, const vit_dense_spec *spec) {
    return spec_row_bytes(e, VIT_OUT_DENSE, spec);
}

/* The chunk's context for nb images written as `out` says: dimensions, whether the last layer is pruned, and the lanes -- their
 * images, streams and rows of the activation buffers.  Launches nothing. */
static void chunk_setup(vit_engine *e, vithip_stream_t s, int nb, const vit_output *out, chunk_ctx *c) {
    const vit_config *cfg = &e->cfg;
    c->e = e;
    c->T = e->tokens; c->D = cfg->embed_dim; c->H = VIT_HIDDEN_DIM(cfg); c->H1 = VIT_FC1_ROWS(cfg); c->NC = cfg->num_classes;
    c->L = e->opt.lanes > VIT_MAX_LANES ? VIT_MAX_LANES : e->opt.lanes;
    if (c->L < 1 || nb < 2 * c->L) c->L = 1;
    const vit_out_kind *k = &OUT_KINDS[out->kind];
    c->pruned = e->opt.prune_last_layer && c->T <= 224 && k->class_rows_only && k->class_rows_only(e, out);
    c->qkv_only = k->qkv_only;
    c->row = k->row_bytes(e, out);
    const int bf16 = e->opt.dtype == VIT_DTYPE_BF16;
    const size_t B = (size_t)e->opt.max_batch, T = (size_t)c->T, D = (size_t)c->D, H1 = (size_t)c->H1;
    const size_t esz = c->esz = bf16 ? sizeof(unsigned short) : sizeof(float);
    /* Where the LayerNorm fold keeps its row statistics.  fp32 engines: ln_rows32 = the pairs of max_batch * T token rows, then
     * of max_batch class rows; ln_part32 = the partial sums, [D / 64][rows][2] per lane.  bf16 engines: the idle halves of the y
     * and qkv allocations, which bf16 activations only half fill -- the bf16 copy of x in y's; the partial sums
     * ([vithip_ln_strips(D)][rows][2] per lane), then the token and the class pairs, in qkv's. */
    float *pairs = e->ln_rows32, *part = e->ln_part32;
    size_t strips = D / 64;
    unsigned short *x16 = NULL;
    if (bf16) {
        x16 = (unsigned short *)e->y + B * T * D;
        strips = (size_t)vithip_ln_strips((int)D);
        part = (float *)((unsigned short *)e->qkv + B * T * 3 * D);
        pairs = part + strips * B * T * 2;
    }
    for (int j = 0; j < c->L; ++j) {
        vit_lane *ln = &c->lane[j];
        memset(ln, 0, sizeof(*ln));
        ln->off = (int)((long)nb * j / c->L);
        ln->n = (int)((long)nb * (j + 1) / c->L) - ln->off;
        ln->s = j == 0 ? s : e->aux_stream[j - 1];
        const size_t row0 = (size_t)ln->off * T;
        ln->x = e->x + row0 * D;
        ln->y = at(e->y, row0 * D, esz); ln->qkv = at(e->qkv, row0 * 3 * D, esz); ln->h = at(e->hbuf, row0 * H1, esz);
        if (e->fold) {
            ln->xa = bf16 ? (void *)(x16 + row0 * D) : (void *)ln->x;
            ln->tok_pairs = pairs + row0 * 2;
            ln->cls_pairs = pairs + (B * T + (size_t)ln->off) * 2;
            ln->partials = part + row0 * strips * 2;
        }
    }
}

/* The LayerNorm in front of layer 0 (CLIP's ln_pre; vit_engine_set_pre_norm): each lane normalises its n * T rows of the fp32
 * residual stream x IN PLACE (y == x, ldy == ldx: the stated contract of vithip_layernorm_f32_eps), with the engine's epsilon.  x is
 * fp32 on both engine dtypes.  Layer 0 then proceeds as ever: with the fold its statistics pass runs on these rows (stats_ready is
 * false at the start of a chunk) and, on bf16 engines, writes their bf16 copy. */
static int stage_pre_norm(chunk_ctx *c) {
    vit_engine *e = c->e;
    for (int j = 0; j < c->L; ++j) {
        const vit_lane *ln = &c->lane[j];
        HIP_TRY(e, stage_begin(e, ln->s, VIT_STAGE_LN));
        HIP_TRY(e, vithip_layernorm_f32_eps(ln->s, ln->x, (size_t)c->D, ln->x, (size_t)c->D, e->pre_g, e->pre_b, ln->n * c->T, c->D, e->ln_eps));
        HIP_TRY(e, stage_end(e, ln->s));
    }
    return VIT_OK;
}

/* d_images: the chunk's first image, of the kind `in` says; f32_stage: where 8-bit images are normalised to (max_batch images);
 * out: what to write, at the chunk's first row */
static int forward_chunk(vit_engine *e, vithip_stream_t s, const void *d_images, const vit_input *in, float *f32_stage, int nb,
                         const vit_output *out) {
    const vit_out_kind *k = &OUT_KINDS[out->kind];
    chunk_ctx ctx, *c = &ctx;
    chunk_setup(e, s, nb, out, c);

    if (c->L > 1) { /* fork: the other lanes start after everything already queued on s */
        HIP_TRY(e, vithip_event_record(e->ev_fork, s));
        for (int j = 1; j < c->L; ++j) HIP_TRY(e, vithip_stream_wait_event(c->lane[j].s, e->ev_fork));
    }
    RUN(stage_embed(c, d_images, in, f32_stage));
    if (e->pre_g) RUN(stage_pre_norm(c));
    /* the one walk: the layers up to the deepest the kind needs, what it runs behind each, then its last stage (OUT_KINDS) */
    for (int l = 0, last = k->last_layer ? k->last_layer(e, out) : e->cfg.depth - 1; l <= last; ++l) {
        RUN(encoder_layer(c, l));
        if (k->after_layer) RUN(k->after_layer(c, out, l));
    }
    if (k->finish) RUN(k->finish(c, out));
    for (int j = 1; j < c->L; ++j) { /* join */
        HIP_TRY(e, vithip_event_record(e->ev_join[j - 1], c->lane[j].s));
        HIP_TRY(e, vithip_stream_wait_event(s, e->ev_join[j - 1]));
    }
    e->last_rows = runs_head(out) ? nb : 0; /* rows of e->logits the chunk wrote (vit_engine_read_logits) */
    return VIT_OK;
}
#undef RUN

/* Images per forward_chunk call: the workspace holds max_batch, and no lane may exceed lane_cap (see vit_engine_create). */
static int chunk_limit(const vit_engine *e) {
    int lanes = e->opt.lanes < 1 ? 1 : (e->opt.lanes > VIT_MAX_LANES ? VIT_MAX_LANES : e->opt.lanes);
    if (e->opt.dtype == VIT_DTYPE_BF16) return e->opt.max_batch; /* bf16 kernels rebase their descriptors per tile */
    const long cap = (long)e->lane_cap * lanes;
    return cap < e->opt.max_batch ? (int)cap : e->opt.max_batch;
}

/* The 8-bit input of a call (vit_engine_forward_device_u8 / _host_u8), its normalisation checked. */
static int input_u8(vit_engine *e, const char *who, const float *mean, const float *std, vit_input *in) {
    memset(in, 0, sizeof(*in));
    in->kind = VIT_IN_U8;
    /* the 8-bit and decoded-image kernels write 16 bytes of a pixel row at a time; an engine with img_size % 4 == 2 takes fp32 input only */
    if (e->cfg.img_size % 4)
        return fail(e, VIT_ERR_ARG, "%s: 8-bit and decoded-image input need img_size %% 4 == 0 (img_size = %d): pass fp32 images", who,
                    e->cfg.img_size);
    if (!mean || !std) return fail(e, VIT_ERR_ARG, "%s: mean and std are required", who);
    if (e->cfg.in_chans > VIT_MAX_U8_CHANS)
        return fail(e, VIT_ERR_ARG, "%s: 8-bit input takes at most %d channels (in_chans = %d)", who, VIT_MAX_U8_CHANS, e->cfg.in_chans);
    for (int c = 0; c < e->cfg.in_chans; ++c) {
        if (!isfinite(mean[c]) || !isfinite(std[c]) || std[c] == 0.0f)
            return fail(e, VIT_ERR_ARG, "%s: channel %d: mean (%g) and std (%g) must be finite, std non-zero", who, c, mean[c], std[c]);
        in->mean[c] = mean[c];
        in->std[c] = std[c];
    }
    return VIT_OK;
}

/* The input of an _images call: decoded 8-bit images of any size and the transform's parameters, everything checked that the kernel
 * launcher would refuse -- every record, before the call enqueues anything. */
static int input_images(vit_engine *e, const char *who, const vit_image_u8 *images, int n, const vit_preproc *pp, vit_input *in) {
    if (!pp) return fail(e, VIT_ERR_ARG, "%s: the preprocessing parameters are required", who);
    const int rc = input_u8(e, who, pp->mean, pp->std, in);
    if (rc) return rc;
    in->kind = VIT_IN_IMAGES;
    in->resize_shorter = pp->resize_shorter;
    in->resize_filter = e->resize_filter;
    if (pp->resize_shorter < e->cfg.img_size || pp->resize_shorter > 4096)
        return fail(e, VIT_ERR_ARG, "%s: resize_shorter = %d must be img_size = %d .. 4096 (a smaller image would have to be padded)", who,
                    pp->resize_shorter, e->cfg.img_size);
    const int bad = vithip_images_u8_resize_crop_check_filter((const vithip_image_u8 *)images, n, e->cfg.img_size, e->cfg.in_chans,
                                                              pp->resize_shorter, in->resize_filter);
    if (bad > 0)
        return fail(e, VIT_ERR_ARG, "%s: image %d (pixels %p, %d x %d): pixels must not be NULL, height and width 1..16384, the shorter side "
                    "at most 64 x resize_shorter", who, bad - 1, (const void *)images[bad - 1].pixels, images[bad - 1].height, images[bad - 1].width);
    if (bad) return fail(e, VIT_ERR_ARG, "%s: unsupported geometry (img_size %d, in_chans %d, resize_shorter %d)", who, e->cfg.img_size,
                         e->cfg.in_chans, pp->resize_shorter);
    return VIT_OK;
}

/* An 8-bit device-path call normalises into in_stage[0] and uses it until s gets past its kernels: the next host-pointer call's
 * uploads wait for that (ev_in_stage). */
static int in_stage_taken(vit_engine *e, const vit_input *in, vithip_stream_t s) {
    if (in->kind == VIT_IN_F32) return VIT_OK;
    HIP_TRY(e, vithip_event_record(e->ev_in_stage, s));
    e->in_stage_pending = 1;
    return VIT_OK;
}

/* The device-resident forward of every input kind: chunks of at most chunk_limit() images, the use_graph cache.  8-bit chunks
 * are normalised into in_stage[0]; chunks run one after the other on s (a chunk's lanes fork behind the previous chunk's join).
 * Decoded images (d_images = the caller's records, a HOST array) run eagerly and leave a captured graph alone: its key would have
 * to hold every pointer and size. */
static int forward_device_in(vit_engine *e, const void *d_images, const vit_input *in, int n, const vit_output *out, void *stream) {
    if (!e->weights_loaded) return fail(e, VIT_ERR_STATE, "forward before vit_engine_load_weights()");
    vithip_stream_t s = stream ? (vithip_stream_t)stream : e->stream;
    /* bytes from one image of d_images to the next: fp32 or 8-bit pixels, or a record */
    const size_t img = in->kind == VIT_IN_IMAGES ? sizeof(vithip_image_u8)
                                                 : (size_t)e->cfg.in_chans * e->cfg.img_size * e->cfg.img_size * (in->kind == VIT_IN_U8 ? 1 : sizeof(float));
    const size_t row = out_row_bytes(e, out);
    HIP_TRY(e, vithip_set_device(e->opt.device)); /* the current device is per host thread: several engines may share a process */
    if (in->kind != VIT_IN_F32 && !e->ev_in_stage) HIP_TRY(e, vithip_event_create(&e->ev_in_stage));
    const int chunk = chunk_limit(e);
    const int graphable = e->opt.use_graph && !e->opt.profile && e->opt.lanes == 1 && s != NULL && in->kind != VIT_IN_IMAGES;
    /* the key holds the input kind, the normalisation and the output descriptor too: all are baked into the captured launches */
    if (graphable && e->graph && e->g_n == n && e->g_images == d_images && !memcmp(&e->g_in, in, sizeof(*in)) &&
        !memcmp(&e->g_out, out, sizeof(*out))) {
        HIP_TRY(e, vithip_graph_launch(e->graph, s));
        return in_stage_taken(e, in, s);
    }
    if (graphable) {
        if (e->graph) { vithip_graph_destroy(e->graph); e->graph = NULL; }
        HIP_TRY(e, vithip_graph_begin(s));
    }
    for (int done = 0; done < n; done += chunk) {
        const int nb = n - done < chunk ? n - done : chunk;
        vit_output o = *out;
        o.dst = (float *)((char *)o.dst + (size_t)done * row);
        if (o.label) o.label += done;
        if (o.prob) o.prob += done;
        int rc = forward_chunk(e, s, (const char *)d_images + (size_t)done * img, in, e->in_stage[0], nb, &o);
        if (rc) {
            if (graphable) { /* never leave the caller's stream in capture mode: end the capture, discard what it recorded */
                vithip_graph_t g = NULL;
                if (vithip_graph_end(s, &g) == 0 && g) vithip_graph_destroy(g);
            }
            return rc;
        }
        if (e->opt.profile) e->pending_images += nb;
        /* read the brackets back lazily (it needs an event sync): only when the pool runs low, that is when the next chunk (at
         * most 12 brackets per layer and lane, 16 around them) might not fit: a depth-40 model takes more than 256 per lane */
        const int chunk_brackets = e->opt.lanes * (12 * e->cfg.depth + 16);
        if (e->opt.profile && e->ev_used > MAX_EVENTS - (chunk_brackets > 256 ? chunk_brackets : 256) && (rc = collect_profile(e))) return rc;
    }
    if (graphable) { /* nothing ran yet: the launches above were recorded; instantiate and run them */
        HIP_TRY(e, vithip_graph_end(s, &e->graph));
        e->g_n = n; e->g_images = d_images; e->g_in = *in; e->g_out = *out;
        HIP_TRY(e, vithip_graph_launch(e->graph, s));
    }
    return in_stage_taken(e, in, s);
}

int vit_engine_sync(vit_engine *e) {
    if (!e) return VIT_ERR_ARG;
    HIP_TRY(e, vithip_stream_sync(e->stream));
    return VIT_OK;
}

/* Host-pointer surface helpers.  The reference's ImageData keeps every image in its own malloc (Network.c:66-93), so a
 * piece has to be gathered into pinned memory before it can be uploaded: one memcpy thread manages ~10 GB/s, which made
 * the gather of the FIRST piece (nothing to overlap it with) 15 ms of a 512-image call.  The gather runs on a few OpenMP
 * threads and a piece goes up in sub-pieces of 64 images, so the H2D copy of one sub-piece overlaps the gather of the
 * next. */
#define GATHER_THREADS_MAX 16
#define SUB_PIECE 64
#define SUB_PIECE_FIRST 16 /* the call's first piece goes up in sub-pieces of 16: its upload starts after 10 MB of gathering */
static int gather_threads(void) {
    int n = omp_get_num_procs();
    return n < 1 ? 1 : (n > GATHER_THREADS_MAX ? GATHER_THREADS_MAX : n);
}
/* The caller's images of a host-pointer call are the input kind plus one pointer: an array of pointers to fp32 [C][S][S] or to 8-bit
 * [S][S][C] images, or the records of decoded 8-bit images of any size. */
static const void *host_image(int kind, const void *images, int i) {
    switch (kind) {
    case VIT_IN_IMAGES: return ((const vit_image_u8 *)images)[i].pixels;
    case VIT_IN_U8: return ((const unsigned char *const *)images)[i];
    default: return ((const float *const *)images)[i];
    }
}
/* its bytes as the caller holds it, and in a staging slot: a piece's images lie back to back, each start rounded up to 16 bytes
 * (fp32 images fill whole 16 bytes anyway: img_size is even; 8-bit ones too: they need img_size % 4 == 0, input_u8) */
static size_t host_image_bytes(const vit_engine *e, int kind, const void *images, int i) {
    const size_t C = (size_t)e->cfg.in_chans, S = (size_t)e->cfg.img_size;
    if (kind != VIT_IN_IMAGES) return C * S * S * (kind == VIT_IN_U8 ? 1 : sizeof(float));
    const vit_image_u8 *im = (const vit_image_u8 *)images + i;
    return (size_t)im->height * (size_t)im->width * C;
}
static size_t image_slot_bytes(const vit_engine *e, int kind, const void *images, int i) {
    return (host_image_bytes(e, kind, images, i) + 15) & ~(size_t)15;
}
static size_t image_slot_cap(const vit_engine *e) { /* what pin_in[slot] holds: max_batch fp32 images */
    return (size_t)e->opt.max_batch * e->cfg.in_chans * e->cfg.img_size * e->cfg.img_size * sizeof(float);
}
/* img_off[0..count] = where the images first .. first + count - 1 of a piece lie in its slot, and where they end */
static void image_offsets(vit_engine *e, int kind, const void *images, int first, int count) {
    e->img_off[0] = 0;
    for (int i = 0; i < count; ++i) e->img_off[i + 1] = e->img_off[i] + image_slot_bytes(e, kind, images, first + i);
}
/* gather a piece into pin_in[slot] at its images' offsets and upload it to dst (in_stage[slot], in8_stage[slot] or img_stage[slot])
 * in sub-pieces of `sub` images */
static int stage_piece(vit_engine *e, int slot, void *dst, int kind, const void *images, int first, int count, int sub) {
    const int nt = gather_threads();
    char *pin = (char *)e->pin_in[slot];
    image_offsets(e, kind, images, first, count);
    for (int s0 = 0; s0 < count; s0 += sub) {
        const int c = count - s0 < sub ? count - s0 : sub;
#pragma omp parallel for num_threads(nt) schedule(static) if (c >= 4)
        for (int i = s0; i < s0 + c; ++i)
            memcpy(pin + e->img_off[i], host_image(kind, images, first + i), host_image_bytes(e, kind, images, first + i));
        HIP_TRY(e, vithip_memcpy_h2d((char *)dst + e->img_off[s0], pin + e->img_off[s0], e->img_off[s0 + c] - e->img_off[s0], e->copy_stream));
    }
    HIP_TRY(e, vithip_event_record(e->ev_h2d[slot], e->copy_stream));
    return VIT_OK;
}
/* the records of a staged piece of decoded images, as the kernel reads them: the images' sizes, their pixels inside img_stage[slot] */
static const vithip_image_u8 *piece_records(vit_engine *e, int slot, const vit_image_u8 *images, int first, int count) {
    image_offsets(e, VIT_IN_IMAGES, images, first, count);
    for (int i = 0; i < count; ++i) {
        e->img_recs[i].pixels = e->img_stage[slot] + e->img_off[i];
        e->img_recs[i].height = images[first + i].height;
        e->img_recs[i].width = images[first + i].width;
    }
    return e->img_recs;
}
/* wait for the piece in slot b and hand its rows back: images first .. first + count - 1 */
static int scatter_piece(vit_engine *e, int b, float *const *rows, int first, int count, size_t row) { /* row: bytes */
    HIP_TRY(e, vithip_event_sync(e->ev_done[b]));
    for (int i = 0; i < count; ++i) memcpy(rows[first + i], (const char *)e->pin_out[b] + (size_t)i * row, row);
    return VIT_OK;
}

/* The pieces of a host-pointer call: piece_lo[0..np] = their first images (piece_lo[np] = n).  The first piece has at most first_n
 * images, every other at most chunk; a piece of decoded images also ends where the next image's bytes would overflow the slot. */
static int cut_pieces(vit_engine *e, const char *who, int kind, const void *images, int n, int first_n, int chunk, int *np_out) {
    if (n + 1 > e->piece_cap) {
        int *p = (int *)realloc(e->piece_lo, ((size_t)n + 1) * sizeof(int));
        if (!p) return fail(e, VIT_ERR_NOMEM, "out of host memory");
        e->piece_lo = p; e->piece_cap = n + 1;
    }
    const size_t cap = image_slot_cap(e);
    int np = 0;
    e->piece_lo[0] = 0;
    for (int i = 0; i < n;) {
        const int limit = np == 0 ? first_n : chunk;
        int cnt = n - i < limit ? n - i : limit;
        if (kind == VIT_IN_IMAGES) {
            const vit_image_u8 *im = (const vit_image_u8 *)images + i;
            size_t bytes = 0;
            int fit = 0;
            while (fit < cnt && bytes + image_slot_bytes(e, kind, images, i + fit) <= cap) bytes += image_slot_bytes(e, kind, images, i + fit++);
            if (!fit)
                return fail(e, VIT_ERR_ARG, "%s: image %d (%d x %d, %zu bytes) does not fit the staging of max_batch = %d fp32 images (%zu bytes)",
                            who, i, im->height, im->width, image_slot_bytes(e, kind, images, i), e->opt.max_batch, cap);
            cnt = fit;
        }
        i += cnt;
        e->piece_lo[++np] = i;
    }
    *np_out = np;
    return VIT_OK;
}

/* The output staging holds max_batch rows of out_row_cap bytes: classes floats at first, grown to the widest feature, attention or intermediate row a
 * host call has asked for (TOKENS: tokens * embed_dim; HEADS: heads * tokens; top-k records: 2k words, wider than a head of fewer classes).  Growing waits for everything in flight, frees both slots and allocates them again; if
 * that fails the call fails with VIT_ERR_NOMEM and the staging is back at its classes-sized start. */
static int alloc_out_stage(vit_engine *e, size_t bytes) { /* both slots, freed first; a HIP error code, with both slots freed again */
    int rc = 0;
    e->out_row_cap = 0;
    for (int pass = 0; pass < 2; ++pass) {
        for (int b = 0; b < 2; ++b) {
            vithip_free(e->out_stage[b]); e->out_stage[b] = NULL;
            if (e->pin_out[b]) vithip_host_free(e->pin_out[b]);
            e->pin_out[b] = NULL;
        }
        if (pass == 1) break; /* the second pass only cleans up after a failure */
        for (int b = 0; b < 2 && !rc; ++b) {
            rc = vithip_malloc((void **)&e->out_stage[b], bytes);
            if (!rc) rc = vithip_host_alloc((void **)&e->pin_out[b], bytes);
        }
        if (!rc) break;
    }
    return rc;
}
static int ensure_out_stage(vit_engine *e, size_t row) { /* row: bytes */
    if (row <= e->out_row_cap) return VIT_OK;
    const size_t bytes = (size_t)e->opt.max_batch * row;
    HIP_TRY(e, vithip_device_sync());
    int rc = alloc_out_stage(e, bytes);
    if (rc) {
        /* the wide rows do not fit: put the classes-sized staging back, so that the forwards go on as before this call */
        const size_t own = (size_t)e->cfg.num_classes * sizeof(float);
        e->out_row_cap = alloc_out_stage(e, (size_t)e->opt.max_batch * own) ? 0 : own;
        return fail(e, VIT_ERR_NOMEM, "no memory for 2 x %zu bytes of pinned and of device output staging (HIP error %d: %s)", bytes,
                    rc, vithip_error_string(rc));
    }
    e->out_row_cap = row;
    return VIT_OK;
}

/* The host-pointer forward of every input kind.  8-bit pieces are gathered into pin_in[slot] as bytes, uploaded into
 * in8_stage[slot] and normalised into in_stage[slot] on the compute stream (stage_embed): the copy stream writes nothing else, so
 * the ev_h2d / ev_done ordering below covers them as it covers the fp32 pieces.  Decoded images of any size go the same way through
 * img_stage[slot], in pieces that the slot's bytes bound as well as the image count (cut_pieces). */
/* out: the kind of output (its pointers unused: the rows go through out_stage / pin_out into rows[i]) */
static int forward_host_in(vit_engine *e, const char *who, const void *images, const vit_input *in, int n, const vit_output *out,
                           float *const *rows) {
    if (!e->weights_loaded) return fail(e, VIT_ERR_STATE, "forward before vit_engine_load_weights()");
    const size_t img = (size_t)e->cfg.in_chans * e->cfg.img_size * e->cfg.img_size;
    const int kind = in->kind, decoded = kind == VIT_IN_IMAGES;
    const size_t row = out_row_bytes(e, out); /* bytes per image of the scatter stage */
    for (int i = 0; i < n; ++i)
        if (!host_image(kind, images, i) || !rows[i]) return fail(e, VIT_ERR_ARG, "%s: image or output row %d is NULL", who, i);
    const int chunk = chunk_limit(e);
    /* Round 5: what the first piece has to do is cover, with its compute, the gather + upload of the piece behind it -- and no
     * more than that, because a small piece computes badly (ViT-B/16 fp32, device-resident: 8 images run at 56 % of the 256-image
     * rate per image, 40 at 86 %, 64 at 90 %, 192 at 99.5 %: tools/batch_time_sweep.py).  Measured at 256 images
     * (tools/host_path_sweep.py, ms per call, device-resident 64.9): first piece 8: 69.3 (the GPU waits for the second piece),
     * 12: 67.7, 16: 68.7, 40: 68.0, 64: 68.8 (the round-4 choice), 128: 71.2 -- on a box whose host gathers at ~40 GB/s.  On
     * one that gathers at ~16 GB/s the 12-image piece left the GPU idle for 4 ms (71.2 ms per call): the choice is 5 n / 32
     * (40 of 256, at most 64), whose compute covers the next piece's staging down to ~11 GB/s.  The bf16 engines compute an
     * image in a tenth of the time: they keep 64. */
    int first_n = n;
    if (e->opt.host_first_piece > 0) first_n = e->opt.host_first_piece;
    else if (e->opt.dtype == VIT_DTYPE_F32 && n >= 128) {
        first_n = (5 * n / 32 + 2) & ~3;
        if (first_n > 64) first_n = 64;
    } else if (n >= 128) first_n = 64;
    else if (n >= 64) first_n = (n + 1) / 2;
    if (first_n > chunk) first_n = chunk;
    if (first_n > n) first_n = n;
    int np = 0;
    {
        const int rc = cut_pieces(e, who, kind, images, n, first_n, chunk, &np); /* before anything is enqueued: it may refuse an image */
        if (rc) return rc;
    }
    const int *lo = e->piece_lo; /* piece k = images lo[k] .. lo[k + 1] - 1 */
    HIP_TRY(e, vithip_set_device(e->opt.device));
    {
        const int rc = ensure_out_stage(e, row);
        if (rc) return rc;
    }
    for (int b = 0; b < 2 && kind == VIT_IN_U8; ++b)
        if (!e->in8_stage[b]) HIP_TRY(e, vithip_malloc((void **)&e->in8_stage[b], (size_t)e->opt.max_batch * img));
    for (int b = 0; b < 2 && decoded; ++b)
        if (!e->img_stage[b]) {
            const int rc = vithip_malloc((void **)&e->img_stage[b], image_slot_cap(e));
            if (rc) {
                e->img_stage[b] = NULL;
                return fail(e, VIT_ERR_NOMEM, "no memory for %zu bytes of device staging for decoded images (HIP error %d: %s)", image_slot_cap(e),
                            rc, vithip_error_string(rc));
            }
        }
    if (e->in_stage_pending) { /* an 8-bit device-path call may still read in_stage[0] */
        HIP_TRY(e, vithip_stream_wait_event(e->copy_stream, e->ev_in_stage));
        e->in_stage_pending = 0;
    }
    void *up[2]; /* where the pieces are uploaded to */
    for (int b = 0; b < 2; ++b)
        up[b] = decoded ? (void *)e->img_stage[b] : kind == VIT_IN_U8 ? (void *)e->in8_stage[b] : (void *)e->in_stage[b];
    /*
     * Pieces of up to max_batch images flow through two staging slots: while the GPU computes piece i,
     * the host gathers the separately allocated images of piece i+1 into pinned memory and the copy
     * stream uploads them; the results of piece i-1 are scattered to the caller's rows meanwhile.
     * Nothing overlaps the gather + upload of the FIRST piece, so it is a small one, uploaded in sub-pieces of 16 images (the copy
     * of one overlaps the gather of the next), and the rest arrives behind its compute in pieces as large as the workspace allows
     * (large pieces keep the GEMMs' tile walks long).  Rows are bit-identical whatever the cut.
     */
    /* stage piece 0 */
    {
        const int rc0 = stage_piece(e, 0, up[0], kind, images, 0, lo[1], np > 1 ? SUB_PIECE_FIRST : SUB_PIECE);
        if (rc0) return rc0;
    }
    for (int k = 0; k < np; ++k) {
        const int b = k & 1, nb = lo[k + 1] - lo[k];
        HIP_TRY(e, vithip_stream_wait_event(e->stream, e->ev_h2d[b]));
        vit_output o = *out;
        o.dst = e->out_stage[b];
        /* decoded images: the kernel reads the piece's records, which point into the slot the piece was uploaded to */
        const void *src = decoded ? (const void *)piece_records(e, b, (const vit_image_u8 *)images, lo[k], nb) : up[b];
        int rc = forward_chunk(e, e->stream, src, in, e->in_stage[b], nb, &o);
        if (rc) return rc;
        HIP_TRY(e, vithip_memcpy_d2h(e->pin_out[b], e->out_stage[b], (size_t)nb * row, e->stream));
        HIP_TRY(e, vithip_event_record(e->ev_done[b], e->stream));
        if (e->opt.profile) e->pending_images += nb;
        /* piece k-1 (slot b^1) is finished by now or soon: hand its rows back */
        if (k >= 1 && (rc = scatter_piece(e, b ^ 1, rows, lo[k - 1], lo[k] - lo[k - 1], row))) return rc;
        /* slot b^1 is free again (its H2D, compute and D2H are complete): refill it */
        if (k + 1 < np && (rc = stage_piece(e, b ^ 1, up[b ^ 1], kind, images, lo[k + 1], lo[k + 2] - lo[k + 1], SUB_PIECE))) return rc;
    }
    {
        const int rc = scatter_piece(e, (np - 1) & 1, rows, lo[np - 1], n - lo[np - 1], row);
        if (rc) return rc;
    }
    if (e->opt.profile) {
        int rc = collect_profile(e);
        if (rc) return rc;
    }
    return VIT_OK;
}

/* One call of the public surface: output kind x input kind x place, with the raw arguments of each as the caller gave them. */
enum { VIT_AT_DEVICE = 0, VIT_AT_HOST = 1 };
typedef struct {
    const char *who;        /* the function's name without vit_engine_, for messages */
    int place;              /* VIT_AT_* */
    int in_kind;            /* VIT_IN_* */
    const void *images;     /* device: fp32 or 8-bit pixels; host: an array of pointers to them; VIT_IN_IMAGES: records (a host array) */
    int n;
    const float *mean, *std; /* VIT_IN_U8 */
    const vit_preproc *pp;  /* VIT_IN_IMAGES */
    int out_kind;           /* VIT_OUT_* */
    const void *spec;       /* vit_feature_spec (VIT_OUT_FEATURES), vit_attention_spec (_ATTENTION), vit_intermediate_spec (_INTERMEDIATE),
                             * vit_topk_spec (_TOPK) or vit_dense_spec (_DENSE) */
    float *dst;             /* VIT_AT_DEVICE: [n][row]; _TOPK: the caller's 32-bit words, carried as the floats they are as wide as; _DENSE:
                             * the caller's rows of bytes, carried untyped */
    float *const *rows;     /* VIT_AT_HOST: a row per image */
    int *label;             /* VIT_AT_DEVICE, VIT_OUT_PROBS: top-1 (may be NULL) */
    float *prob;
    void *stream;           /* VIT_AT_DEVICE */
} vit_call;

/* Every public forward comes through here, so this order decides which message a caller sees: the engine, the pointers and n, the
 * alignment of device 8-bit pixels, the input, the output spec -- and only then, in the place's forward, whether weights are loaded. */
static int run_call(vit_engine *e, const vit_call *c) {
    const int host = c->place == VIT_AT_HOST;
    if (!e) return VIT_ERR_ARG;
    if (!c->images || !(host ? (const void *)c->rows : (const void *)c->dst) || c->n <= 0)
        return fail(e, VIT_ERR_ARG, "%s: bad arguments (n=%d)", c->who, c->n);
    if (!host && c->in_kind == VIT_IN_U8 && ((size_t)c->images & 3)) return fail(e, VIT_ERR_ARG, "%s: d_images must be 4-byte aligned", c->who);
    vit_input in;
    vit_output out;
    int rc = VIT_OK;
    memset(&in, 0, sizeof(in));
    if (c->in_kind == VIT_IN_U8) rc = input_u8(e, c->who, c->mean, c->std, &in);
    else if (c->in_kind == VIT_IN_IMAGES) rc = input_images(e, c->who, (const vit_image_u8 *)c->images, c->n, c->pp, &in);
    if (rc) return rc;
    if ((rc = make_output(e, c->who, c->out_kind, c->spec, c->dst, c->label, c->prob, &out))) return rc;
    return host ? forward_host_in(e, c->who, c->images, &in, c->n, &out, c->rows) : forward_device_in(e, c->images, &in, c->n, &out, c->stream);
}

int vit_engine_forward_device(vit_engine *e, const float *d_images, int n, float *d_probs,
                              int *d_top1_label, float *d_top1_prob, void *stream) {
    return run_call(e, &(vit_call){.who = "forward_device", .place = VIT_AT_DEVICE, .in_kind = VIT_IN_F32, .images = d_images, .n = n,
                                    .out_kind = VIT_OUT_PROBS, .dst = d_probs, .label = d_top1_label, .prob = d_top1_prob,
                                    .stream = stream});
}

int vit_engine_forward_device_u8(vit_engine *e, const unsigned char *d_images, int n, const float *mean, const float *std,
                                 float *d_probs, int *d_top1_label, float *d_top1_prob, void *stream) {
    return run_call(e, &(vit_call){.who = "forward_device_u8", .place = VIT_AT_DEVICE, .in_kind = VIT_IN_U8, .images = d_images, .n = n,
                                    .mean = mean, .std = std, .out_kind = VIT_OUT_PROBS, .dst = d_probs, .label = d_top1_label,
                                    .prob = d_top1_prob, .stream = stream});
}

int vit_engine_forward_device_images(vit_engine *e, const vit_image_u8 *images, int n, const vit_preproc *pp, float *d_probs,
                                     int *d_top1_label, float *d_top1_prob, void *stream) {
    return run_call(e, &(vit_call){.who = "forward_device_images", .place = VIT_AT_DEVICE, .in_kind = VIT_IN_IMAGES, .images = images,
                                    .n = n, .pp = pp, .out_kind = VIT_OUT_PROBS, .dst = d_probs, .label = d_top1_label,
                                    .prob = d_top1_prob, .stream = stream});
}

int vit_engine_features_device(vit_engine *e, const float *d_images, int n, const vit_feature_spec *spec, float *d_out, void *stream) {
    return run_call(e, &(vit_call){.who = "features_device", .place = VIT_AT_DEVICE, .in_kind = VIT_IN_F32, .images = d_images, .n = n,
                                    .out_kind = VIT_OUT_FEATURES, .spec = spec, .dst = d_out, .stream = stream});
}

int vit_engine_features_device_u8(vit_engine *e, const unsigned char *d_images, int n, const float *mean, const float *std,
                                  const vit_feature_spec *spec, float *d_out, void *stream) {
    return run_call(e, &(vit_call){.who = "features_device_u8", .place = VIT_AT_DEVICE, .in_kind = VIT_IN_U8, .images = d_images, .n = n,
                                    .mean = mean, .std = std, .out_kind = VIT_OUT_FEATURES, .spec = spec, .dst = d_out, .stream = stream});
}

int vit_engine_features_device_images(vit_engine *e, const vit_image_u8 *images, int n, const vit_preproc *pp, const vit_feature_spec *spec,
                                      float *d_out, void *stream) {
    return run_call(e, &(vit_call){.who = "features_device_images", .place = VIT_AT_DEVICE, .in_kind = VIT_IN_IMAGES, .images = images,
                                    .n = n, .pp = pp, .out_kind = VIT_OUT_FEATURES, .spec = spec, .dst = d_out, .stream = stream});
}

int vit_engine_cls_attention_device(vit_engine *e, const float *d_images, int n, const vit_attention_spec *spec, float *d_out, void *stream) {
    return run_call(e, &(vit_call){.who = "cls_attention_device", .place = VIT_AT_DEVICE, .in_kind = VIT_IN_F32, .images = d_images,
                                    .n = n, .out_kind = VIT_OUT_ATTENTION, .spec = spec, .dst = d_out, .stream = stream});
}

int vit_engine_cls_attention_device_u8(vit_engine *e, const unsigned char *d_images, int n, const float *mean, const float *std,
                                       const vit_attention_spec *spec, float *d_out, void *stream) {
    return run_call(e, &(vit_call){.who = "cls_attention_device_u8", .place = VIT_AT_DEVICE, .in_kind = VIT_IN_U8, .images = d_images,
                                    .n = n, .mean = mean, .std = std, .out_kind = VIT_OUT_ATTENTION, .spec = spec, .dst = d_out,
                                    .stream = stream});
}

int vit_engine_cls_attention_device_images(vit_engine *e, const vit_image_u8 *images, int n, const vit_preproc *pp,
                                           const vit_attention_spec *spec, float *d_out, void *stream) {
    return run_call(e, &(vit_call){.who = "cls_attention_device_images", .place = VIT_AT_DEVICE, .in_kind = VIT_IN_IMAGES,
                                    .images = images, .n = n, .pp = pp, .out_kind = VIT_OUT_ATTENTION, .spec = spec, .dst = d_out,
                                    .stream = stream});
}

int vit_engine_intermediate_device(vit_engine *e, const float *d_images, int n, const vit_intermediate_spec *spec, float *d_out, void *stream) {
    return run_call(e, &(vit_call){.who = "intermediate_device", .place = VIT_AT_DEVICE, .in_kind = VIT_IN_F32, .images = d_images,
                                    .n = n, .out_kind = VIT_OUT_INTERMEDIATE, .spec = spec, .dst = d_out, .stream = stream});
}

int vit_engine_intermediate_device_u8(vit_engine *e, const unsigned char *d_images, int n, const float *mean, const float *std,
                                      const vit_intermediate_spec *spec, float *d_out, void *stream) {
    return run_call(e, &(vit_call){.who = "intermediate_device_u8", .place = VIT_AT_DEVICE, .in_kind = VIT_IN_U8, .images = d_images,
                                    .n = n, .mean = mean, .std = std, .out_kind = VIT_OUT_INTERMEDIATE, .spec = spec, .dst = d_out,
                                    .stream = stream});
}

int vit_engine_intermediate_device_images(vit_engine *e, const vit_image_u8 *images, int n, const vit_preproc *pp,
                                          const vit_intermediate_spec *spec, float *d_out, void *stream) {
    return run_call(e, &(vit_call){.who = "intermediate_device_images", .place = VIT_AT_DEVICE, .in_kind = VIT_IN_IMAGES,
                                    .images = images, .n = n, .pp = pp, .out_kind = VIT_OUT_INTERMEDIATE, .spec = spec, .dst = d_out,
                                    .stream = stream});
}

int vit_engine_forward_host(vit_engine *e, const float *const *images, int n, float *const *probs) {
    return run_call(e, &(vit_call){.who = "forward_host", .place = VIT_AT_HOST, .in_kind = VIT_IN_F32, .images = images, .n = n,
                                    .out_kind = VIT_OUT_PROBS, .rows = probs});
}

int vit_engine_forward_host_u8(vit_engine *e, const unsigned char *const *images, int n, const float *mean, const float *std,
                               float *const *probs) {
    return run_call(e, &(vit_call){.who = "forward_host_u8", .place = VIT_AT_HOST, .in_kind = VIT_IN_U8, .images = images, .n = n,
                                    .mean = mean, .std = std, .out_kind = VIT_OUT_PROBS, .rows = probs});
}

int vit_engine_forward_host_images(vit_engine *e, const vit_image_u8 *images, int n, const vit_preproc *pp, float *const *probs) {
    return run_call(e, &(vit_call){.who = "forward_host_images", .place = VIT_AT_HOST, .in_kind = VIT_IN_IMAGES, .images = images, .n = n,
                                    .pp = pp, .out_kind = VIT_OUT_PROBS, .rows = probs});
}

int vit_engine_features_host(vit_engine *e, const float *const *images, int n, const vit_feature_spec *spec, float *const *out) {
    return run_call(e, &(vit_call){.who = "features_host", .place = VIT_AT_HOST, .in_kind = VIT_IN_F32, .images = images, .n = n,
                                    .out_kind = VIT_OUT_FEATURES, .spec = spec, .rows = out});
}

int vit_engine_features_host_u8(vit_engine *e, const unsigned char *const *images, int n, const float *mean, const float *std,
                                const vit_feature_spec *spec, float *const *out) {
    return run_call(e, &(vit_call){.who = "features_host_u8", .place = VIT_AT_HOST, .in_kind = VIT_IN_U8, .images = images, .n = n,
                                    .mean = mean, .std = std, .out_kind = VIT_OUT_FEATURES, .spec = spec, .rows = out});
}

int vit_engine_features_host_images(vit_engine *e, const vit_image_u8 *images, int n, const vit_preproc *pp, const vit_feature_spec *spec,
                                    float *const *out) {
    return run_call(e, &(vit_call){.who = "features_host_images", .place = VIT_AT_HOST, .in_kind = VIT_IN_IMAGES, .images = images, .n = n,
                                    .pp = pp, .out_kind = VIT_OUT_FEATURES, .spec = spec, .rows = out});
}

int vit_engine_cls_attention_host(vit_engine *e, const float *const *images, int n, const vit_attention_spec *spec, float *const *out) {
    return run_call(e, &(vit_call){.who = "cls_attention_host", .place = VIT_AT_HOST, .in_kind = VIT_IN_F32, .images = images, .n = n,
                                    .out_kind = VIT_OUT_ATTENTION, .spec = spec, .rows = out});
}

int vit_engine_cls_attention_host_u8(vit_engine *e, const unsigned char *const *images, int n, const float *mean, const float *std,
                                     const vit_attention_spec *spec, float *const *out) {
    return run_call(e, &(vit_call){.who = "cls_attention_host_u8", .place = VIT_AT_HOST, .in_kind = VIT_IN_U8, .images = images, .n = n,
                                    .mean = mean, .std = std, .out_kind = VIT_OUT_ATTENTION, .spec = spec, .rows = out});
}

int vit_engine_cls_attention_host_images(vit_engine *e, const vit_image_u8 *images, int n, const vit_preproc *pp,
                                         const vit_attention_spec *spec, float *const *out) {
    return run_call(e, &(vit_call){.who = "cls_attention_host_images", .place = VIT_AT_HOST, .in_kind = VIT_IN_IMAGES, .images = images,
                                    .n = n, .pp = pp, .out_kind = VIT_OUT_ATTENTION, .spec = spec, .rows = out});
}

int vit_engine_intermediate_host(vit_engine *e, const float *const *images, int n, const vit_intermediate_spec *spec, float *const *out) {
    return run_call(e, &(vit_call){.who = "intermediate_host", .place = VIT_AT_HOST, .in_kind = VIT_IN_F32, .images = images, .n = n,
                                    .out_kind = VIT_OUT_INTERMEDIATE, .spec = spec, .rows = out});
}

int vit_engine_intermediate_host_u8(vit_engine *e, const unsigned char *const *images, int n, const float *mean, const float *std,
                                    const vit_intermediate_spec *spec, float *const *out) {
    return run_call(e, &(vit_call){.who = "intermediate_host_u8", .place = VIT_AT_HOST, .in_kind = VIT_IN_U8, .images = images, .n = n,
                                    .mean = mean, .std = std, .out_kind = VIT_OUT_INTERMEDIATE, .spec = spec, .rows = out});
}

int vit_engine_intermediate_host_images(vit_engine *e, const vit_image_u8 *images, int n, const vit_preproc *pp,
                                        const vit_intermediate_spec *spec, float *const *out) {
    return run_call(e, &(vit_call){.who = "intermediate_host_images", .place = VIT_AT_HOST, .in_kind = VIT_IN_IMAGES, .images = images,
                                    .n = n, .pp = pp, .out_kind = VIT_OUT_INTERMEDIATE, .spec = spec, .rows = out});
}

int vit_engine_topk_device(vit_engine *e, const float *d_images, int n, const vit_topk_spec *spec, int *d_out, void *stream) {
    return run_call(e, &(vit_call){.who = "topk_device", .place = VIT_AT_DEVICE, .in_kind = VIT_IN_F32, .images = d_images, .n = n,
                                    .out_kind = VIT_OUT_TOPK, .spec = spec, .dst = (float *)d_out, .stream = stream});
}

int vit_engine_topk_device_u8(vit_engine *e, const unsigned char *d_images, int n, const float *mean, const float *std,
                              const vit_topk_spec *spec, int *d_out, void *stream) {
    return run_call(e, &(vit_call){.who = "topk_device_u8", .place = VIT_AT_DEVICE, .in_kind = VIT_IN_U8, .images = d_images, .n = n,
                                    .mean = mean, .std = std, .out_kind = VIT_OUT_TOPK, .spec = spec, .dst = (float *)d_out, .stream = stream});
}

int vit_engine_topk_device_images(vit_engine *e, const vit_image_u8 *images, int n, const vit_preproc *pp, const vit_topk_spec *spec,
                                  int *d_out, void *stream) {
    return run_call(e, &(vit_call){.who = "topk_device_images", .place = VIT_AT_DEVICE, .in_kind = VIT_IN_IMAGES, .images = images,
                                    .n = n, .pp = pp, .out_kind = VIT_OUT_TOPK, .spec = spec, .dst = (float *)d_out, .stream = stream});
}

int vit_engine_topk_host(vit_engine *e, const float *const *images, int n, const vit_topk_spec *spec, int *const *out) {
    return run_call(e, &(vit_call){.who = "topk_host", .place = VIT_AT_HOST, .in_kind = VIT_IN_F32, .images = images, .n = n,
                                    .out_kind = VIT_OUT_TOPK, .spec = spec, .rows = (float *const *)out});
}

int vit_engine_topk_host_u8(vit_engine *e, const unsigned char *const *images, int n, const float *mean, const float *std,
                            const vit_topk_spec *spec, int *const *out) {
    return run_call(e, &(vit_call){.who = "topk_host_u8", .place = VIT_AT_HOST, .in_kind = VIT_IN_U8, .images = images, .n = n,
                                    .mean = mean, .std = std, .out_kind = VIT_OUT_TOPK, .spec = spec, .rows = (float *const *)out});
}

int vit_engine_topk_host_images(vit_engine *e, const vit_image_u8 *images, int n, const vit_preproc *pp, const vit_topk_spec *spec,
                                int *const *out) {
    return run_call(e, &(vit_call){.who = "topk_host_images", .place = VIT_AT_HOST, .in_kind = VIT_IN_IMAGES, .images = images, .n = n,
                                    .pp = pp, .out_kind = VIT_OUT_TOPK, .spec = spec, .rows = (float *const *)out});
}

/* the dense calls: rows of bytes, carried through the one call path as the untyped pointers they are */
int vit_engine_dense_device(vit_engine *e, const float *d_images, int n, const vit_dense_spec *spec, void *d_out, void *stream) {
    return run_call(e, &(vit_call){.who = "dense_device", .place = VIT_AT_DEVICE, .in_kind = VIT_IN_F32, .images = d_images, .n = n,
                                    .out_kind = VIT_OUT_DENSE, .spec = spec, .dst = (float *)d_out, .stream = stream});
}

int vit_engine_dense_device_u8(vit_engine *e, const unsigned char *d_images, int n, const float *mean, const float *std,
                               const vit_dense_spec *spec, void *d_out, void *stream) {
    return run_call(e, &(vit_call){.who = "dense_device_u8", .place = VIT_AT_DEVICE, .in_kind = VIT_IN_U8, .images = d_images, .n = n,
                                    .mean = mean, .std = std, .out_kind = VIT_OUT_DENSE, .spec = spec, .dst = (float *)d_out, .stream = stream});
}

int vit_engine_dense_device_images(vit_engine *e, const vit_image_u8 *images, int n, const vit_preproc *pp, const vit_dense_spec *spec,
                                   void *d_out, void *stream) {
    return run_call(e, &(vit_call){.who = "dense_device_images", .place = VIT_AT_DEVICE, .in_kind = VIT_IN_IMAGES, .images = images,
                                    .n = n, .pp = pp, .out_kind = VIT_OUT_DENSE, .spec = spec, .dst = (float *)d_out, .stream = stream});
}

int vit_engine_dense_host(vit_engine *e, const float *const *images, int n, const vit_dense_spec *spec, void *const *out) {
    return run_call(e, &(vit_call){.who = "dense_host", .place = VIT_AT_HOST, .in_kind = VIT_IN_F32, .images = images, .n = n,
                                    .out_kind = VIT_OUT_DENSE, .spec = spec, .rows = (float *const *)out});
}

int vit_engine_dense_host_u8(vit_engine *e, const unsigned char *const *images, int n, const float *mean, const float *std,
                             const vit_dense_spec *spec, void *const *out) {
    return run_call(e, &(vit_call){.who = "dense_host_u8", .place = VIT_AT_HOST, .in_kind = VIT_IN_U8, .images = images, .n = n,
                                    .mean = mean, .std = std, .out_kind = VIT_OUT_DENSE, .spec = spec, .rows = (float *const *)out});
}

int vit_engine_dense_host_images(vit_engine *e, const vit_image_u8 *images, int n, const vit_preproc *pp, const vit_dense_spec *spec,
                                 void *const *out) {
    return run_call(e, &(vit_call){.who = "dense_host_images", .place = VIT_AT_HOST, .in_kind = VIT_IN_IMAGES, .images = images, .n = n,
                                    .pp = pp, .out_kind = VIT_OUT_DENSE, .spec = spec, .rows = (float *const *)out});
}

int vit_engine_handover_stats(vit_engine *e, long *taken, long *recomputed) {
    if (!e) return VIT_ERR_ARG;
    HIP_TRY(e, vithip_set_device(e->opt.device));
    HIP_TRY(e, vithip_device_sync()); /* lanes and caller-provided streams */
    for (int j = 0; j < VIT_MAX_LANES; ++j) {
        int t = 0, r = 0;
        if (!e->gemm_ws[j]) continue;
        HIP_TRY(e, vithip_gemm_f32_workspace_stats(e->gemm_ws[j], &t, &r));
        e->handover_taken += t;
        e->handover_recomputed += r;
    }
    if (taken) *taken = e->handover_taken;
    if (recomputed) *recomputed = e->handover_recomputed;
    e->handover_taken = e->handover_recomputed = 0;
    return VIT_OK;
}

int vit_engine_read_logits(vit_engine *e, float *dst, int rows) {
    if (!e || !dst) return VIT_ERR_ARG;
    if (rows <= 0 || rows > e->last_rows) return fail(e, VIT_ERR_ARG, "read_logits: %d rows requested, last chunk had %d", rows, e->last_rows);
    HIP_TRY(e, vithip_device_sync()); /* the chunk may have run on a caller-provided stream */
    HIP_TRY(e, vithip_memcpy_d2h(dst, e->logits, (size_t)rows * e->cfg.num_classes * sizeof(float), e->stream));
    HIP_TRY(e, vithip_stream_sync(e->stream));
    return VIT_OK;
}

/* The head spec, checked against the model: NULL, or what is wrong as a format for (arg[0], arg[1]). */
static const char *head_spec_fault(const vit_engine *e, const vit_head_spec *spec, int arg[2]) {
    arg[0] = arg[1] = 0;
    arg[0] = spec->num_cls_layers; arg[1] = VIT_MAX_TAPS;
    if (spec->num_cls_layers < 0 || spec->num_cls_layers > VIT_MAX_TAPS) return "set_head: num_cls_layers = %d must be 0..%d";
    arg[0] = spec->pool;
    if (spec->pool != VIT_HEAD_POOL_NONE && spec->pool != VIT_HEAD_POOL_AVG && spec->pool != VIT_HEAD_POOL_AVG_FCNORM)
        return "set_head: unknown pool %d";
    arg[0] = spec->reserved;
    if (spec->reserved != 0) return "set_head: vit_head_spec.reserved must be 0 (got %d)";
    for (int j = 0; j < spec->num_cls_layers; ++j) {
        arg[0] = j; arg[1] = spec->cls_layers[j];
        if (spec->cls_layers[j] < 0 || spec->cls_layers[j] >= e->cfg.depth) return "set_head: cls_layers[%d] = %d is not a layer of the model";
        if (j && spec->cls_layers[j] <= spec->cls_layers[j - 1]) return "set_head: cls_layers[%d] = %d is not above the entry before it (strictly increasing)";
    }
    if (spec->num_cls_layers == 0 && spec->pool == VIT_HEAD_POOL_NONE) return "set_head: the operand is empty (no class layers and no pooled block)";
    if (spec->pool != VIT_HEAD_POOL_NONE && e->patches < 1) return "set_head: a pooled block needs at least one patch token";
    return NULL;
}

size_t vit_engine_head_in_features(const vit_engine *e, const vit_head_spec *spec) {
    int arg[2];
    if (!e || !spec || head_spec_fault(e, spec, arg)) return 0;
    return (size_t)(spec->num_cls_layers + (spec->pool != VIT_HEAD_POOL_NONE)) * (size_t)e->cfg.embed_dim;
}

int vit_engine_set_head(vit_engine *e, const vit_head_spec *spec, const float *weight, const float *bias) {
    if (!e) return VIT_ERR_ARG;
    if (!spec && (weight || bias)) return fail(e, VIT_ERR_ARG, "set_head: a NULL spec (the checkpoint's own head) takes no weight and no bias");
    if (spec) {
        int arg[2];
        const char *fault = head_spec_fault(e, spec, arg);
        if (fault) return fail(e, VIT_ERR_ARG, fault, arg[0], arg[1]);
        if (!weight || !bias) return fail(e, VIT_ERR_ARG, "set_head: weight and bias are required with a spec");
    }
    if (!e->weights_loaded) return fail(e, VIT_ERR_STATE, "set_head before vit_engine_load_weights()");
    HIP_TRY(e, vithip_set_device(e->opt.device));
    if (!spec) { /* as an install: nothing in flight, no graph with the old operands in its launches */
        HIP_TRY(e, vithip_device_sync());
        drop_graph(e);
        restore_own_head(e);
        return VIT_OK;
    }
    /* the new head first, whole; only then the old one goes */
    const size_t F = vit_engine_head_in_features(e, spec), NC = (size_t)e->cfg.num_classes, B = (size_t)e->opt.max_batch;
    const size_t wbytes = NC * F * sizeof(float);
    const size_t pad = 128 * F * sizeof(float) > WEIGHT_TAIL_PAD ? 128 * F * sizeof(float) : WEIGHT_TAIL_PAD; /* a GEMM tile of rows */
    float *w = NULL, *b = NULL, *operand = NULL;
    int hrc = vithip_malloc((void **)&w, wbytes + pad);
    if (!hrc) hrc = vithip_malloc((void **)&b, NC * sizeof(float));
    if (!hrc) hrc = vithip_malloc((void **)&operand, B * F * sizeof(float));
    if (hrc) {
        vithip_free(w); vithip_free(b); vithip_free(operand);
        return fail(e, VIT_ERR_NOMEM, "set_head: no memory for a head of %zu x %zu floats and %zu operand rows (HIP error %d: %s); the previous head stays",
                    NC, F, B, hrc, vithip_error_string(hrc));
    }
    hrc = vithip_memcpy_h2d(w, weight, wbytes, e->stream);
    if (!hrc) hrc = vithip_memset((char *)w + wbytes, 0, pad, e->stream);
    if (!hrc) hrc = vithip_memcpy_h2d(b, bias, NC * sizeof(float), e->stream);
    if (!hrc) hrc = vithip_memset(operand, 0, B * F * sizeof(float), e->stream);
    if (!hrc) hrc = vithip_device_sync(); /* the uploads, and every forward that still reads the old head, on whatever stream */
    if (hrc) {
        vithip_free(w); vithip_free(b); vithip_free(operand);
        return fail(e, VIT_ERR_HIP, "set_head: HIP error %d (%s) uploading the head; the previous head stays", hrc, vithip_error_string(hrc));
    }
    drop_graph(e);
    release_head(&e->head);
    e->head = (vit_head){.in = F, .ops = {.W = w, .bias = b}, .operand = operand, .owned = 1};
    e->head.spec.num_cls_layers = spec->num_cls_layers; /* the entries of cls_layers behind num_cls_layers stay zero */
    for (int j = 0; j < spec->num_cls_layers; ++j) e->head.spec.cls_layers[j] = spec->cls_layers[j];
    e->head.spec.pool = spec->pool;
    e->last_rows = 0;
    return VIT_OK;
}

int vit_engine_read_head_operand(vit_engine *e, float *dst, int rows) {
    if (!e || !dst) return VIT_ERR_ARG;
    if (rows <= 0 || rows > e->last_rows) return fail(e, VIT_ERR_ARG, "read_head_operand: %d rows requested, last chunk had %d", rows, e->last_rows);
    HIP_TRY(e, vithip_device_sync()); /* the chunk may have run on a caller-provided stream */
    HIP_TRY(e, vithip_memcpy_d2h(dst, e->head.operand, (size_t)rows * e->head.in * sizeof(float), e->stream));
    HIP_TRY(e, vithip_stream_sync(e->stream));
    return VIT_OK;
}

/* The dense head spec, checked against the model: NULL, or what is wrong as a format for (arg[0], arg[1]). */
static const char *dense_head_spec_fault(const vit_engine *e, const vit_dense_head_spec *spec, int arg[2]) {
    arg[0] = spec->num_layers; arg[1] = VIT_MAX_TAPS;
    if (spec->num_layers < 1 || spec->num_layers > VIT_MAX_TAPS) return "set_dense_head: num_layers = %d must be 1..%d";
    arg[0] = spec->norm; arg[1] = 0;
    if (spec->norm != 0 && spec->norm != 1) return "set_dense_head: norm must be 0 or 1 (got %d)";
    arg[0] = spec->num_classes;
    if (spec->num_classes < 1 || spec->num_classes > 255) return "set_dense_head: num_classes = %d must be 1..255 (a label is a byte, 255 the empty one)";
    arg[0] = spec->reserved;
    if (spec->reserved != 0) return "set_dense_head: vit_dense_head_spec.reserved must be 0 (got %d)";
    for (int j = 0; j < spec->num_layers; ++j) {
        arg[0] = j; arg[1] = spec->layers[j];
        if (spec->layers[j] < 0 || spec->layers[j] >= e->cfg.depth) return "set_dense_head: layers[%d] = %d is not a layer of the model";
        if (j && spec->layers[j] <= spec->layers[j - 1]) return "set_dense_head: layers[%d] = %d is not above the entry before it (strictly increasing)";
    }
    const int g = e->cfg.img_size / VIT_PATCH_SIZE(&e->cfg);
    arg[0] = g; arg[1] = e->patches;
    if (g < 1 || g * g != e->patches) return "set_dense_head: needs a square grid of patches: (img_size / patch_size = %d)^2 is not the model's %d";
    return NULL;
}

int vit_engine_set_dense_head(vit_engine *e, const vit_dense_head_spec *spec, const float *weight, const float *bias) {
    if (!e) return VIT_ERR_ARG;
    if (!spec && (weight || bias)) return fail(e, VIT_ERR_ARG, "set_dense_head: a NULL spec (no dense head) takes no weight and no bias");
    if (spec) {
        int arg[2];
        const char *fault = dense_head_spec_fault(e, spec, arg);
        if (fault) return fail(e, VIT_ERR_ARG, fault, arg[0], arg[1]);
        if (!weight || !bias) return fail(e, VIT_ERR_ARG, "set_dense_head: weight and bias are required with a spec");
    }
    if (!e->weights_loaded) return fail(e, VIT_ERR_STATE, "set_dense_head before vit_engine_load_weights()");
    HIP_TRY(e, vithip_set_device(e->opt.device));
    if (!spec) { /* as an install: nothing in flight, no graph with the head's buffers in its launches */
        HIP_TRY(e, vithip_device_sync());
        drop_graph(e);
        release_dense_head(&e->dense);
        return VIT_OK;
    }
    /* the new head first, whole; only then the old one goes */
    const size_t D = (size_t)e->cfg.embed_dim, F = (size_t)spec->num_layers * D, NC = (size_t)spec->num_classes,
                 B = (size_t)e->opt.max_batch, P = (size_t)e->patches;
    const size_t wbytes = NC * F * sizeof(float);
    const size_t pad = 128 * F * sizeof(float) > WEIGHT_TAIL_PAD ? 128 * F * sizeof(float) : WEIGHT_TAIL_PAD; /* a GEMM tile of rows */
    vit_dense_head h;
    memset(&h, 0, sizeof(h));
    int hrc = vithip_malloc((void **)&h.W, wbytes + pad);
    if (!hrc) hrc = vithip_malloc((void **)&h.bias, NC * sizeof(float));
    if (!hrc) hrc = vithip_malloc((void **)&h.zero_bias, NC * sizeof(float));
    if (!hrc) hrc = vithip_malloc((void **)&h.rows, B * P * D * sizeof(float));
    if (!hrc) hrc = vithip_malloc((void **)&h.logits, B * P * NC * sizeof(float));
    if (hrc) {
        release_dense_head(&h);
        return fail(e, VIT_ERR_NOMEM, "set_dense_head: no memory for a head of %zu x %zu floats, %zu x %zu patch rows and their logits (HIP error %d: %s); "
                    "the previous dense head stays", NC, F, B, P, hrc, vithip_error_string(hrc));
    }
    hrc = vithip_memcpy_h2d(h.W, weight, wbytes, e->stream);
    if (!hrc) hrc = vithip_memset((char *)h.W + wbytes, 0, pad, e->stream);
    if (!hrc) hrc = vithip_memcpy_h2d(h.bias, bias, NC * sizeof(float), e->stream);
    if (!hrc) hrc = vithip_memset(h.zero_bias, 0, NC * sizeof(float), e->stream);
    if (!hrc) hrc = vithip_device_sync(); /* the uploads, and every call that still uses the old head, on whatever stream */
    if (hrc) {
        release_dense_head(&h);
        return fail(e, VIT_ERR_HIP, "set_dense_head: HIP error %d (%s) uploading the head; the previous dense head stays", hrc, vithip_error_string(hrc));
    }
    drop_graph(e);
    release_dense_head(&e->dense);
    h.spec.num_layers = spec->num_layers; /* the entries of layers behind num_layers stay zero */
    for (int j = 0; j < spec->num_layers; ++j) h.spec.layers[j] = spec->layers[j];
    h.spec.norm = spec->norm; h.spec.num_classes = spec->num_classes;
    e->dense = h;
    return VIT_OK;
}

int vit_engine_debug_pool_scratch(vit_engine *e, int nb, int lane, size_t range[6]) {
    if (!e || !range || nb <= 0 || nb > e->opt.max_batch || lane < 0) return -1;
    vit_feature_spec spec = {VIT_FEAT_MEAN, 0};
    vit_output out;
    chunk_ctx c;
    if (make_output(e, "debug_pool_scratch", VIT_OUT_FEATURES, &spec, NULL, NULL, NULL, &out)) return -1;
    chunk_setup(e, e->stream, nb, &out, &c);
    if (lane >= c.L) return -1;
    const vit_lane *ln = &c.lane[lane];
    const size_t rows = (size_t)ln->n * c.T * c.D;
    size_t need;
    const char *base = (const char *)e->y, *scratch = (const char *)pool_scratch(&c, ln, &need);
    range[0] = (size_t)(scratch - base); range[1] = range[0] + need;
    range[2] = (size_t)((const char *)ln->y - base); range[3] = range[2] + rows * c.esz;
    range[4] = range[5] = 0;
    if (ln->xa && ln->xa != (void *)ln->x) { /* the fold's bf16 copy of x, in y's upper half */
        range[4] = (size_t)((const char *)ln->xa - base); range[5] = range[4] + rows * sizeof(unsigned short);
    }
    return c.L;
}

int vit_engine_get_stage_times(vit_engine *e, vit_stage_times *out) {
    if (!e || !out) return VIT_ERR_ARG;
    int rc = collect_profile(e);
    if (rc) return rc;
    *out = e->times;
    return VIT_OK;
}

void vit_engine_reset_stage_times(vit_engine *e) {
    if (!e) return;
    collect_profile(e); /* drain the pool so earlier brackets do not leak into the next window */
    memset(&e->times, 0, sizeof(e->times));
}
