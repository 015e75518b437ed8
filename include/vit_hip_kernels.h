/*
 * include/vit_hip_kernels.h -- the thin C-ABI over HIP.
 *
 * The host side of this project is C (as the reference's is); everything that needs the HIP
 * runtime or a gfx950 kernel sits behind these extern "C" entry points, compiled by hipcc
 * (csrc/ *.hip).  Only plain pointers, sizes and ints cross the boundary.  Each launcher is
 * asynchronous on the given stream (NULL = the default stream) and returns 0 on success or
 * a hipError_t value; vithip_error_string() renders it.
 *
 * What each kernel launcher replaces in the reference's OpenCL path:
 *   vithip_patch_embed_f32   Conv2d_opencl + CPU flatten_transpose/class_token/pos_emb
 *                            (ViT_opencl.c:126-180,806-810; kernel.cl:120-175)
 *   vithip_layernorm_f32     layer_norm_opencl (ViT_opencl.c:233-291; kernel.cl:6-80) -- but with
 *                            ViT_seq.c:103-121 numerics (eps = 1e-6, added in double)
 *   vithip_gemm_f32          enqueue_gemm_stage/add_bias_helper, fc1/gelu/fc2 kernels,
 *                            linear_layer_opencl and the CPU residual adds
 *                            (ViT_opencl.c:294-335,369-380,449-497,607-729,758-777;
 *                             kernel.cl:208-284,374-533) with exact-erf GELU (ViT_seq.c:231-233)
 *   vithip_attention_f32     the per-head scores GEMM / softmax / P.V chain
 *                            (ViT_opencl.c:499-602; kernel.cl:289-365), ViT_seq.c:156-215 numerics
 *   vithip_softmax_top1_f32  CPU Softmax (ViT_opencl.c:881 -> ViT_seq.c:304-324) and the
 *                            argmax loop of Main.c:62-72
 */
#ifndef VIT_HIP_KERNELS_H
#define VIT_HIP_KERNELS_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *vithip_stream_t; /* hipStream_t     */
typedef void *vithip_event_t;  /* hipEvent_t      */
typedef void *vithip_graph_t;  /* hipGraphExec_t  */

typedef struct {
    char name[256];
    char arch[64];            /* gcnArchName, e.g. "gfx950:sramecc+:xnack-" */
    int compute_units;
    int clock_mhz;            /* max engine clock */
    int wavefront;
    int lds_per_block;        /* bytes */
    unsigned long long hbm_bytes;
} vithip_device_info;

/* ---- runtime plumbing --------------------------------------------------------------- */
const char *vithip_error_string(int code);
int vithip_device_count(int *count);
int vithip_set_device(int device);
int vithip_get_device_info(int device, vithip_device_info *info);
int vithip_malloc(void **ptr, size_t bytes);
int vithip_free(void *ptr);
int vithip_host_alloc(void **ptr, size_t bytes);   /* pinned */
int vithip_host_free(void *ptr);
int vithip_memcpy_h2d(void *dst, const void *src, size_t bytes, vithip_stream_t stream);
int vithip_memcpy_d2h(void *dst, const void *src, size_t bytes, vithip_stream_t stream);
int vithip_memcpy_d2d(void *dst, const void *src, size_t bytes, vithip_stream_t stream);
int vithip_memcpy_peer(void *dst, int dst_device, const void *src, int src_device, size_t bytes, vithip_stream_t stream);
int vithip_memset(void *dst, int value, size_t bytes, vithip_stream_t stream);
int vithip_stream_create(vithip_stream_t *stream);
int vithip_stream_destroy(vithip_stream_t stream);
int vithip_stream_sync(vithip_stream_t stream);
int vithip_device_sync(void);
int vithip_event_create(vithip_event_t *event);
int vithip_event_destroy(vithip_event_t event);
int vithip_event_record(vithip_event_t event, vithip_stream_t stream);
int vithip_event_sync(vithip_event_t event);
int vithip_event_elapsed_ms(float *ms, vithip_event_t start, vithip_event_t stop);
int vithip_stream_wait_event(vithip_stream_t stream, vithip_event_t event);
int vithip_graph_begin(vithip_stream_t stream);
int vithip_graph_end(vithip_stream_t stream, vithip_graph_t *graph);
int vithip_graph_launch(vithip_graph_t graph, vithip_stream_t stream);
int vithip_graph_destroy(vithip_graph_t graph);

/* ---- kernels ------------------------------------------------------------------------- */

/* The LayerNorm epsilon of every entry point that does not take one: the DOUBLE 1e-6 of the reference (ViT_seq.c:103-121), added to
 * the variance in double before the cast back to float.  Every such entry point has a sibling `<name>_eps(..., double eps)` with one
 * more, last, argument (finite, > 0, else hipErrorInvalidValue) and IS a call of that sibling with VITHIP_LN_EPS: the two cannot
 * drift, and with this value the sibling gives the old entry point's bits.  (CLIP: 1e-5.  HF ViTModel: 1e-12.) */
#define VITHIP_LN_EPS 1e-6
enum { VITHIP_EPI_BIAS = 0, VITHIP_EPI_BIAS_GELU = 1, VITHIP_EPI_BIAS_RESIDUAL = 2,
       VITHIP_EPI_BIAS_QGELU = 6 /* 3, 4, 5 and 7 are the library's own fold forms */ };

/*
 * C[M][ldc] (first N columns) = epilogue(A[M][K] . W[N][K]^T + bias[N]):
 * the shape of every linear layer of the model (weights are [out][in], K contiguous in both
 * operands).  fp32 in, fp32 MFMA accumulate (v_mfma_f32_32x32x2_f32), fp32 out.
 *   EPI_BIAS_GELU:     y = 0.5*y*(1+erff(y/sqrtf(2)))                 (ViT_seq.c:231-233)
 *   EPI_BIAS_RESIDUAL: y += residual[m][n]; residual may alias C      (ViT_seq.c:286-288,297-299)
 *   EPI_BIAS_QGELU:    y = y / (1 + exp(-1.702 y)), CLIP's QuickGELU: PyTorch's x * torch.sigmoid(1.702 * x).  One sequence in every
 *                      kernel, fp32 and bf16, value by value: t = y * fp32(-1.702 * log2 e) (v_mul_f32), e = 2^t (v_exp_f32),
 *                      d = 1 + e (v_add_f32), r = 1 / d (v_rcp_f32), y * r (v_mul_f32).  +Inf gives +Inf, -Inf and NaN give NaN, a
 *                      large negative finite y gives a tiny negative value or -0 (r flushes to 0 once d passes 2^126), never NaN.
 * Requirements, the same for every tile code, both arithmetics and the w_split image (anything else: hipErrorInvalidValue):
 *   K % 32 == 0; lda, ldw >= K and % 4 == 0, A and W 16-byte aligned (the operands are read 128 bits at a time);
 *   ldc, ldr >= N, any value: C, residual and bias are accessed one float at a time and need only their natural 4-byte
 *     alignment (the 10-class head stores with ldc = 10 through a C that is only 4-byte aligned);
 *   W has exactly N rows: every tile clamps the row index of W to N - 1, nothing behind row N - 1 is read.
 * Only columns 0..N-1 of rows 0..M-1 of C are written.
 */
typedef struct {
    const float *A; int lda;
    const float *W; int ldw;
    const float *bias;
    const float *residual; int ldr;
    float *C; int ldc;
    int M, N, K;
    int epilogue;
    /* tuning, per call (the library keeps no process-wide tuning state); 0 = auto:
     * tile: 0 = auto (persistent walk of 128x128 tiles from ~1,280 tiles on, 64x64 / 32x32 tiles as the problem
     *   shrinks); one software-pipelined tile per workgroup: 10 = 128x128, 6 = 128x128 with K step 16, 7 = 256x128, 8 = 128x64,
     *   11 = 64x64; 12 = 32x32 on 16x16x4 MFMA (K % 128 == 0); 9 = persistent 128x128 (with arith = 1 and w_split: 64x256 where
     *   N % 256 == 0, see w_split).  All of them give the same bits.
     * group_m: tile rows per L2 group of the XCD-aware tile walk (0 = default: plain N-fastest order when N is at most 8 tiles of
     *   128 wide, groups of 4 tile rows beyond that; 1 = plain N-fastest order). */
    int tile, group_m;
    /* optional scratch: the HANDLE made by vithip_gemm_f32_workspace_create() on the device the launch runs on (one per
     * stream: launches that share it must be ordered).  With it, large problems whose tile count is not a multiple of the
     * workgroup count hand the first K-steps of the last round's tiles to the workgroups that would idle (bit-identical
     * results: the accumulation chain moves between workgroups, it is not split; csrc/vit_gemm_persistent.hip).  Nobody
     * waits in that hand-over: an owner that does not find its piece computes the whole tile.  NULL = off. */
    void *workspace;
    /* testing: 1 = the helper workgroups run their pieces LAST, so that owners look for them too early and take the
     * compute-it-yourself path (results must not change); 0 = normal. */
    int handover_test;
    /* LayerNorm folded into the GEMM behind it (both NULL = off; EPI_BIAS, EPI_BIAS_GELU and EPI_BIAS_QGELU only): A holds the UN-normalised
     * rows x, W and bias are the gamma- and beta-folded operands of vithip_ln_fold_weights_f32(), ln_rows [M][2] = (rstd, mean)
     * per row of A (vithip_rowstats_f32), ln_colsum [N] -- or NULL when W is the CENTRED weight of
     * vithip_ln_fold_weights_f32_centered(), whose product needs no centring (the term below is then skipped); the epilogue computes
     *     fmaf(rstd, fmaf(-mean, colsum, acc), bias) = LayerNorm(x) . W^T + b                 (ViT_seq.c:103-121 is the LayerNorm)
     * with the same two roundings in every kernel (the 32x32 kernels take the inner one as a rank-1 matrix instruction, four per
     * wave and tile: csrc/vit_gemm_common.hpp), so that the tile shapes stay bit-identical to each other.
     * (Rows of near-zero variance: the cancellation error of the inner term is scaled by rstd, up to 1e3 there, where
     * LayerNorm-then-GEMM gives exact zeros; real residual rows have rstd of order 1.  Measured, not asserted away:
     * tests/test_gpu_lnfold.py::test_fp32_fold_on_near_constant_rows_stays_inside_its_stated_bound.)  The normalised activations never exist in memory: the pass that wrote them (read x, write y: 310 MB at batch 256, 24 times per
     * ViT-B/16 forward) becomes a pass that reads x and writes 8 bytes per row. */
    const float *ln_rows, *ln_colsum;
    /* ... and the producer side (NULL = off; EPI_BIAS_RESIDUAL only, N % 64 == 0, N <= 2048): stats_out [M][2] receives (rstd,
     * mean) of the rows of C as stored -- what vithip_rowstats_f32(C) would write, bit for bit.  With stats_partials
     * ([N / 64][M][2] floats of scratch) the persistent walk takes the sums in its epilogue, where the row is in the accumulators
     * (one small launch then finalises them: vithip_gemm_f32_stats_in_epilogue() says whether a call would); any other kernel,
     * or no scratch, and the call runs vithip_rowstats_f32 behind the GEMM. */
    float *stats_out, *stats_partials;
    /* arithmetic of the contraction: 0 = fp32 operands on v_mfma_f32_32x32x2_f32; 1 = three-piece split: each fp32 operand is
     * staged as hi + mid + lo bf16 pieces (exact) and the six piece products of rank <= 2 run on v_mfma_f32_32x32x16_bf16,
     * 6/16 of the fp32 instruction's matrix time, error of the order of an fp32 dot product's.  With 1 the
     * tile codes 0, 9, 10 and 11 are accepted and give the same bits as each other; 6, 7, 8 and 12 are refused. */
    int arith;
    /* optional, arith = 1 only: W's pieces made ahead of time by vithip_split3_weights_f32(W, ldw, N, K) (16-byte aligned; NULL =
     * split W on the fly).  The persistent walk (tile 9, or auto where it picks the walk) then feeds W's pieces straight from the
     * image and splits only A: in 64x256 tiles where N % 256 == 0 (four waves side by side share one split of A), in 128x128 tiles
     * otherwise (vithip_gemm_f32_walk_tile() says which); every other kernel ignores the field.  The pieces are the ones the
     * on-the-fly split makes, so the result has the same bits with and without it, in either tile. */
    const void *w_split;
    /* the LayerNorm epsilon of stats_out (ignored without it): 0 = VITHIP_LN_EPS, else a finite positive double */
    double stats_eps;
} vithip_gemm_args;
/* Non-finite values (NaN, +-Inf, or finite ones whose products overflow) in one row of A reach only that row of C and of stats_out,
 * whatever the tile, arith, w_split or workspace: every other output has the bits of the same launch on clean data
 * (tests/test_gpu_isolation.py). */
int vithip_gemm_f32(vithip_stream_t stream, const vithip_gemm_args *args);
/* Pre-split weight image for vithip_gemm_args.w_split: the hi / mid / lo bf16 pieces of W [N][ldw] (K % 32 == 0, ldw % 4 == 0,
 * 16-byte aligned), the arithmetic of the on-the-fly split (round to nearest even, +-Inf, NaN and subnormals included).  Layout: one
 * 12 KB block per 128-row panel and 16-deep K step (panel-major, K steps ascending inside a panel), a block = 3 planes x 128 rows
 * x 16 bf16; rows past N are zero.  vithip_split3_weights_bytes(N, K) = ceil(N / 128) * 128 * K * 6 (0 for bad arguments). */
size_t vithip_split3_weights_bytes(int N, int K);
int vithip_split3_weights_f32(vithip_stream_t stream, const float *W, int ldw, int N, int K, void *out);
int vithip_gemm_f32_stats_in_epilogue(const vithip_gemm_args *args);  /* 1 / 0 (0 also for arguments vithip_gemm_f32 would refuse) */
/* Host only, launches nothing: the tile (*bm rows x *bn columns) the persistent walk takes for these arguments -- 64 x 256 for the
 * image walk (arith = 1 with w_split) where N % 256 == 0, 128 x 128 otherwise -- whether or not the call's tile code picks the
 * walk.  A pure function of N, the epilogue (with ln_rows / the row statistics), arith and w_split.  0, or hipErrorInvalidValue. */
int vithip_gemm_f32_walk_tile(const vithip_gemm_args *args, int *bm, int *bn);
/* ---- LayerNorm folding, fp32: LN(x) . W^T + b = rstd * (x . (gamma*W)^T) - rstd * mean * colsum(gamma*W) + (b + W . beta).
 * Wf[n][k] = gamma[k] * W[n][k] (fp32 product); colsum[n] = sum_k Wf[n][k] and bias_f[n] = bias[n] + sum_k beta[k] * W[n][k], both
 * accumulated in double and rounded once.  W fp32 [N][K], K % 4 == 0, 16-byte aligned. */
int vithip_ln_fold_weights_f32(vithip_stream_t stream, const float *W, const float *bias, const float *gamma, const float *beta,
                               float *Wf, float *colsum, float *bias_f, int N, int K);
/* The CENTRED form of the same fold (round 5; what vit_engine uses): Wc[n][k] = gamma[k] * W[n][k] - cbar[n] with
 * cbar[n] = sum_k gamma[k] * W[n][k] / K (sum and difference in double, one rounding per weight).  Since mean(x) = sum_k x[k] / K,
 *     x . Wc^T = x . (gamma*W)^T - mean * colsum(gamma*W):
 * the GEMM delivers the centred product itself and its epilogue only scales: pass Wc and bias_f with ln_rows set and
 * ln_colsum = NULL.  residual_colsum[n] = sum_k Wc[n][k] (what the rounding of the weights left of the column sum, for the
 * record: ~1e-7 of |W|).  Same alignment rules. */
int vithip_ln_fold_weights_f32_centered(vithip_stream_t stream, const float *W, const float *bias, const float *gamma,
                                        const float *beta, float *Wc, float *residual_colsum, float *bias_f, int N, int K);
/* rows_out[m] = (rstd, mean) of x [rows][ldx], dim % 64 == 0, dim <= 2048: mean and E[x^2] - mean^2 as ViT_seq.c:103-121
 * takes them, 1 / sqrtf((double)var + 1e-6).  The sums run in ONE documented order (per 64-column strip: columns c and c + 32
 * added first, then a 32-lane butterfly 16, 8, 4, 2, 1; strips in ascending order), the order a GEMM epilogue that holds the
 * row in its accumulators can reproduce -- so that whoever produces the statistics produces the same bits. */
int vithip_rowstats_f32(vithip_stream_t stream, const float *x, size_t ldx, float *rows_out, int rows, int dim);
int vithip_rowstats_f32_eps(vithip_stream_t stream, const float *x, size_t ldx, float *rows_out, int rows, int dim, double eps);
/* partials [dim / 64][rows][2] (sum, sum of squares per 64-column strip, in the order above) -> rows_out [rows][2] */
int vithip_rowstats_finalize_f32(vithip_stream_t stream, const float *partials, int rows, int dim, float *rows_out);
int vithip_rowstats_finalize_f32_eps(vithip_stream_t stream, const float *partials, int rows, int dim, float *rows_out, double eps);
size_t vithip_gemm_f32_workspace_bytes(void);             /* device bytes a workspace takes on the current device */
int vithip_gemm_f32_workspace_create(void **workspace);   /* on the current device */
int vithip_gemm_f32_workspace_destroy(void *workspace);
/* Hand-over counters since the last call (blocking; the stream's launches should be complete): tiles finished from a parked
 * piece / tiles an owner computed whole because the piece was not there yet.  Either pointer may be NULL.  Clears them. */
int vithip_gemm_f32_workspace_stats(void *workspace, int *taken, int *recomputed);
void *vithip_gemm_f32_workspace_device_ptr(void *workspace);  /* [flag per owner ... ][64 KB slots]; tests */
/* ---- bf16 variant (BASELINE.json configs[2]) ---------------------------------
 * bf16 values are raw uint16 (upper half of the fp32 bit pattern, round-to-nearest-even). */
enum { VITHIP_BF16_EPI_BF16 = 0, VITHIP_BF16_EPI_BF16_GELU = 1, VITHIP_BF16_EPI_F32_RESIDUAL = 2,
       VITHIP_BF16_EPI_F32_EMBED = 3 /* internal to vithip_patch_embed_bf16 */,
       VITHIP_BF16_EPI_BF16_QGELU = 4 /* C bf16 = bf16(q(acc + bias)): the fp32 sequence of VITHIP_EPI_BIAS_QGELU on the fp32 accumulator, rounded once */ };
typedef struct {
    const unsigned short *A; int lda;   /* bf16 [M][lda], K contiguous */
    const unsigned short *W; int ldw;   /* bf16 [N][ldw] */
    const float *bias;                  /* fp32 [N] */
    const float *residual; int ldr;     /* fp32, EPI_F32_RESIDUAL only; may alias C */
    void *C; int ldc;                   /* bf16 (EPI_BF16, EPI_BF16_GELU, EPI_BF16_QGELU) or fp32 (EPI_F32_RESIDUAL) */
    int M, N, K;                        /* K % 64 == 0, N % 4 == 0, lda/ldw % 8 == 0 */
    int epilogue;
    /* testing, per call: 0 auto (ping-pong kernel whenever K >= 128), 1 two-stage kernel (vit_gemm_bf16.hip: the fallback for
     * K < 128), 2 ping-pong kernel (vit_gemm_bf16_pp.hip; invalid-value error when K < 128) */
    int variant;
    /* LayerNorm folded into the GEMMs either side of it (all NULL = off; ping-pong kernel only, i.e. K >= 128):
     * producer, EPI_F32_RESIDUAL with x16 and row_partials set: besides C the epilogue stores bf16(C) to x16 [M][ldx16]
     *   (ldx16 % 8 == 0, 16-byte aligned) and the partial (sum, sum of squares) of every row over every 64-column strip to
     *   row_partials [vithip_ln_strips(N)][M][2]; vithip_rowstats_finalize() turns them into ln_rows;
     * consumer, EPI_BF16 / EPI_BF16_GELU / EPI_BF16_QGELU with ln_rows and ln_colsum set: A is the UN-normalised bf16 row, W and bias are the
     *   gamma- and beta-folded operands of vithip_ln_fold_weights(), ln_rows [M][2] = (rstd, mean * rstd) per row of A and
     *   ln_colsum [N]; the epilogue computes rstd * acc - (mean * rstd) * colsum + bias = LayerNorm(x) . W^T + b. */
    const float *ln_rows, *ln_colsum;
    unsigned short *x16; int ldx16;
    float *row_partials;
} vithip_gemm_bf16_args;
/* C = epilogue(A . W^T + bias) on the bf16 matrix pipe (v_mfma_f32_16x16x32_bf16 in the ping-pong kernel,
 * v_mfma_f32_32x32x16_bf16 in the two-stage one), fp32 accumulate.  BF16_GELU rounds gelu(acc + bias) to bf16 (a
 * polynomial erfc whose error stays below 5 % of half a bf16 ulp for acc + bias >= -4 sqrt 2; below it an absolute 4.4e-8: the
 * result is the constant -4.36e-8 there, where gelu tends to 0); F32_RESIDUAL adds an fp32 residual in fp32.
 * Non-finite values in one row of A reach only that row of C, x16 and row_partials -- and do reach it: a NaN accumulator comes out
 * of BF16_GELU as NaN, an infinite one as NaN or Inf -- every other output has the bits of the same launch on clean data. */
int vithip_gemm_bf16(vithip_stream_t stream, const vithip_gemm_bf16_args *args);
/* ---- LayerNorm folding (bf16 forward): LN(x) . W^T + b = rstd * (x . (gamma*W)^T) - rstd * mean * colsum(gamma*W) + (b + W . beta),
 * so the normalised activations never exist in memory: the residual GEMM in front stores bf16(x) and row sums, the GEMM
 * behind multiplies the raw bf16 rows with the folded weight and rescales in its epilogue (ViT_seq.c:103-121 is the
 * LayerNorm being folded: mean, var = E[x^2] - mean^2, 1/sqrt(var + 1e-6)). */
/* Wf[n][k] = bf16(gamma[k] * W[n][k]); colsum[n] = sum_k float(Wf[n][k]) (the ROUNDED values: the mean term then cancels
 * exactly what the matrix pipe accumulates); bias_f[n] = bias[n] + sum_k beta[k] * W[n][k].  W fp32 [N][K], K % 4 == 0. */
int vithip_ln_fold_weights(vithip_stream_t stream, const float *W, const float *bias, const float *gamma, const float *beta,
                           unsigned short *Wf, float *colsum, float *bias_f, int N, int K);
/* The same with output features [0, scale_rows) made `scale` times as large (rows of Wf and their bias_f; colsum is taken of the
 * scaled, rounded rows): the engine folds the factor of the attention scores' exponent, VITHIP_QSCALE, into the Q rows of in_proj,
 * so that q is still rounded to bf16 once and the attention kernels need no scaling pass (vithip_attention_bf16io_qscaled). */
#define VITHIP_QSCALE 0.18033688011112042f /* (1/sqrtf(64)) * log2(e): softmax(q.k / 8) = 2^(QSCALE q.k - max) / sum */
int vithip_ln_fold_weights_scaled(vithip_stream_t stream, const float *W, const float *bias, const float *gamma, const float *beta,
                                  unsigned short *Wf, float *colsum, float *bias_f, int N, int K, int scale_rows, float scale);
/* x16 = bf16(x) and rows[m] = (rstd, mean * rstd) of fp32 rows x [rows][ldx] (the first LayerNorm of the stack, which has no
 * residual GEMM in front of it). */
int vithip_rowstats_bf16(vithip_stream_t stream, const float *x, size_t ldx, unsigned short *x16, size_t ldx16,
                         float *rows_out, int rows, int dim);
int vithip_rowstats_bf16_eps(vithip_stream_t stream, const float *x, size_t ldx, unsigned short *x16, size_t ldx16,
                             float *rows_out, int rows, int dim, double eps);
/* strips = vithip_ln_strips(N) = 4 * ceil(N / 256): partials [strips][rows][2] (sum, sum of squares) -> rows_out [rows][2]. */
int vithip_ln_strips(int N);
int vithip_rowstats_finalize(vithip_stream_t stream, const float *partials, int strips, int rows, int dim, float *rows_out);
int vithip_rowstats_finalize_eps(vithip_stream_t stream, const float *partials, int strips, int rows, int dim, float *rows_out, double eps);
/* dst[r * dst_stride .. + width) = src[r * src_stride .. + width): a strided row subset made compact (e.g. the pairs of the class
 * rows).  rows, width >= 1; both strides >= width; 4-byte alignment suffices. */
int vithip_gather_rows_f32(vithip_stream_t stream, const float *src, size_t src_stride, float *dst, size_t dst_stride, int rows,
                           int width);
/* LayerNorm with fp32 statistics and a bf16 store; attention reading bf16 Q/K/V [n*tokens][3*heads*64] and
 * writing bf16 [n*tokens][heads*64]: both products on bf16 MFMA with fp32 softmax (P rounded to bf16 once);
 * vithip_attention_bf16io_f32math: same I/O, K/V widened to fp32 in LDS and the fp32 kernel's arithmetic (cross-check).
 * Which kernel an attention entry runs for which arguments, and what each refuses: the table at the head of csrc/vit_attention.hip.
 * Non-finite values in one row (LayerNorm) / in one image's rows (both attention entries) reach only that row's / that image's
 * outputs; all other outputs have the bits of the same launch on clean data. */
int vithip_layernorm_f32_bf16out(vithip_stream_t stream, const float *x, size_t ldx, unsigned short *y, size_t ldy,
                                 const float *gamma, const float *beta, int rows, int dim);
int vithip_layernorm_f32_bf16out_eps(vithip_stream_t stream, const float *x, size_t ldx, unsigned short *y, size_t ldy,
                                     const float *gamma, const float *beta, int rows, int dim, double eps);
int vithip_attention_bf16io(vithip_stream_t stream, const unsigned short *qkv, unsigned short *out,
                            int n_images, int tokens, int heads);
int vithip_attention_bf16io_f32math(vithip_stream_t stream, const unsigned short *qkv, unsigned short *out,
                                    int n_images, int tokens, int heads);
/* As vithip_attention_f32 / vithip_attention_bf16io, but only the first q_rows query rows of every image are computed
 * and stored (rows q_rows.. of `out` are left untouched); tokens <= 224.  q_rows = 1 is the class token.  Non-finite values in one
 * image's rows reach only that image's outputs; all other outputs have the bits of the same launch on clean data. */
int vithip_attention_f32_rows(vithip_stream_t stream, const float *qkv, float *out, int n_images, int tokens, int heads,
                              int q_rows);
int vithip_attention_bf16io_rows(vithip_stream_t stream, const unsigned short *qkv, unsigned short *out, int n_images,
                                 int tokens, int heads, int q_rows);
/* As vithip_attention_bf16io (q_rows = tokens) / _rows (q_rows < tokens: tokens <= 224), for Q columns that already hold
 * VITHIP_QSCALE * q: the kernels then scale no score.  Non-finite values in one image's rows reach only that image's outputs; all
 * other outputs have the bits of the same launch on clean data. */
int vithip_attention_bf16io_qscaled(vithip_stream_t stream, const unsigned short *qkv, unsigned short *out, int n_images,
                                    int tokens, int heads, int q_rows);
/*
 * The attention entries for any accepted head_dim: 64, and every multiple of 8 from 72 to 128 (csrc/vit_attention_hd.hip).  The
 * layout is the one of vithip_attention_f32 / _bf16io with 64 replaced by head_dim: qkv [n*T][3*heads*head_dim], columns [Q | K | V],
 * head h = columns head_dim*h.. of each; out [n*T][heads*head_dim]; scores = q.k / sqrtf(head_dim), row softmax with max
 * subtraction, out = P.V.  Only the first q_rows (1..tokens) query rows of every image are computed and stored.
 *   head_dim == 64: the bits and the limits of vithip_attention_f32 / _f32_rows, _bf16io / _bf16io_rows / _bf16io_qscaled
 *     (q_rows < tokens needs tokens <= 224).
 *   otherwise: any tokens >= 1 and any q_rows, heads <= 65535; fp32 arithmetic for fp32, for bf16 both products on the bf16 matrix
 *     pipe with fp32 scores and softmax and the output rounded to bf16 once.  Nothing is read behind column head_dim of a head's slice.
 *   The kernels behind both: the table at the head of csrc/vit_attention.hip.
 *   q_scaled = 1 (bf16): the Q columns hold vithip_qscale(head_dim) * q; p = exp2(q.k - max), no further scaling.
 * No atomics; an image's output bits depend on neither the batch size nor its place in the batch; non-finite values in one image's
 * rows reach only that image's outputs; nothing is written outside rows 0..q_rows-1 of an image or behind column heads*head_dim.
 * hipErrorInvalidValue, nothing launched: any other head_dim, NULL or not 16-byte aligned pointers, non-positive sizes,
 * q_rows outside 1..tokens, q_scaled other than 0 / 1.
 */
int vithip_attention_f32_hd(vithip_stream_t stream, const float *qkv, float *out, int n_images, int tokens, int heads, int head_dim,
                            int q_rows);
int vithip_attention_bf16io_hd(vithip_stream_t stream, const unsigned short *qkv, unsigned short *out, int n_images, int tokens,
                               int heads, int head_dim, int q_rows, int q_scaled);
/* vithip_attention_f32_hd's layout, arguments and guarantees at head_dim 64 (any other head_dim: hipErrorInvalidValue), any tokens >= 1
 * and any q_rows, heads <= 65535, with both products on the bf16 matrix pipe: every fp32 operand (Q, K, V and the softmax weights) is
 * split into three bf16 pieces and each fp32 product becomes the six piece products of rank <= 2, added small terms first (the
 * arithmetic of vithip_gemm_args.arith = 1).  Scores, softmax and accumulation are fp32; the result differs from fp32 arithmetic in
 * the last bits.  A row's bits depend on neither the batch size, nor the image's place in the batch, nor q_rows. */
int vithip_attention_f32_split(vithip_stream_t stream, const float *qkv, float *out, int n_images, int tokens, int heads, int head_dim,
                               int q_rows);
/* (float)((1 / sqrt((double)head_dim)) * log2(e)): the factor of the scores' exponent, softmax(q.k / sqrt(hd)) = 2^(qscale q.k -
 * max) / sum; vithip_qscale(64) has the bits of VITHIP_QSCALE.  0.0f for a head_dim the kernels refuse. */
float vithip_qscale(int head_dim);
/* Patch embedding on the bf16 matrix pipe (same result layout as vithip_patch_embed_f32: x[n][tokens][D] fp32 with
 * class token and pos_emb applied; ViT_seq.c:25-101): the images are cut into bf16 patch rows
 * (patches16: workspace of n * (img/patch)^2 * chans*patch^2 bf16), multiplied with the bf16 conv weight
 * conv_w16 [D][chans*patch^2] with fp32 accumulation, bias / pos_emb / class token added in fp32.
 * Needs chans*patch^2 % 64 == 0, chans*patch^2 >= 128, D % 4 == 0, patch % 8 == 0. */
int vithip_patch_embed_bf16(vithip_stream_t stream, const float *images, const unsigned short *conv_w16,
                            const float *conv_b, const float *cls, const float *pos, float *x,
                            unsigned short *patches16, int n_images, int img_size, int patch_size, int in_chans,
                            int embed_dim);
/* The same result as ONE implicit GEMM that reads the NCHW fp32 images directly (pixels rounded to bf16 in the A-tile loader; no
 * staging pass, no workspace).  A tested alternative, not the engine's default: 2.4 ms against 1.0 ms at batch 2048, bound by
 * the fp32 pixel bytes every 128-wide N tile re-reads (csrc/vit_patch_embed_bf16.hip).
 * Needs patch % 4 == 0, chans*patch^2 % 32 == 0, img % 4 == 0, n * patches <= 2^24. */
int vithip_patch_embed_bf16_implicit(vithip_stream_t stream, const float *images, const unsigned short *conv_w16,
                                     const float *conv_b, const float *cls, const float *pos, float *x,
                                     int n_images, int img_size, int patch_size, int in_chans, int embed_dim);
/* dst[i] = bf16(src[i]), round to nearest even; count % 4 == 0. */
int vithip_f32_to_bf16(vithip_stream_t stream, const float *src, unsigned short *dst, size_t count);

/*
 * Patch embedding straight from NCHW images (implicit GEMM over the 16x16 patches), with the
 * embedding tail fused into the store:
 *   x[img][0][:]     = cls[:] + pos[0][:]
 *   x[img][1+p][:]   = conv_bias[:] + sum_{ic,kh,kw} image * conv_w + pos[1+p][:]
 * images: [n][C][S][S]; conv_w: [D][C*P*P]; x: [n][T][D], T = (S/P)^2 + 1.
 * Two kernels: geometries with P % 4 == 0, S % 4 == 0 and C*P*P % 32 == 0 (images and conv_w 16-byte aligned) take the 16-byte gather
 * of csrc/vit_gemm.hip; every other geometry goes to vithip_patch_embed_f32_general below and follows its rules.
 */
int vithip_patch_embed_f32(vithip_stream_t stream, const float *images, const float *conv_w,
                           const float *conv_b, const float *cls, const float *pos, float *x,
                           int n_images, int img_size, int patch_size, int in_chans, int embed_dim);
/*
 * The same result for any even geometry (csrc/vit_patch_embed_general.hip; DINOv2's 14 x 14 patches, K = C*P*P = 588): P even, S even,
 * S % P == 0, C >= 1, D % 4 == 0, n * (S/P)^2 <= 2^24; images and conv_w 8-byte aligned (they are read 8 bytes at a time, straight
 * from the NCHW images and from conv_w [D][K] as it lies: no staging pass, no workspace).  Anything else (an odd patch or image
 * included, NULL pointers): hipErrorInvalidValue, nothing launched.  fp32 MFMA with k ascending from a zero accumulator, then + bias,
 * then + pos: an output row's bits do not depend on the batch or on the image's place in it.  The K tail of the last K step is
 * zero-filled on chip; nothing is read past the last weight row, the last image or column K of a weight row.  This entry always runs
 * the general kernel, also at geometries the 16-byte gather takes (there the two agree to rounding, not to the bit: the gather's k
 * order inside a K step is another).
 */
int vithip_patch_embed_f32_general(vithip_stream_t stream, const float *images, const float *conv_w,
                                   const float *conv_b, const float *cls, const float *pos, float *x,
                                   int n_images, int img_size, int patch_size, int in_chans, int embed_dim);
/*
 * The three embeddings the engine runs, for a model with num_registers register tokens between the class token and the patch tokens
 * (DINOv2 `_reg4`; transformers' Dinov2WithRegistersEmbeddings).  prefix: [(1 + num_registers)][D], the class token, then the
 * register tokens; pos: [(S/P)^2 + 1][D] as ever -- registers take no position embedding; x: [n][T][D], T = 1 + num_registers + (S/P)^2:
 *   x[img][0][:]                     = prefix[0] + pos[0]
 *   x[img][1 + r][:]                 = prefix[1 + r]                         r = 0..num_registers-1, the bits of prefix
 *   x[img][1 + num_registers + p][:] = conv_b + patch_p . conv_w + pos[1 + p]
 * Everything else is the entry of the same name without _reg, which is this one at num_registers == 0, bit for bit; a patch row has
 * the same bits at every num_registers (k ascending; neither the batch nor the image's place in it changes a row), and nothing is
 * written outside x[n][T][D].  hipErrorInvalidValue, nothing launched: num_registers outside 0..VITHIP_MAX_REGISTER_TOKENS,
 * n * T >= 2^31, and whatever the plain entry refuses.
 */
#define VITHIP_MAX_REGISTER_TOKENS 16
int vithip_patch_embed_f32_reg(vithip_stream_t stream, const float *images, const float *conv_w, const float *conv_b,
                               const float *prefix, const float *pos, float *x, int n_images, int img_size, int patch_size,
                               int in_chans, int embed_dim, int num_registers);
int vithip_patch_embed_f32_general_reg(vithip_stream_t stream, const float *images, const float *conv_w, const float *conv_b,
                                       const float *prefix, const float *pos, float *x, int n_images, int img_size, int patch_size,
                                       int in_chans, int embed_dim, int num_registers);
int vithip_patch_embed_bf16_reg(vithip_stream_t stream, const float *images, const unsigned short *conv_w16, const float *conv_b,
                                const float *prefix, const float *pos, float *x, unsigned short *patches16, int n_images,
                                int img_size, int patch_size, int in_chans, int embed_dim, int num_registers);

/*
 * y[r][0..dim) = (x[r] - mean) * inv_std * gamma + beta for rows r = 0..rows-1 where row r
 * starts at x + r*ldx (ldx lets the final LayerNorm touch only the class-token rows).
 * mean/var as ViT_seq.c:103-121: var = E[x^2] - mean^2, inv_std = 1/sqrtf((double)var + 1e-6).
 * dim % 4 == 0, dim <= 2048; ldx, ldy >= dim and % 4 == 0; x, y, gamma, beta 16-byte aligned (vithip_layernorm_f32_bf16out: the same).
 * Non-finite values in one row of x reach only that row of y; all other rows have the bits of the same launch on clean data.
 */
int vithip_layernorm_f32(vithip_stream_t stream, const float *x, size_t ldx, float *y, size_t ldy,
                         const float *gamma, const float *beta, int rows, int dim);
/* x and y: either the SAME rows (y == x and ldy == ldx: in place, the bits of the out-of-place call -- a wave holds its whole row in
 * registers before it stores any of it) or disjoint; rows that overlap in any other way are refused (both layernorm entries and
 * their siblings; the bf16 store is never in place). */
int vithip_layernorm_f32_eps(vithip_stream_t stream, const float *x, size_t ldx, float *y, size_t ldy,
                             const float *gamma, const float *beta, int rows, int dim, double eps);

/*
 * SwiGLU: the gate of a gated MLP (csrc/vit_swiglu.hip; Dinov2SwiGLUFFN of transformers, SwiGLUFFNFused of DINOv2).
 *     h[r][j] = silu(u[r][j]) * u[r][H + j]   for r < rows, j < H,   silu(g) = g / (1 + exp(-g))
 * u: [rows][ldu], the first 2H columns are read (gate | value: what chunk(2, dim=-1) makes of the w12 output);
 * h: [rows][ldh], the first H columns are written and nothing else.
 * Arithmetic, per element with gate g and value v, all fp32, one rounding per step:
 *     e = expf(-g)  (the library expf, within 1 ulp);  s = 1.0f + e;  q = g / s  (IEEE-rounded);  h = q * v
 * and, for g < -87 only, where expf(-g) nears and then passes the end of the fp32 range while silu(g) is still a normal number
 * (silu(-89) = -2.0e-37):
 *     t = expf(0.5f * g);  h = ((g * t) * v) * t          (1 + exp(g) rounds to 1 there)
 * which keeps the result inside 4 ulp + 2^-126 of the exact one over the whole range.  _bf16 widens both inputs to fp32 (exact), does
 * the same and rounds h to bf16 once, to nearest even (the conversion of every other bf16 store).  So: g = +Inf gives v * Inf,
 * g = -Inf gives NaN (as PyTorch's x * sigmoid(x)), a NaN in g or v gives NaN, g < -208 (t underflows) gives -0 * v.
 * Aliasing: exactly in place (h == u and ldh == ldu: the gate half of a row becomes h, the value half keeps its bits) or disjoint
 * address ranges; any other overlap is hipErrorInvalidValue.
 * Requirements (anything else: hipErrorInvalidValue, nothing launched): rows >= 1; H >= 4 and H % 4 == 0 (_bf16: 8); ldu >= 2H,
 * ldh >= H, both multiples of 4 (_bf16: 8); u and h 16-byte aligned.  Offsets are 64-bit (rows * ldu may pass 2^31 elements).
 * Values are element-local: a non-finite u[r][j] or u[r][H + j] reaches h[r][j] alone; every other output has the bits of the same
 * launch on clean data.
 */
int vithip_swiglu_f32(vithip_stream_t stream, const float *u, size_t ldu, float *h, size_t ldh, int rows, int H);
int vithip_swiglu_bf16(vithip_stream_t stream, const unsigned short *u, size_t ldu, unsigned short *h, size_t ldh, int rows, int H);

/*
 * Fused scaled-dot-product attention, one workgroup per (image, head) (x blocks of 256 queries when chunked).
 * qkv: [n*T][3*D] rows = tokens, columns [Q | K | V], head h = columns 64h..64h+63 of each.
 * out: [n*T][D].  scores = q.k / sqrtf(64); row softmax with max subtraction; out = P.V.
 * head_dim is 64 here (other head dims: vithip_attention_f32_hd below the bf16 entries); any tokens >= 1.  The kernels by sequence
 * length: the table at the head of csrc/vit_attention.hip.
 * Non-finite values in one image's rows reach only that image's outputs; all other outputs have the bits of the same launch on
 * clean data.
 */
int vithip_attention_f32(vithip_stream_t stream, const float *qkv, float *out,
                         int n_images, int tokens, int heads);

/*
 * probs[r][0..classes) = softmax(logits[r]) (ViT_seq.c:304-324) and the top-1 record
 * (first index of the maximum probability, Main.c:62-70).  top1_label / top1_prob may be NULL.
 */
int vithip_softmax_top1_f32(vithip_stream_t stream, const float *logits, int ld_logits,
                            float *probs, int ld_probs, int *top1_label, float *top1_prob,
                            int rows, int classes);

/*
 * The k best classes of every row as records instead of the probabilities (csrc/vit_topk.hip): the output row of image i is
 *     out[i * ld_out + 0 .. k-1]   the labels (int32), best first
 *     out[i * ld_out + k .. 2k-1]  their scores, as fp32 bit patterns
 * (labels, then bit patterns: the convention of the records in vit_dp.h).  ld_out counts 32-bit words.
 * The score of class c:
 *   VITHIP_SCORE_PROB   the probability vithip_softmax_top1_f32 stores for the same logits row, bit for bit:
 *                       mx = max_c logits[c]; e_c = expf(logits[c] - mx); sum = sum_c e_c in that kernel's order (thread-strided
 *                       partial sums, a wave butterfly, the four waves added 0..3); score = e_c / sum
 *   VITHIP_SCORE_LOGIT  logits[c]
 * Order: slot 0 is the best; slot j holds the best candidate after the one in slot j-1 under the total order "higher score first;
 * among equal scores (==, so -0.0 ties +0.0) the lower label first" -- the first-maximum-wins rule of Main.c:64-68, continued.
 * A class whose score is NaN is not a candidate (+-inf are ordinary values); slots left over when fewer than k candidates exist hold
 * label 0x7fffffff and score -1.0f (PROB) or -INFINITY (LOGIT).  PROB slot 0 is therefore always the (label, prob) pair of
 * vithip_softmax_top1_f32, including its (0x7fffffff, -1.0f) for a row whose probabilities are all NaN.
 * Nothing but the 2k words of each row is written and logits is only read; a row's records depend on that row's logits alone (one
 * workgroup per row, no atomics: reproducible bit for bit whatever rows is and wherever the row sits).
 * hipErrorInvalidValue, before anything is launched: NULL pointers, rows <= 0, k < 1, k > classes, k > VITHIP_MAX_TOPK,
 * ld_logits < classes, ld_out < 2k, an unknown score.
 */
enum { VITHIP_SCORE_PROB = 0, VITHIP_SCORE_LOGIT = 1 };
#define VITHIP_MAX_TOPK 64
int vithip_softmax_topk_f32(vithip_stream_t stream, const float *logits, int ld_logits,
                            int *out, int ld_out /* 32-bit words per row, >= 2k */,
                            int rows, int classes, int k, int score);

/*
 * The model input from 8-bit pixels (csrc/vit_input.hip): src [n][S][S][C] uint8, channels interleaved as image decoders
 * write them -> dst [n][C][S][S] fp32,
 *     dst[i][c][h][w] = ((float)src[i][h][w][c] / 255.0f - mean[c]) / std[c]
 * torchvision's ToTensor() + Normalize(mean, std), every step one fp32 IEEE operation (true divisions): bit for bit what a
 * CPU computes from the same formula.  mean / std: HOST arrays of chans floats, copied into the launch (a captured graph keeps
 * the values of its capture).  Needs 1 <= chans <= 4, n >= 1, S % 4 == 0, src 4-byte and dst 16-byte aligned, every mean[c]
 * finite, every std[c] finite and non-zero; hipErrorInvalidValue otherwise.
 */
int vithip_images_u8_to_f32(vithip_stream_t stream, const unsigned char *src, float *dst, int n, int img_size, int chans,
                            const float *mean, const float *std);

/*
 * The model input from decoded 8-bit images of any size (csrc/vit_preproc.hip): torchvision's evaluation transform
 *     Resize(R) -> CenterCrop(S) -> ToTensor() -> Normalize(mean, std)
 * in one kernel, bit for bit what torchvision computes on the PIL images a dataset hands it.  images: a HOST array of n records,
 * read during the call only (the records travel as kernel arguments, 64 per launch; the call is asynchronous on `stream`); pixels:
 * DEVICE pointer to [height][width][chans] uint8, rows packed, no alignment needed.  dst [n][chans][S][S] fp32, S = img_size.
 *
 * Geometry (Resize with an int, CenterCrop): short, long = min, max(height, width); the shorter side becomes R = resize_shorter,
 * the longer L = (R * long) / short (integer division); width <= height gives a resized image of oh = L, ow = R, otherwise oh = R,
 * ow = L.  top = rne((oh - S) / 2), left = rne((ow - S) / 2), round half to even.  dst pixel (i, j) is pixel (top + i, left + j) of
 * the resized image; only those are computed.
 * Resize (Pillow's Image.resize((ow, oh), BILINEAR), 8 bits per channel).  Per axis (in = source extent, out = resized extent), for
 * resized index xx, in IEEE double without fused multiply-add:
 *     scale = (double)in / out; fs = max(scale, 1.0); support = fs; ss = 1.0 / fs; center = (xx + 0.5) * scale;
 *     xmin = max((int)(center - support + 0.5), 0); xmax = min((int)(center + support + 0.5), in); cnt = xmax - xmin;
 *     w[x] = 1 - a if a < 1 else 0, a = |(x + xmin - center + 0.5) * ss|; ww = sum of w[x] in index order; w[x] /= ww if ww != 0;
 *     k[x] = (int)(0.5 + w[x] * 4194304.0)
 * A pass: acc = 2097152 + sum_x pixel[xmin + x] * k[x] in int32, byte = min(acc >> 22, 255).  The horizontal pass comes first and is
 * rounded to bytes, the vertical pass runs over those bytes; an axis with in == out is skipped.
 * Normalise: the byte u of the vertical pass gives dst[c][i][j] = ((float)u / 255.0f - mean[c]) / std[c] (vithip_images_u8_to_f32).
 *
 * hipErrorInvalidValue, nothing launched: NULL images / dst / mean / std / pixels, n < 1, chans outside 1..4, img_size < 4 or not a
 * multiple of 4, resize_shorter < img_size (torchvision would pad) or > 4096, a height or width outside 1..16384, a source whose
 * shorter side exceeds 64 * resize_shorter, dst not 16-byte aligned, a non-finite mean or std, a zero std.
 */
typedef struct {
    const unsigned char *pixels; /* device, [height][width][chans] */
    int height, width;
} vithip_image_u8;
int vithip_images_u8_resize_crop_to_f32(vithip_stream_t stream, const vithip_image_u8 *images, int n, float *dst, int img_size, int chans,
                                        int resize_shorter, const float *mean, const float *std);
/* The launcher's checks of the records and sizes alone, for callers that must know before they enqueue anything: 0 = accepted,
 * i + 1 = record i is refused, -1 = one of n, img_size, chans, resize_shorter (or a NULL array) is. */
int vithip_images_u8_resize_crop_check(const vithip_image_u8 *images, int n, int img_size, int chans, int resize_shorter);
/*
 * The same transform with the resize filter chosen: the two entries above are the VITHIP_RESIZE_BILINEAR case of these, to the bit.
 * VITHIP_RESIZE_BICUBIC is Pillow's Image.resize((ow, oh), BICUBIC) on 8 bits per channel -- torchvision's
 * Resize(R, interpolation=BICUBIC) on PIL images, the evaluation transform of DINOv2, DINO, DeiT, MAE and timm's vit_* configs -- bit
 * for bit.  Everything is as stated for bilinear above (IEEE double, no fused multiply-add, true divisions; scale, fs, ss, center, xmin,
 * xmax and cnt by the same expressions), except:
 *     support = 2.0 * fs
 *     w[x] = f((x + xmin - center + 0.5) * ss), with a = -0.5 and t = |argument|:
 *            f = ((a + 2.0) * t - (a + 3.0)) * t * t + 1     if t < 1.0
 *            f = (((t - 5) * t + 8) * t - 4) * a             if t < 2.0
 *            f = 0.0                                         otherwise
 *     ww = sum of w[x] in index order; w[x] /= ww if ww != 0.0
 *     k[x] = w[x] < 0 ? (int)(-0.5 + w[x] * 4194304.0) : (int)(0.5 + w[x] * 4194304.0)
 *     a pass: acc = 2097152 + sum_x pixel[xmin + x] * k[x] in int32, byte = min(max(acc >> 22, 0), 255), the shift arithmetic
 * The coefficients are signed, so a pass can leave [0, 255] on both sides and both passes clamp on both.  An output index has at most
 * (int)(4 * fs) + 2 taps (bilinear: (int)(2 * fs) + 2), and the int32 sum cannot overflow: the positive coefficients of an index sum
 * to less than 1.2 * 2^22.
 * Size limit: the same for both filters -- a source's shorter side is at most 64 * resize_shorter (the bicubic kernel keeps coefficient
 * tables of twice the size for it) -- and so are all the other refusals.  An unknown filter: hipErrorInvalidValue, nothing launched,
 * and -1 from the check.
 */
enum { VITHIP_RESIZE_BILINEAR = 0, VITHIP_RESIZE_BICUBIC = 1 };
int vithip_images_u8_resize_crop_to_f32_filter(vithip_stream_t stream, const vithip_image_u8 *images, int n, float *dst, int img_size,
                                               int chans, int resize_shorter, int filter, const float *mean, const float *std);
int vithip_images_u8_resize_crop_check_filter(const vithip_image_u8 *images, int n, int img_size, int chans, int resize_shorter, int filter);

/*
 * Embedding outputs (csrc/vit_pool.hip).  LayerNorm and mean over tokens in ONE pass over x; the LayerNorm rows are never stored:
 *     out[i][0..dim) = gamma * mean_{t in [first_tok, tokens)} ((x_it - mean_it) * inv_std_it) + beta,
 * row (i, t) at x + (i * tokens + t) * ldx, the row statistics those of vithip_layernorm_f32 to the bit.  gamma / beta are applied
 * once, to the pooled normalised rows, for every shape (the mean is linear: it is the mean of the LayerNorm rows up to rounding).
 * Deterministic and position independent: an image's rows are cut into segments of 16 tokens, a workgroup sums one segment in a
 * fixed order, a second small launch adds the segment sums in index order -- the order depends on (tokens, first_tok, dim) only,
 * so an image's output row has the same bits at every place of every batch.  No atomics.
 * l2_normalize = 1: each output row is then divided by max(||row||_2, 1e-12) (vithip_l2_normalize_rows_f32, a third launch).
 * workspace: vithip_layernorm_pool_f32_workspace_floats(images, tokens, first_tok, dim) floats of device scratch, 16-byte aligned,
 * owned by the caller and free again when the launches have run (never more than the images * tokens * dim floats of x's own size).
 * dim % 4 == 0, dim <= 2048, tokens >= 2, 0 <= first_tok < tokens, ldx / ldo >= dim and multiples of 4, pointers 16-byte aligned;
 * hipErrorInvalidValue otherwise.
 */
size_t vithip_layernorm_pool_f32_workspace_floats(int images, int tokens, int first_tok, int dim);
int vithip_layernorm_pool_f32(vithip_stream_t stream, const float *x, size_t ldx, float *out, size_t ldo, const float *gamma,
                              const float *beta, int images, int tokens, int first_tok, int dim, int l2_normalize, float *workspace);
int vithip_layernorm_pool_f32_eps(vithip_stream_t stream, const float *x, size_t ldx, float *out, size_t ldo, const float *gamma,
                                  const float *beta, int images, int tokens, int first_tok, int dim, int l2_normalize, float *workspace,
                                  double eps);
/* x[r][0..dim) /= max(||x[r]||_2, 1e-12) in place (torch.nn.functional.normalize), one workgroup per row: a row's bits do not
 * depend on the number of rows.  dim % 4 == 0, ldx >= dim and a multiple of 4, x 16-byte aligned. */
int vithip_l2_normalize_rows_f32(vithip_stream_t stream, float *x, size_t ldx, int rows, int dim);
/*
 * The other order, pool first and normalise the pooled row (timm's fc_norm heads; csrc/vit_pool.hip):
 *     m[i][0..dim) = (sum_{t in [first_tok, tokens)} x_it) / (tokens - first_tok);   out[i] = LayerNorm(m[i]) with gamma / beta,
 * or out[i] = m[i] itself when gamma and beta are both NULL.  Rows of x as above.  The LayerNorm is the arithmetic of
 * vithip_layernorm_f32 (csrc/vit_row.hpp) on the stored fp32 m[i]:
 *     pool_layernorm(x, gamma, beta) == vithip_layernorm_f32(pool_layernorm(x, NULL, NULL), gamma, beta)   bit for bit.
 * Same structure and contract as vithip_layernorm_pool_f32: segments of 16 token rows per workgroup summed in a fixed order, one
 * small finishing launch (one wave per image) that adds the segment sums in index order, divides and normalises; the order depends
 * on (tokens, first_tok, dim) only, so an image's output row has the same bits at every place of every batch; no atomics; x is read
 * once; a non-finite row of x reaches its own image's row only.  Only out[i][0..dim) is written.
 * workspace: vithip_pool_layernorm_f32_workspace_floats(images, tokens, first_tok, dim) floats, 16-byte aligned, free again when the
 * launches have run.  dim % 4 == 0, dim <= 2048, tokens >= 2, 0 <= first_tok < tokens, ldx / ldo >= dim and multiples of 4, pointers
 * 16-byte aligned, gamma and beta both NULL or both set; hipErrorInvalidValue otherwise, nothing launched.
 */
size_t vithip_pool_layernorm_f32_workspace_floats(int images, int tokens, int first_tok, int dim);
int vithip_pool_layernorm_f32(vithip_stream_t stream, const float *x, size_t ldx, float *out, size_t ldo, const float *gamma,
                              const float *beta, int images, int tokens, int first_tok, int dim, float *workspace);
int vithip_pool_layernorm_f32_eps(vithip_stream_t stream, const float *x, size_t ldx, float *out, size_t ldo, const float *gamma,
                                  const float *beta, int images, int tokens, int first_tok, int dim, float *workspace, double eps);

/*
 * The class token's attention over the tokens of its image (csrc/vit_cls_attention.hip): the softmax row of query 0, stored instead
 * of multiplied with V.  qkv as vithip_attention_f32 / _bf16io read it: rows = tokens, q_row_stride elements from one token row to
 * the next (3 * heads * 64 for packed rows), columns [Q | K | V], head h = columns 64h..64h+63 of each.  For image i and head h, with
 * q = Q[i*tokens][64h..] and k_t = K[i*tokens + t][64h..]:
 *     s_t = (q . k_t) / sqrtf(64);  p_t = expf(s_t - max_t s) / sum_t expf(s_t - max),  t = 0..tokens-1   (ViT_seq.c:156-190, one row)
 * in fp32 for both element types (bf16 elements are widened, never rounded again).  Only the Q of the class rows and K are read.
 *   head_mean = 0: out[i][h][t], a row of heads * tokens floats per image at out + i * ld_out;
 *   head_mean = 1: out[i][t] = (p[0][t] + p[1][t] + ... in head order) / (float)heads, of exactly the bits head_mean = 0 stores.
 * q_scaled = 1 (bf16): the Q columns hold VITHIP_QSCALE * q; p_t = exp2f(q . k_t - max) / sum, no further scaling.
 * Deterministic (no atomics) and position independent: an image's row has the same bits wherever the image sits in whatever batch.
 * Non-finite values in one image's rows reach only that image's row of `out`; all other rows have the bits of the same launch on clean data.
 * Any tokens >= 1 and heads >= 1; head_dim is 64.  Elements of `out` outside the rows are not touched.
 * hipErrorInvalidValue: NULL pointers, non-positive sizes, flags other than 0 / 1, q_row_stride < 3 * heads * 64 or not a multiple
 * of 4 (fp32) / 8 (bf16), ld_out smaller than a row, qkv not 16-byte or out not 4-byte aligned.
 */
int vithip_cls_attention_f32(vithip_stream_t stream, const float *qkv, size_t q_row_stride, float *out, size_t ld_out, int n_images,
                             int tokens, int heads, int head_mean);
int vithip_cls_attention_bf16(vithip_stream_t stream, const unsigned short *qkv, size_t q_row_stride, float *out, size_t ld_out,
                              int n_images, int tokens, int heads, int head_mean, int q_scaled);
/* The same contract with 64 replaced by head_dim (64, or a multiple of 8 from 72 to 128; anything else: hipErrorInvalidValue):
 * s_t = (q . k_t) / sqrtf(head_dim), q_scaled Q columns hold vithip_qscale(head_dim) * q.  head_dim == 64 gives the bits of the
 * entries above; all four are one kernel and one launcher (csrc/vit_cls_attention.hip). */
int vithip_cls_attention_f32_hd(vithip_stream_t stream, const float *qkv, size_t q_row_stride, float *out, size_t ld_out, int n_images,
                                int tokens, int heads, int head_dim, int head_mean);
int vithip_cls_attention_bf16_hd(vithip_stream_t stream, const unsigned short *qkv, size_t q_row_stride, float *out, size_t ld_out,
                                 int n_images, int tokens, int heads, int head_dim, int head_mean, int q_scaled);

/*
 * Rows of the residual stream as an output (csrc/vit_tap.hip): per image the class row, every token, the patch tokens, or the patch
 * tokens as a channel-major map.  x: [images * tokens] rows of dim floats, ldx floats from one row to the next; r(t) = row
 * i * tokens + t of x for image i; f = the LayerNorm of vithip_layernorm_f32 with gamma / beta, or the identity when both are NULL;
 * P = tokens - 1.  Written at out + i * out_image_stride:
 *   VITHIP_TAP_CLS      [dim]          = f(r(0))
 *   VITHIP_TAP_TOKENS   [tokens][dim]  = f(r(0..tokens-1)), class row first
 *   VITHIP_TAP_PATCHES  [P][dim]       = f(r(1..P))
 *   VITHIP_TAP_MAP      [dim][P]       element [d][t - 1] = f(r(t))[d]: [dim][g][g] for a square grid of g x g patches, raster order
 * Normalised values are the bits vithip_layernorm_f32 gives for the same row (one device function holds the arithmetic of both,
 * csrc/vit_row.hpp), unnormalised ones the bits of x; MAP is the exact transpose of PATCHES.  Only the block of each
 * image is written: the floats from its end up to out_image_stride are not touched, so several launches can fill one output row
 * side by side.  MAP goes through an LDS tile and stores runs of up to 32 tokens per channel (16 above dim 1024), as 16 bytes per lane when P % 4 == 0
 * and as 4 bytes per lane otherwise; any P >= 1 is correct.  No atomics; results do not depend on the grid.  Non-finite values in
 * one row of x reach only that row's outputs (the MAP's LDS tile included); all others have the bits of the same launch on clean data.
 * hipErrorInvalidValue, nothing launched: x or out NULL, exactly one of gamma / beta NULL, a non-positive size, an unknown layout,
 * PATCHES or MAP with tokens < 2, dim % 4 != 0 or dim > 2048, ldx < dim or ldx % 4 != 0, out_image_stride % 4 != 0 or smaller than the
 * block, x / out / gamma / beta not 16-byte aligned, images * tokens >= 2^31.
 */
enum { VITHIP_TAP_CLS = 0, VITHIP_TAP_TOKENS = 1, VITHIP_TAP_PATCHES = 2, VITHIP_TAP_MAP = 3 };
int vithip_tap_f32(vithip_stream_t s, const float *x, size_t ldx,          /* [images * tokens] rows, ldx >= dim */
                   float *out, size_t out_image_stride,                     /* floats from one image's block to the next */
                   const float *gamma, const float *beta,                   /* both NULL: copy the rows unnormalised */
                   int images, int tokens, int dim, int layout);
int vithip_tap_f32_eps(vithip_stream_t s, const float *x, size_t ldx, float *out, size_t out_image_stride, const float *gamma,
                       const float *beta, int images, int tokens, int dim, int layout, double eps);
/* The same with `prefix` rows in front of an image's patch rows instead of one (a register model keeps its register tokens between
 * the class token and the patches: prefix = 1 + registers), 1 <= prefix <= tokens, and prefix < tokens for PATCHES and MAP.
 * P = tokens - prefix; CLS is row 0 and TOKENS every row in stored order, as above; PATCHES and MAP read rows prefix..tokens-1, and
 * MAP's 16-byte stores key on this P % 4.  No row in front of `prefix` is read by PATCHES or MAP: a non-finite register row reaches
 * neither.  The two entries above are this one at prefix == 1, bit for bit.  Also refused: prefix outside those bounds. */
int vithip_tap_f32_prefix_eps(vithip_stream_t s, const float *x, size_t ldx, float *out, size_t out_image_stride, const float *gamma,
                              const float *beta, int images, int tokens, int prefix, int dim, int layout, double eps);

/*
 * A position embedding resampled to another patch grid (csrc/vit_pos_resample.hip), so that a checkpoint runs at another input size.
 * src [1 + g_src^2][dim] -> dst [1 + g_dst^2][dim], device pointers: row 0, the class token's embedding, is copied bit for bit; rows
 * 1.. are a g_src x g_src raster of dim-vectors, resampled separably to g_dst x g_dst.
 *   VITHIP_POS_BICUBIC     torch.nn.functional.interpolate(mode="bicubic", align_corners=False, antialias=False): DINO, DeiT, DINOv2
 *   VITHIP_POS_BICUBIC_AA  the same with antialias=True: the default of timm's resample_abs_pos_embed
 * An axis (in = source extent, out = destination extent) is a table: per output index o a first source index, a tap count and fp32
 * weights; the source index of tap k is clamp(first + k, 0, in - 1).  Every operation below is one IEEE fp32 operation, none
 * contracted into a fused multiply-add; scale = (float)in / (float)out.
 *   BICUBIC, A = -0.75f:   r = scale * ((float)o + 0.5f) - 0.5f;  b = floorf(r);  t = r - b;  first = (int)b - 1;  4 taps
 *                          cub1(x) = ((A + 2) * x - (A + 3)) * x * x + 1;   cub2(x) = ((A * x - 5 * A) * x + 8 * A) * x - 4 * A
 *                          w = { cub2(t + 1), cub1(t), cub1(1 - t), cub2(2 - t) }      (a clamped index may repeat: no taps are merged)
 *   BICUBIC_AA, A = -0.5f: support = scale >= 1 ? 2.0f * scale : 2.0f;  inv = scale >= 1 ? 1.0f / scale : 1.0f;
 *                          center = scale * ((float)o + 0.5f);  first = max((int)(center - support + 0.5f), 0);
 *                          count = min((int)(center + support + 0.5f), in) - first;
 *                          w[j] = filter(((float)(j + first) - center + 0.5f) * inv), with x := |x|,
 *                          filter(x) = ((A + 2) * x - (A + 3)) * x * x + 1 for x < 1, (((x - 5) * x + 8) * x - 4) * A for x < 2, else 0;
 *                          w[j] /= w[0] + w[1] + ... (added in index order)
 * With (iy_j, wy_j) the taps of output row y and (ix_i, wx_i) those of output column x:
 *     row_j[d] = sum_i wx_i * src[iy_j][ix_i][d];   dst[y][x][d] = sum_j wy_j * row_j[d]
 * each accumulator starting at 0.0f, taps in order, multiply then add, each rounded.  tests/pos_resample_model.py restates all of it
 * in numpy; it agrees with PyTorch's CPU kernels to a few 1e-6 on values in [-1, 1] (their summation order is another).
 *
 * vithip_pos_resample_table: the table of one axis, on the host (no device needed).  first / count: out ints each; weights: out rows
 * of max_taps floats, the entries behind a row's count zero.  Returns the widest tap count of the axis; with all three arrays NULL
 * it only returns that (to size them).  Negative: an unknown mode, in or out outside 1..256, some but not all arrays NULL, or
 * max_taps smaller than the widest count (the arrays are then partly written).
 * vithip_pos_resample_f32: builds the table (the grids are square: one serves both axes), uploads it and launches ONE kernel that
 * writes every element of dst exactly once.  The table lives for the call only, so unlike the other launchers this one returns when
 * the kernel has run: it synchronises `stream`.  hipErrorInvalidValue, nothing launched: NULL pointers, a grid outside 1..256, dim
 * outside 4..2048 or not a multiple of 4, src or dst not 16-byte aligned, an unknown mode.  src and dst must not overlap.
 */
enum { VITHIP_POS_BICUBIC = 0, VITHIP_POS_BICUBIC_AA = 1 };
int vithip_pos_resample_table(int mode, int in, int out, int *first, int *count, float *weights, int max_taps);
int vithip_pos_resample_f32(vithip_stream_t stream, const float *src, int g_src, float *dst, int g_dst, int dim, int mode);

/*
 * The tail of a dense linear head (csrc/vit_dense.hip): per-pixel labels from the logits of a g x g patch grid.  logits: per image
 * (image_stride floats apart) P = g * g rows of `classes` floats, ld_logits floats from one row to the next, row p the patch p in
 * raster order -- what a GEMM over the patch tokens writes.  out: per image (out_image_stride BYTES apart) out_h x out_w bytes,
 *     out[y][x] = argmax_c  F.interpolate(map_c, size=(out_h, out_w), mode="bilinear", align_corners=False)[y][x]
 * with the arithmetic, per axis (g source cells, `out` destination pixels), in fp32, nothing contracted, every product and sum rounded:
 *     scale = (float)g / (float)out;  src = scale * ((float)dst + 0.5f) - 0.5f, a negative value becomes 0;
 *     i0 = (int)src;  i1 = i0 + (i0 < g - 1);  l1 = src - (float)i0;  l0 = 1.0f - l1
 *     v = l0y * (l0x * v00 + l1x * v01) + l1y * (l0x * v10 + l1x * v11)            v_rc = logits[(i_r(y) * g + i_c(x))][c]
 * A higher v wins; among equal values (==) the lower label; a class whose v is NaN is not a candidate (+-Inf are ordinary values, and
 * 0 * Inf is the NaN IEEE says); a pixel without a candidate gets 255 -- hence classes <= 255.  tests/dense_head_model.py restates it.
 * No full-resolution logit is stored anywhere: a workgroup stages its tile's window of cells in LDS, walks the classes with a
 * running best per pixel and stores bytes.  Any g >= 1 (g * g an int), any out_h, out_w in 1..4096 and any classes in 1..255 runs: a
 * window that outgrows the LDS budget (out <= g) is walked in slices of classes, then the tile shrinks.  Only the out_h * out_w bytes
 * of each image are written, through byte stores: out needs no alignment.  No atomics; results do not depend on the grid; an image's
 * labels depend on that image's logits alone.
 * hipErrorInvalidValue, nothing launched: NULL pointers, images < 1, g < 1, classes outside 1..255, out_h or out_w outside 1..4096,
 * ld_logits < classes, image_stride < (P - 1) * ld_logits + classes, out_image_stride < out_h * out_w.
 *
 * vithip_dense_grid_f32: the same logits channel-major, out per image (out_image_stride FLOATS apart) [classes][P] = [classes][g][g],
 * out[c][p] = logits[p][c] bit for bit.  (Not vithip_tap_f32's MAP: that one skips a class row and needs dim % 4 == 0 and 16-byte
 * aligned rows, which a head of 21 or 150 classes does not give.)  The same refusals, with out_image_stride < classes * P.
 */
int vithip_dense_upsample_argmax_f32(vithip_stream_t stream, const float *logits, int ld_logits, size_t image_stride, unsigned char *out,
                                     size_t out_image_stride, int images, int g, int classes, int out_h, int out_w);
int vithip_dense_grid_f32(vithip_stream_t stream, const float *logits, int ld_logits, size_t image_stride, float *out,
                          size_t out_image_stride, int images, int g, int classes);

#ifdef __cplusplus
}
#endif
#endif /* VIT_HIP_KERNELS_H */
