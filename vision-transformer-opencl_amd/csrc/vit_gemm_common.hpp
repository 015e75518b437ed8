// csrc/vit_gemm_common.hpp -- pieces shared by the fp32 GEMM kernels (vit_gemm.hip, vit_gemm_persistent.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "vit_hip_kernels.h"
#include "vit_split3.hpp"

namespace vitgemm {


typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int KALIGN = 32;  // K must be a multiple of this (covers every K step below)

enum { A_DENSE = 0, A_PATCHES = 1 };
// epilogue codes beyond the public three (vit_hip_kernels.h): the consumer side of the LayerNorm fold (ln_rows / ln_colsum set)
// and the producer side: the residual epilogue that also leaves the row sums of what it stored (row_partials set; persistent walk)
enum { EPI_BIAS_LN = 3, EPI_BIAS_GELU_LN = 4, EPI_RESIDUAL_STATS = 5, EPI_BIAS_QGELU_LN = 7 /* 6 is VITHIP_EPI_BIAS_QGELU */ };
// compile-time properties of an epilogue code: fold consumer; which activation follows the bias
constexpr bool epi_is_fold(int epi) { return epi == EPI_BIAS_LN || epi == EPI_BIAS_GELU_LN || epi == EPI_BIAS_QGELU_LN; }
constexpr bool epi_is_gelu(int epi) { return epi == VITHIP_EPI_BIAS_GELU || epi == EPI_BIAS_GELU_LN; }
constexpr bool epi_is_qgelu(int epi) { return epi == VITHIP_EPI_BIAS_QGELU || epi == EPI_BIAS_QGELU_LN; }

// ---- host side: a run-time epilogue code -> a kernel's template argument ----------------------------------------------------
// f(std::integral_constant<int, E>) for the E among EPIS... that equals `epilogue`, and its result; hipErrorInvalidValue for a code
// that is none of them.  Only the listed codes are instantiated: a launcher's list IS the set of kernels it builds.
template <int... EPIS, typename F>
int with_epilogue(int epilogue, F &&f) {
    int rc = static_cast<int>(hipErrorInvalidValue);
    (void)((epilogue == EPIS && (rc = f(std::integral_constant<int, EPIS>{}), true)) || ...);
    return rc;
}
template <int... EPIS> struct EpilogueList {};
template <int... EPIS, typename F>
int with_epilogue(EpilogueList<EPIS...>, int epilogue, F &&f) { return with_epilogue<EPIS...>(epilogue, f); }
// What each kernel family takes (a new epilogue is added to the lists of the kernels that implement it, nowhere else):
// one tile per workgroup (vit_gemm.hip) and the latency tile (vit_gemm_latency.hip)
using TileEpilogues = EpilogueList<VITHIP_EPI_BIAS, VITHIP_EPI_BIAS_GELU, VITHIP_EPI_BIAS_RESIDUAL, EPI_BIAS_LN, EPI_BIAS_GELU_LN,
                                   VITHIP_EPI_BIAS_QGELU, EPI_BIAS_QGELU_LN>;
// the persistent walk (vit_gemm_persistent.hip): those, and the residual epilogue that leaves the row sums
using WalkEpilogues = EpilogueList<VITHIP_EPI_BIAS, VITHIP_EPI_BIAS_GELU, VITHIP_EPI_BIAS_RESIDUAL, EPI_BIAS_LN, EPI_BIAS_GELU_LN,
                                   VITHIP_EPI_BIAS_QGELU, EPI_BIAS_QGELU_LN, EPI_RESIDUAL_STATS>;
// bf16: the two-stage kernel (vit_gemm_bf16.hip) and the ping-pong kernel with a LayerNorm folded in (vit_gemm_bf16_pp.hip)
using Bf16Epilogues = EpilogueList<VITHIP_BF16_EPI_BF16, VITHIP_BF16_EPI_BF16_GELU, VITHIP_BF16_EPI_BF16_QGELU, VITHIP_BF16_EPI_F32_RESIDUAL>;
// bf16: the ping-pong kernel without a fold, which is also the GEMM of vithip_patch_embed_bf16
using Bf16PingPongEpilogues = EpilogueList<VITHIP_BF16_EPI_BF16, VITHIP_BF16_EPI_BF16_GELU, VITHIP_BF16_EPI_BF16_QGELU,
                                           VITHIP_BF16_EPI_F32_RESIDUAL, VITHIP_BF16_EPI_F32_EMBED>;

// p.tiles_m x p.tiles_n tiles of bm x bn over p.M x p.N, and the workgroups of the launch: one per tile, or, for a persistent walk,
// at most `wgs` of them
template <typename Params>
int set_tile_grid(Params &p, int bm, int bn, int wgs = 0) {
    p.tiles_m = (p.M + bm - 1) / bm;
    p.tiles_n = (p.N + bn - 1) / bn;
    const int total = p.tiles_m * p.tiles_n;
    return wgs > 0 && wgs < total ? wgs : total;
}

// what the embedding kernels' token-row remap takes: a register count the ABI allows, and token rows of x that are ints
inline bool embed_rows_ok(int n_images, int patches, int registers) {
    return registers >= 0 && registers <= VITHIP_MAX_REGISTER_TOKENS && (long long)n_images * (patches + 1 + registers) <= 0x7fffffffLL;
}
// vit_gemm.hip: the rows in front of the patch rows of every image of x [n_images][tokens][dim], for every patch embedding:
// x[img][0][:] = prefix[0] + pos[0] (the class row), x[img][1 + r][:] = prefix[1 + r] for the `registers` register tokens
int launch_prefix_rows(hipStream_t stream, const float *prefix, const float *pos, float *x, int n_images, int tokens, int registers, int dim);

struct GemmParams {
    const float *A;
    const float *W;
    const float *bias;
    const float *R;
    float *C;
    int lda, ldw, ldr, ldc;
    int M, N, K;
    int tiles_m, tiles_n;
    int group_m;     // tile rows per L2 group (see tile_coords)
    // A_PATCHES only
    const float *pos;
    unsigned long long *dbg;  // DBG == 5: 8 stamps per workgroup
    int patches;     // patches per image (G*G)
    int grid;        // G = img/patch
    int patch;       // P
    int img;         // S
    int chans;       // C
    int prefix;      // rows in front of an image's patch rows in C: 1 (the class token) + the register tokens
    // persistent kernel, helper pieces (vit_gemm_persistent.hip): workspace lent by the caller (NULL: off), piece length
    void *sk_ws;     // device side of the workspace handle: [4 KB of flags and counters][sk_slots x 64 KB]
    int sk_slots;
    int sk_x;
    int sk_late;     // tests: helpers run their pieces last (vithip_gemm_args.handover_test)
    int sk_gen;      // launch number on this workspace (1 .. 2^28): flag words of other generations read as empty
    // LayerNorm fold, consumer side (EPI_BIAS_LN, EPI_BIAS_GELU_LN): (rstd, mean) per row of A, column sums of the folded W
    const float *ln_rows;
    const float *ln_colsum;
    // producer side (EPI_RESIDUAL_STATS): [N / 64][M][2] partial (sum, sum of squares) of the stored rows per 64-column strip;
    // stats_in_epilogue: set by the dispatcher when the kernel it chose writes them (the caller then only finalises)
    float *row_partials;
    int stats_in_epilogue;
    // the pre-split weight image (vithip_gemm_args.w_split; NULL: split W on the fly): read by the persistent split walk only
    // (128 x 128 tiles, or 64 x 256: walk_tile())
    const void *w_split;
};

// erf(x) = sign(x) * (1 - exp(t*q(t))), t = min(|x|, 4), q = degree-7 minimax fit of log(erfc(t))/t
// (fitted against scipy.special.erf; max |error| 1.2e-7 when evaluated in fp32, i.e. fp32 rounding
// noise -- libm's erff costs ~45 VALU instructions and two divergent branches per element, which made
// the fc1 epilogue 10 % of that GEMM; this form is 14 straight-line instructions).
__device__ __forceinline__ float erf_fp32(float x) {
    const float t = fminf(fabsf(x), 4.0f);
    float q = -3.144179208902642e-05f;
    q = fmaf(q, t, 3.0881378916092217e-04f);
    q = fmaf(q, t, -1.0324339382350445e-03f);
    q = fmaf(q, t, -5.368884885683656e-04f);
    q = fmaf(q, t, 1.95839274674654e-02f);
    q = fmaf(q, t, -1.0291960090398788e-01f);
    q = fmaf(q, t, -6.36597752571106e-01f);
    q = fmaf(q, t, -1.128380298614502f);
    const float e = __builtin_amdgcn_exp2f(q * t * 1.4426950408889634f);  // v_exp_f32
    return copysignf(1.0f - e, x);
}

// GELU of the reference: 0.5f * x * (1.0f + erff(x / sqrtf(2.0f)))  (ViT_seq.c:231-233)
__device__ __forceinline__ float gelu_erf(float x) {
    return 0.5f * x * (1.0f + erf_fp32(x * 0.70710678118654752440f));
}

// GELU of 8 values in lock-step.  One erf is a chain of ~20 DEPENDENT VALU instructions; hipcc
// schedules consecutive calls one chain after the other, and a dependent fp32 op beside a busy matrix
// pipe issues every ~13 cycles (measured: 19k cycles for the 64 values of a lane, 9 % of fc1).  Eight
// chains advanced together -- the scheduling fences keep the compiler from re-serialising them --
// issue back to back.
__device__ __forceinline__ void gelu_erf_x8(float (&y)[8]) {
    // the same arithmetic as gelu_erf() value by value (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 round like their scalar
    // forms), two values per instruction where a packed form exists: the polynomial, the scalings and the final products --
    // 21 VALU instructions per pair instead of 38.  Every one of them is paid for in fp32 matrix-pipe time (item 4 of DESIGN 4.1).
    typedef float v2 __attribute__((ext_vector_type(2)));
    v2 yy[4], u[4], t[4], q[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        yy[v] = v2{y[2 * v], y[2 * v + 1]};
        u[v] = yy[v] * v2{0.70710678118654752440f, 0.70710678118654752440f};
        t[v] = v2{fminf(fabsf(u[v][0]), 4.0f), fminf(fabsf(u[v][1]), 4.0f)};
        q[v] = __builtin_elementwise_fma(v2{-3.144179208902642e-05f, -3.144179208902642e-05f}, t[v],
                                         v2{3.0881378916092217e-04f, 3.0881378916092217e-04f});
    }
    __builtin_amdgcn_sched_barrier(0);
    constexpr float c[6] = {-1.0324339382350445e-03f, -5.368884885683656e-04f, 1.95839274674654e-02f,
                            -1.0291960090398788e-01f, -6.36597752571106e-01f, -1.128380298614502f};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
#pragma unroll
        for (int v = 0; v < 4; ++v) q[v] = __builtin_elementwise_fma(q[v], t[v], v2{c[k], c[k]});
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int v = 0; v < 4; ++v) q[v] = q[v] * t[v] * v2{1.4426950408889634f, 1.4426950408889634f};
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int v = 0; v < 4; ++v) q[v] = v2{__builtin_amdgcn_exp2f(q[v][0]), __builtin_amdgcn_exp2f(q[v][1])};
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const v2 e = v2{1.0f, 1.0f} - q[v];
        const v2 sgn = v2{copysignf(e[0], u[v][0]), copysignf(e[1], u[v][1])};
        const v2 r = v2{0.5f, 0.5f} * yy[v] * (v2{1.0f, 1.0f} + sgn);
        y[2 * v] = r[0];
        y[2 * v + 1] = r[1];
    }
}

// GELU for a bf16 destination, two values per instruction (v_pk_fma_f32).
//   gelu(y) = max(y, 0) - h(|y|),   h = 0.5 |y| erfc(|y|/sqrt2) = t * exp2(Q(t)),  t = min(|y|, 4 sqrt2),
//   Q(t) = log2(erfc(t/sqrt2)) - 1 as a degree-6 polynomial in |y| itself (the fit on [0,4] of erfc's argument with the
//   powers of 1/sqrt2 folded into the coefficients: no scaling multiply, and |y| is a source modifier of the v_min).
// Max abs error 4.7e-6, at most 4.4 % of half a bf16 ulp of the result for y >= -4 sqrt 2; below it an absolute 4.4e-8 (t is clamped:
// the result is the constant -t exp2(Q(t)) = -4.36e-8 where gelu tends to 0, so no relative figure holds there; tests/test_bf16_gemm_model.py
// measures both on a step-by-step emulation): invisible after the bf16
// rounding that follows, at 6.5 VALU instructions per value (6 + 1 v_pk_fma_f32, v_min, v_max, v_exp_f32 per pair and
// value) instead of 19 for the fp32-accurate form above
// (ViT_seq.c:231-233 is the fp32 definition; the bf16 path's parity bar is in tests/test_gpu_bf16.py).
// max(y, 0) that stays non-finite for a non-finite y: v_min / v_max return their OTHER operand for a NaN, so t and the maximum alone
// turned a NaN row of the GEMM into finite values.  y * 0 is +-0 for a finite y (max + (+-0) is max bit for bit, +0 + -0 = +0) and
// NaN for NaN and +-Inf: one v_pk_fma_f32 per pair, off the polynomial's dependent chain.
__device__ __forceinline__ f32x2 relu_keep_nan(f32x2 y) {
    return __builtin_elementwise_fma(y, f32x2{0.f, 0.f}, __builtin_elementwise_max(y, f32x2{0.f, 0.f}));
}

// NP pairs advanced TOGETHER (the scheduling fences keep hipcc from putting the chains back one after the other):
// one pair is a chain of dependent v_pk_fma_f32, and on gfx950 a packed fma that reads the previous one's result needs a wait state --
// hipcc fills it with `s_nop 0`, 5 per pair in the one-pair form (1,255 in the GELU kernel: a quarter of its vector issue slots beside
// the 9 v_pk_fma_f32, 2 v_exp_f32, 4 v_min / v_max and the conversion of a pair).  With a second chain in between there is nothing to pad.
template <int NP>
__device__ __forceinline__ void gelu_bf16_lockstep(f32x2 (&y)[NP]) {
    constexpr float kClamp = 5.656854249492381f;  // 4 sqrt2
    constexpr float c[7] = {-1.000037431716919f,   -1.1505244970321655f,   -0.4605136811733246f,  -0.05179140716791153f,
                            0.007414536084979773f, -0.0006474481779150665f, 2.524326555430889e-05f};
    f32x2 t[NP], q[NP];
#pragma unroll
    for (int v = 0; v < NP; ++v) {
        t[v] = f32x2{fminf(__builtin_fabsf(y[v].x), kClamp), fminf(__builtin_fabsf(y[v].y), kClamp)};
        q[v] = __builtin_elementwise_fma(f32x2{c[6], c[6]}, t[v], f32x2{c[5], c[5]});
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 4; k >= 0; --k) {
#pragma unroll
        for (int v = 0; v < NP; ++v) q[v] = __builtin_elementwise_fma(q[v], t[v], f32x2{c[k], c[k]});
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int v = 0; v < NP; ++v) q[v] = f32x2{__builtin_amdgcn_exp2f(q[v].x), __builtin_amdgcn_exp2f(q[v].y)};
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int v = 0; v < NP; ++v) y[v] = __builtin_elementwise_fma(-t[v], q[v], relu_keep_nan(y[v]));
}

// QuickGELU (CLIP): q(y) = y / (1 + exp(-1.702 y)), PyTorch's x * torch.sigmoid(1.702 * x).  The one sequence of every GEMM kernel,
// fp32 and bf16 alike (include/vit_hip_kernels.h states it):
//     t = y * QGELU_K         v_mul_f32     QGELU_K = fp32(-1.702 * log2 e)
//     e = exp2(t)             v_exp_f32
//     d = 1 + e               v_add_f32
//     r = 1 / d               v_rcp_f32
//     q = y * r               v_mul_f32
// Five dependent steps against ~20 of gelu_erf.  +Inf: e = 0, r = 1, q = +Inf.  -Inf: e = Inf, r = 0, q = -Inf * 0 = NaN (as PyTorch).
// NaN: NaN.  A large negative finite y: e overflows to Inf (or d is past 2^126 and v_rcp_f32 flushes its subnormal result), r = 0,
// q = -0 -- never NaN: only an infinite y meets the zero.
constexpr float QGELU_K = -2.4554669595930157f;
__device__ __forceinline__ float quick_gelu(float y) {
    const float e = __builtin_amdgcn_exp2f(y * QGELU_K);
    return y * __builtin_amdgcn_rcpf(1.0f + e);
}
// The same values for NP pairs advanced TOGETHER, as gelu_bf16_lockstep / gelu_erf_x8 do it: the multiplies and the add in their packed
// forms (v_pk_mul_f32 / v_pk_add_f32 round like the scalar ones), v_exp_f32 and v_rcp_f32 -- quarter-rate, one value each -- of all
// the chains back to back behind the scheduling fences instead of one chain's exp waiting for its own rcp.
template <int NP>
__device__ __forceinline__ void quick_gelu_lockstep(f32x2 (&y)[NP]) {
    f32x2 t[NP];
#pragma unroll
    for (int v = 0; v < NP; ++v) t[v] = y[v] * f32x2{QGELU_K, QGELU_K};
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int v = 0; v < NP; ++v) t[v] = f32x2{__builtin_amdgcn_exp2f(t[v].x), __builtin_amdgcn_exp2f(t[v].y)};
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int v = 0; v < NP; ++v) t[v] = f32x2{1.0f, 1.0f} + t[v];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int v = 0; v < NP; ++v) t[v] = f32x2{__builtin_amdgcn_rcpf(t[v].x), __builtin_amdgcn_rcpf(t[v].y)};
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int v = 0; v < NP; ++v) y[v] = y[v] * t[v];
}
__device__ __forceinline__ void quick_gelu_x8(float (&y)[8]) {
    f32x2 yy[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) yy[v] = f32x2{y[2 * v], y[2 * v + 1]};
    quick_gelu_lockstep<4>(yy);
#pragma unroll
    for (int v = 0; v < 4; ++v) y[2 * v] = yy[v].x, y[2 * v + 1] = yy[v].y;
}

// Workgroup id -> tile id such that ids sharing an XCD (id % 8) get consecutive tiles.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, rem = nwg & 7;
    const int xcd = bid & 7, idx = bid >> 3;
    const int base = xcd < rem ? xcd * (q + 1) : rem * (q + 1) + (xcd - rem) * q;
    return base + idx;
}

// Tile id -> (tm, tn).  Tiles are walked in groups of `group_m` tile rows: inside a group the id
// runs down the rows first, then across the columns, so the ~64 workgroups resident on one XCD
// cover a compact group_m x (64/group_m) block of tiles and share both their A row-panels and their
// W column-panels through that XCD's 4 MB L2 (instead of sweeping all of W per A panel).
__device__ __forceinline__ void tile_coords(int tile, int tiles_m, int tiles_n, int group_m, int &tm, int &tn) {
    const int per_group = group_m * tiles_n;
    const int g = tile / per_group, in_g = tile - g * per_group;
    const int first = g * group_m;
    const int rows = tiles_m - first < group_m ? tiles_m - first : group_m;
    tn = in_g / rows;
    tm = first + (in_g - tn * rows);
}


// ---- three-piece split: fp32 products on the bf16 matrix pipe (vithip_gemm_args.arith = 1) ----------------
// Every fp32 operand x (A and W alike) is staged as three bf16 pieces, each rounded to nearest even:
//     hi = bf16(x),  mid = bf16(x - hi),  lo = bf16(x - hi - mid),   x == hi + mid + lo exactly
// (both differences are exact in fp32 and the last remainder has at most 8 significant bits).  a . w is then the sum of the
// six piece products of rank <= 2 (mid.lo, lo.mid and lo.lo, below ~2^-26 |a.w|, are dropped); a bf16 x bf16 product is exact
// in fp32.  One v_mfma_f32_32x32x16_bf16 per piece pair and 16-deep K step (1/16 of the cycles of v_mfma_f32_32x32x2_f32 per
// product): 6/16 of the fp32 instruction's matrix time.  It writes the 32x32 accumulator layout of v_mfma_f32_32x32x2_f32, so
// every epilogue above and below is shared.  Every output adds its K steps in ascending order and, inside a step, the six
// products small terms first in SPLIT_TERMS order, into one accumulator: every tile shape gives the same bits, and A = I gives
// W exactly (lo, + mid, + hi: each partial sum exact).
enum { ARITH_F32 = 0, ARITH_SPLIT3 = 1 };
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
constexpr int SPLIT_BK = 16;  // K step of the split kernels
// LDS row of the split kernels: [hi 16 x bf16 | mid 16 | lo 16 | 16 bytes of padding] = 28 dwords.  A ds_read_b128 of 16
// consecutive rows (one piece, one half of the K step) then touches 16 distinct 4-bank slots: conflict-free like the fp32 rows.
constexpr int SPLIT_LD = 28;  // floats
// The pieces themselves, their arithmetic and the order of the six products: vit_split3.hpp (shared with the attention kernel).
using vitsplit::SPLIT_TERM_A;
using vitsplit::SPLIT_TERM_W;
using vitsplit::bf16_to_f32;
using vitsplit::split3_piece;
using vitsplit::split3_piece2;
using vitsplit::split3_piece8;
// four consecutive-k values of one row -> the three pieces of each, written to their planes of the split LDS row `row`
// (kc = k offset inside the K step, a multiple of 4: one ds_write_b64 per piece)
__device__ __forceinline__ void split3_store(float *row, int kc, f32x4 x) {
#pragma unroll
    for (int piece = 0; piece < 3; ++piece) *reinterpret_cast<u32x2 *>(row + piece * 8 + kc / 2) = split3_piece(x, piece);
}

// ---- pre-split weights (vithip_gemm_args.w_split) and the swizzled LDS rows of the walk that reads them --------------------------
// Image of W [N][K]: one block per (128-row panel, 16-deep K step), panel-major, K steps ascending inside a panel.  A block is
// 3 planes x 128 rows x 16 bf16; its 16-byte chunk c = plane * 256 + 2 * row + half holds k 8 half .. 8 half + 7 of one plane of
// one row.  Chunks 2 * row + half of 32 consecutive rows of one plane are 1 KB in the order of a matrix instruction's B operand
// (lane r + 32 h: row r, k 8 h .. 8 h + 7): the walk loads its W fragments from the image as they are (split3_step_pf).
constexpr int WIMG_ROWS = 128;
constexpr int WIMG_BLOCK_BYTES = 3 * WIMG_ROWS * SPLIT_BK * 2;  // 12 KB
// LDS row of the image walk (A only): 8 slots of 16 bytes, the six (plane, half) chunks s = 2 plane + half at slot
// s ^ split_swizzle(row).
// Conflict-free both ways (MI355X LDS banking: ds_write_b128 in 8-lane groups on (a/4) mod 32, ds_read_b128 in 16-lane groups on
// (a/4) mod 64):
//   writes: 8 consecutive threads = one aligned quad of rows x both halves; (row & 3) ^ ((row >> 2) & 3) takes 4 distinct values
//           over a quad, so the 8 chunks of one plane land in the 8 slots of a 32-bank line;
//   reads:  a fragment read = one (plane, half) of 16 rows distinct mod 16; (row & 1, slot) is distinct over them because the
//           swizzle is one-to-one on the 8 even and on the 8 odd rows of 16 (bit 3 of the row separates the two rows of each
//           parity that share bits 0..2 of it).
// (The on-the-fly split's rows of SPLIT_LD = 28 dwords read conflict-free but take their ds_write_b64 of neighbouring rows onto
// the same banks: 2.4 conflict cycles per LDS instruction in the r06 counters.)
constexpr int SPLIT_LD_SW = 32;  // floats
__device__ __forceinline__ int split_swizzle(int row) { return 2 * ((row & 3) ^ ((row >> 2) & 3)) + ((row >> 3) & 1); }
// float offset of chunk s of row `row` in a swizzled LDS tile
__device__ __forceinline__ int split_sw_offset(int row, int s) { return row * SPLIT_LD_SW + 4 * (s ^ split_swizzle(row)); }
// One 16-deep K step of a wave's TM x TN accumulators from the split LDS tiles As / Bs (at the lane's fragment: row r of the
// wave's first block, k offset 8h): the three pieces of every fragment, then 6 x TM x TN matrix instructions, term by term (the
// accumulators of one term are independent of each other).  restage(q), q < NS, is spread over the first half of them: the
// caller's staging slots (global -> registers -> LDS) of later steps.
template <int TM, int TN, int NS, typename Restage>
__device__ __forceinline__ void split3_step(f32x16 (&acc)[TM][TN], const float *As, const float *Bs, Restage &&restage) {
    bf16x8 a[TM][3], b[TN][3];
#pragma unroll
    for (int o = 0; o < 3; ++o) {  // the pieces in the order the first three terms need them: (hi, lo), (lo, hi), (mid, mid)
        const int pa = SPLIT_TERM_A[o], pb = SPLIT_TERM_W[o];
#pragma unroll
        for (int i = 0; i < TM; ++i) a[i][pa] = *reinterpret_cast<const bf16x8 *>(As + i * 32 * SPLIT_LD + pa * 8);
#pragma unroll
        for (int j = 0; j < TN; ++j) b[j][pb] = *reinterpret_cast<const bf16x8 *>(Bs + j * 32 * SPLIT_LD + pb * 8);
    }
    __builtin_amdgcn_sched_barrier(0);
    constexpr int NM = 6 * TM * TN, NR = NM / 2 > 0 ? NM / 2 : 1;
#pragma unroll
    for (int idx = 0; idx < NM; ++idx) {
        const int t = idx / (TM * TN), i = (idx / TN) % TM, j = idx % TN;
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][SPLIT_TERM_A[t]], b[j][SPLIT_TERM_W[t]], acc[i][j], 0, 0, 0);
        if (idx < NR) {
            const int slot_before = (idx * NS) / NR, slot_after = ((idx + 1) * NS) / NR;
            if (slot_after > slot_before) {
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int q = slot_before; q < slot_after; ++q) restage(q);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
}

// ---- the step of the image walk: W's fragments straight from the image, A's through LDS ---------------------------------------
// W.  A wave's fragment of one piece and one 32-row block is one contiguous 1 KB of the image, already in the matrix instruction's
// operand order: lane (r, h) takes chunk plane * 256 + 2 * (wn * 64 + j * 32 + r) + h of the K step's block.  So W never enters LDS:
// one 16-byte buffer load per lane, piece and block fetches the fragment where it is used, under the matrix instructions of the
// step before (SPLIT_W_LOADS).  The term order kills W-lo behind instruction 3 and W-mid behind 15 (2 x 2 accumulators): those are
// loaded in place behind their last use, 18 and 16 matrix instructions ahead of their first use in step g + 1; W-hi, live to the
// step's end, goes into a spare set that is moved over at the top of step g + 1.  hi and lo are requested in front of the step's
// two loads of A, which the next step's first restage slot waits for anyway (vmcnt retires in order: their wait is never the
// longer one); mid behind them, for the eighth matrix instruction of the next step.
// (A complete second register set for W, moved over at the step's top -- 12 v_mov_b64 instead of 4 -- gave back half of the gain:
// +1.2 % against +2.5 % images/s at the metric configuration, profiles/r30.)
// A.  Two LDS buffers of 128 swizzled rows (SPLIT_LD_SW) and one barrier per step.  Pipelined form (PFA, the fold consumers' and
// the plain walks): the barrier sits INSIDE the step, behind matrix instruction SPLIT_PF_BARRIER: all restage writes into the other
// buffer go in front of it, and behind it that buffer holds step g + 1 complete, so its six fragment reads are issued under the rest
// of this step's matrix instructions.  The term order kills A-lo behind instruction 7 and A-mid behind 19 (2 x 2 accumulators), so
// those are read in place; A-hi, live to the step's end, is read into a spare set and moved over at the step's end.  The residual
// walks (PFA = false) read A's fragments at the step's top, behind the barrier at the end of the step before.
// Segments.  A segment's first step reads A's fragments (split3_read_cold) and requests W's (the walk's cold load) at its top; its
// last step (PF = false) prefetches neither: no fragment is live across an epilogue, where the register count peaks.  As points at
// the lane's row r of the wave's first block, poff[piece] is the lane's float offset of its chunk (2 piece + h) inside that row
// (the same for every block: blocks are 32 rows apart and the swizzle repeats every 16).
struct Split3PfRead { int piece, behind; };  // A's piece, the matrix instruction its reads go behind
constexpr int SPLIT_PF_BARRIER = 15;
// hi first (the moves out of the spare set at the step's end wait for it), then in the order the next step's terms need the rest
constexpr Split3PfRead SPLIT_PF_READS[3] = {{0, 15}, {2, 17}, {1, 19}};
// W's loads of the next step: (piece, block j, the matrix instruction the load goes behind).  hi (into the spare set) in the first
// gaps, lo and mid behind their last use, in gaps that carry neither an LDS write nor a fragment read of A.
struct Split3WLoad { int piece, j, behind; };
constexpr Split3WLoad SPLIT_W_LOADS[6] = {{0, 0, 1}, {0, 1, 2}, {2, 0, 5}, {2, 1, 6}, {1, 0, 16}, {1, 1, 18}};
// Restage slots of the image walk's step (restage_fine of the walk): slot q goes behind matrix instruction at(q).  A's split in
// quarters of a plane (two values: 4 vector instructions for hi and mid, 1 for lo), so that no gap between two matrix instructions
// carries more than 4 of them plus one LDS write or one global load.
//   q 0-3 hi quarters, 4 hi write | 5-8 mid quarters, 9 mid write | 10, 11 lo halves, 12 lo write | 13, 14 the loads of A
struct Split3SlotsFine {
    static constexpr int N = 15, PASSES = 1;
    static constexpr int at(int q) {
        constexpr int gap[N] = {0, 1, 2, 3, 4, 4, 5, 6, 7, 8, 8, 9, 10, 12, 13};
        return gap[q];
    }
};
// The same 15 slots of the 64 x 256 walk's 32-deep step: two passes of the 24-instruction body, one per 16-deep sub-step, and ONE
// barrier, behind instruction SPLIT_PF_BARRIER of the second pass.  at(q) counts the matrix instructions of both passes (pass
// at(q) / 24, instruction at(q) % 24).  A thread's staging work per 32 of k is what the 128 x 128 walk does per 16, so one slot per
// gap is enough: no gap carries more than one quarter (4 vector instructions) or one LDS write or one load, and none of them shares
// its gap with a load of W (1, 2, 5, 6, 16, 18 of either pass) or a fragment read of A (15, 17, 19).  The two loads of A go out
// right behind the last quarter that consumes the registers they land in: 13 matrix instructions ahead of the step's end.
struct Split3SlotsFine2 {
    static constexpr int N = 15, PASSES = 2;
    static constexpr int at(int q) {
        constexpr int gap[N] = {0, 3, 7, 9, 11, 13, 20, 22, 24 + 0, 24 + 3, 24 + 4, 24 + 7, 24 + 8, 24 + 9, 24 + 10};
        return gap[q];
    }
};
// last matrix instruction (of 6 x per_term) that reads piece `piece` of operand w (0 = A, 1 = W)
constexpr int split3_last_use(int w, int piece, int per_term) {
    int last = -1;
    for (int t = 0; t < 6; ++t)
        if ((w ? SPLIT_TERM_W[t] : SPLIT_TERM_A[t]) == piece) last = (t + 1) * per_term - 1;
    return last;
}
// Slots: the restage table of a step of Slots::PASSES passes.  The tables of A's fragment reads and W's loads are per pass (every
// pass requests the W fragments of the pass behind it; a pass reads A's fragments of the next one in place).
template <typename Slots = Split3SlotsFine>
constexpr bool split3_pf_schedule_ok(int per_term, int blocks_w) {
    const int nm = 6 * per_term, barrier = (Slots::PASSES - 1) * nm + SPLIT_PF_BARRIER;  // the step's one barrier: in its last pass
    for (int q = 0; q < Slots::N; ++q) {
        // slots run in the order of q (a plane's quarters, its write; the loads of A behind the last quarter that reads what they
        // overwrite); every restage write of A (and, in the one-pass table, the loads too) in front of the barrier
        if (Slots::at(q) < 0 || Slots::at(q) >= Slots::PASSES * nm) return false;
        if (q > 0 && Slots::at(q) < Slots::at(q - 1)) return false;
        if ((q <= 12 || Slots::PASSES == 1) && Slots::at(q) > barrier) return false;
    }
    bool seen[3] = {};
    for (int e = 0; e < 3; ++e) {
        const Split3PfRead rd = SPLIT_PF_READS[e];
        if (rd.behind < SPLIT_PF_BARRIER || rd.behind >= 6 * per_term) return false;  // every read of the other buffer behind it
        // mid and lo are overwritten in place: behind their last use (hi goes to the spare set)
        if (rd.piece != 0 && rd.behind < split3_last_use(0, rd.piece, per_term)) return false;
        if (e > 0 && rd.behind < SPLIT_PF_READS[e - 1].behind) return false;
        seen[rd.piece] = true;
    }
    for (int pc = 0; pc < 3; ++pc)
        if (!seen[pc]) return false;
    // W: every (piece, block) requested once per pass; mid and lo are overwritten in place: behind their last use (hi goes to the
    // spare set)
    int asked = 0;
    for (int e = 0; e < 6; ++e) {
        const Split3WLoad ld = SPLIT_W_LOADS[e];
        if (ld.piece < 0 || ld.piece > 2 || ld.j < 0 || ld.j >= blocks_w) return false;
        if (ld.behind < 0 || ld.behind >= 6 * per_term) return false;
        if (ld.piece != 0 && ld.behind < split3_last_use(1, ld.piece, per_term)) return false;
        if (e > 0 && ld.behind < SPLIT_W_LOADS[e - 1].behind) return false;
        if (asked & (1 << (ld.piece * blocks_w + ld.j))) return false;
        asked |= 1 << (ld.piece * blocks_w + ld.j);
    }
    return asked == (1 << (3 * blocks_w)) - 1;
}
template <int TM, int TN>
struct Split3Frags {
    bf16x8 a[TM][3], b[TN][3];  // the step's pieces; mid and lo of the next step are read (A) and loaded (W) in place
    bf16x8 a_hn[TM], b_hn[TN];  // hi of the next step (hi of this one is live to the step's last matrix instruction)
};
// where a W load of the next step lands
template <int TM, int TN>
__device__ __forceinline__ bf16x8 &split3_w_dst(Split3Frags<TM, TN> &f, int piece, int j) {
    return piece != 0 ? f.b[j][piece] : f.b_hn[j];
}
// the reads of entry e of SPLIT_PF_READS from the tile As; NEXT: hi goes to the spare set
template <int TM, int TN, bool NEXT>
__device__ __forceinline__ void split3_read_piece(Split3Frags<TM, TN> &f, const float *As, const int (&poff)[3], int e) {
    const Split3PfRead rd = SPLIT_PF_READS[e];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const bf16x8 v = *reinterpret_cast<const bf16x8 *>(As + i * 32 * SPLIT_LD_SW + poff[rd.piece]);
        if (NEXT && rd.piece == 0) f.a_hn[i] = v;
        else f.a[i][rd.piece] = v;
    }
}
// A's fragments of a step from its own buffer, read at the step's top, in the order the prefetch reads them
template <int TM, int TN>
__device__ __forceinline__ void split3_read_cold(Split3Frags<TM, TN> &f, const float *As, const int (&poff)[3]) {
#pragma unroll
    for (int e = 0; e < 3; ++e) split3_read_piece<TM, TN, false>(f, As, poff, e);
}
struct Split3NoHook {
    __device__ __forceinline__ void operator()() const {}
};
// One step from the fragments in f, W's hi moving over from the spare set first (requested a step ago, or by the segment's cold
// load); restage(q), q < Slots::N, behind matrix instruction Slots::at(q) (pass PASS of the table's passes); sync() is the step's
// barrier (SYNC: this pass has it); PFW: the W fragments of the next pass by load_w(piece, j) into split3_w_dst; PFA: A's fragments
// of the next pass from An into f (the other buffer behind the barrier; without a barrier in this pass, the next sub-step of the
// SAME buffer, complete since the barrier of the step before); landed(): a hook in front of the first matrix instruction (the
// stamped probe instantiation; nothing otherwise).
template <int TM, int TN, bool PFA, bool PFW, typename Slots = Split3SlotsFine, int PASS = 0, bool SYNC = true, typename Restage,
          typename LoadW, typename Sync, typename Landed = Split3NoHook>
__device__ __forceinline__ void split3_step_pf(f32x16 (&acc)[TM][TN], Split3Frags<TM, TN> &f, const float *An, const int (&poff)[3],
                                               Restage &&restage, LoadW &&load_w, Sync &&sync, Landed &&landed = Landed{}) {
    constexpr int NM = 6 * TM * TN;
    static_assert(NM == 24, "the schedule table is laid out for 2 x 2 accumulators");
    static_assert(PASS >= 0 && PASS < Slots::PASSES && (SYNC || PASS + 1 < Slots::PASSES), "the barrier sits in the step's last pass");
    static_assert(split3_pf_schedule_ok<Slots>(TM * TN, TN),
                  "A: restage writes in front of the barrier, reads of the other buffer behind it and behind the last use of what they "
                  "overwrite; W: every fragment requested once per pass, mid and lo behind their last use");
#pragma unroll
    for (int j = 0; j < TN; ++j) f.b[j][0] = f.b_hn[j];
    landed();
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int idx = 0; idx < NM; ++idx) {
        const int t = idx / (TM * TN), i = (idx / TN) % TM, j = idx % TN;
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[i][SPLIT_TERM_A[t]], f.b[j][SPLIT_TERM_W[t]], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (PFW) {
#pragma unroll
            for (int e = 0; e < 6; ++e)
                if (SPLIT_W_LOADS[e].behind == idx) split3_w_dst(f, SPLIT_W_LOADS[e].piece, SPLIT_W_LOADS[e].j) = load_w(SPLIT_W_LOADS[e].piece, SPLIT_W_LOADS[e].j);
        }
#pragma unroll
        for (int q = 0; q < Slots::N; ++q)
            if (Slots::at(q) == PASS * NM + idx) restage(q);
        if (SYNC && idx == SPLIT_PF_BARRIER) sync();
        if constexpr (PFA) {
#pragma unroll
            for (int e = 0; e < 3; ++e)
                if (SPLIT_PF_READS[e].behind == idx) split3_read_piece<TM, TN, true>(f, An, poff, e);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (PFA) {
#pragma unroll
        for (int i = 0; i < TM; ++i) f.a[i][0] = f.a_hn[i];
    }
}

// ---- which tile the persistent walk takes (host; the ONE place: the launcher, the dispatcher's hand-over question and
// vithip_gemm_f32_walk_tile() all ask here) -------------------------------------------------------------------------------------
// The image walk (split arithmetic with a weight image) runs 64 x 256 tiles -- four waves side by side share one split of A -- where
// N is whole 256-column tiles and the epilogue's class keeps it by measurement; every other walk is 128 x 128.
// `epilogue`: the kernel's code (the fold forms and EPI_RESIDUAL_STATS included).  force: 1 = 128 x 128, 2 = 64 x 256 wherever it can
// run (the probe library's override), 0 = the standing choice.
struct WalkTile { int bm, bn; };
constexpr bool WALK_SHARED_A_FOLD = true, WALK_SHARED_A_RESIDUAL_STATS = true, WALK_SHARED_A_RESIDUAL = true, WALK_SHARED_A_PLAIN = true;
inline WalkTile walk_tile(int N, int epilogue, bool image, int force = 0) {
    const bool can = image && N > 0 && N % 256 == 0;
    const bool keeps = epi_is_fold(epilogue) ? WALK_SHARED_A_FOLD
                       : epilogue == EPI_RESIDUAL_STATS ? WALK_SHARED_A_RESIDUAL_STATS
                       : epilogue == VITHIP_EPI_BIAS_RESIDUAL ? WALK_SHARED_A_RESIDUAL : WALK_SHARED_A_PLAIN;
    return (can && force != 1 && (keeps || force == 2)) ? WalkTile{64, 256} : WalkTile{128, 128};
}

// ---- epilogue ---------------------------------------------------------------------------------
// Stores one workgroup tile.  A lane holds column n of 16 rows per accumulator; each store
// instruction writes two 128-B row segments.  vmcnt counts stores as well as loads, so any load that
// is waited for between stores serialises them on the full write latency (measured: 70k cycles per
// tile, 29 % of the kernel).  Hence: the bias is passed in registers (fetched long before), interior
// tiles take a branch-free path, and the residual / pos_emb operands of one accumulator are loaded
// in batches before their stores.
// LayerNorm fold, consumer side (EPI_BIAS_LN / EPI_BIAS_GELU_LN): what the epilogue needs besides the bias
template <int TN, int TM = 1>
struct FoldOperands {
    float colsum[TN];   // column sums of the folded weight at this lane's columns (fetched with the bias, long before)
    const f32x2 *rows;  // (rstd, mean) of the tile's rows m0, m0 + 1, ...: p.ln_rows + 2 m0, or the persistent walk's LDS copy of them
    // one tile per workgroup: the lane's own values, fetched with the bias when the kernel starts -- the bias's rule: no load
    // pending in the epilogue (17 per 32-row block otherwise); `preloaded` says so
    float rstd[TM][16], mean[TM];
    bool preloaded;
};
// the lane's (rstd of its 16 rows, mean of row r) per 32-row block, for FoldOperands::rstd / mean
template <int TN, int TM>
__device__ __forceinline__ void fold_preload(FoldOperands<TN, TM> &fold, const float *ln_rows, int M, int m_tile, int r, int h) {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int mr = m_tile + i * 32 + r;
        fold.mean[i] = ln_rows[2 * (size_t)(mr < M ? mr : M - 1) + 1];
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int m = m_tile + i * 32 + 4 * h + (v & 3) + 8 * (v >> 2);
            fold.rstd[i][v] = ln_rows[2 * (size_t)(m < M ? m : M - 1)];
        }
    }
    fold.preloaded = true;
}
// The fold's value, the same two fused multiply-adds in every kernel:
//     acc' = fma(-mean, colsum, acc)     x . (gamma W)^T - mean * colsum(gamma W) = (x - mean) . (gamma W)^T
//     y    = fma(rstd, acc', bias_f)
// The 32x32 kernels take the first one as ONE more v_mfma_f32_32x32x2_f32 per accumulator -- a rank-1 update with the k = 0
// operands (-mean of the lane's row, colsum of the lane's column) and zeros at k = 1: the instruction adds its two products to
// the accumulator one after the other, each with one rounding (tools/probes/mfma_order_probe.hip), so the result is
// fma(0, 0, fma(-mean, colsum, acc)) = the line above -- four matrix instructions per wave and tile instead of 64 vector ones.
__device__ __forceinline__ float fold_center(float acc, float mean, float colsum) { return __builtin_fmaf(-mean, colsum, acc); }
__device__ __forceinline__ float fold_scale(float centered, float rstd, float bias) { return __builtin_fmaf(rstd, centered, bias); }

template <int BM, int BN, int WM, int WN, int EPI, int AMODE>
__device__ __forceinline__ void epilogue_store(const GemmParams &p, const f32x16 (&acc)[WM / 32][WN / 32],
                                               const float (&bias_r)[WN / 32], int m0, int n0, int wm, int wn,
                                               int r, int h, const FoldOperands<WN / 32, WM / 32> &fold = FoldOperands<WN / 32, WM / 32>{}) {
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr bool FOLD = epi_is_fold(EPI);
    constexpr bool GELU = epi_is_gelu(EPI), QGELU = epi_is_qgelu(EPI);
    constexpr int ST_NT = 2;  // cache policy of the bias / GELU stores: non-temporal (qkv and the hidden layer are read by the NEXT launch)
    const bool interior = (m0 + BM <= p.M) && (n0 + BN <= p.N);  // workgroup-uniform
    if (interior) {
        if constexpr (FOLD) {
            // acc' = acc - mean * colsum as one rank-1 MFMA per accumulator: A operand = -mean of row r of the block (k = 0, lanes
            // h = 0; the h = 1 lanes supply k = 1: zero), B operand = colsum of column r.  One 32-row block at a time: its two
            // matrix instructions, the 16 rstd of the lane's rows (LDS reads in the persistent walk -- fetched once per block:
            // behind the scheduling fences of the GELU batches every batch would wait for its own), then the batches.
            const __amdgpu_buffer_rsrc_t c_rsrc = __builtin_amdgcn_make_buffer_rsrc(p.C, 0, 0x7fffffff, 0x00020000);
            // Centred weights (p.ln_colsum == NULL, vithip_ln_fold_weights_f32_centered): the accumulator IS the centred product and
            // the block goes straight to the scaling.  (With the colsum 0 the matrix instruction below would return the accumulator bit
            // for bit -- fma(-mean, 0, acc) -- so skipping it changes no result, in this kernel or against the ones that do not skip.)
            // What the skip is worth is not the four instructions (0.26 % of a K = 768 tile) but where they sit: in the epilogue of one
            // workgroup while the CU's other workgroup saturates the matrix pipe, each waits its turn and the FMAs wait for it -- stamps
            // put the fold's epilogue at 9.5k cycles per QKV tile against 5.1k for the plain one (round 5).
            const bool center = p.ln_colsum != nullptr;  // workgroup-uniform
            // Two code paths, chosen once per tile (a copy "centered = acc" on the path that does not centre cost 60 registers).
            // The path that does not centre reads the rstd of ALL the lane's rows first (LDS reads in the persistent walk) -- one exposed LDS round trip per tile
            // instead of one per 32-row block: they queue behind the fragment reads of the CU's other workgroup, and the scheduling
            // fences of the GELU batches keep the second block's reads from being issued before the first block's stores.
            auto rstd_of_block = [&](int i, float (&dst)[16]) __attribute__((always_inline)) {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int lr = wm * WM + i * 32 + 4 * h + 8 * g;  // tile-local row of registers 4g .. 4g + 3
#pragma unroll
                    for (int e = 0; e < 4; ++e) dst[4 * g + e] = fold.preloaded ? fold.rstd[i][4 * g + e] : fold.rows[lr + e].x;
                }
            };
            auto scale_and_store = [&](int i, const f32x16 (&src)[TN], const float (&row_rstd)[16]) __attribute__((always_inline)) {
                const int mb = m0 + wm * WM + i * 32 + 4 * h;  // row of register 0
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int n = n0 + wn * WN + j * 32 + r;
                    const int c_off = (mb * p.ldc + n) * 4, c_row = p.ldc * 4;
#pragma unroll
                    for (int half = 0; half < 2; ++half) {  // two batches of 8: values first (eight erf chains in lock-step), then 8 stores
                        float y[8];
#pragma unroll
                        for (int q = 0; q < 8; ++q) y[q] = fold_scale(src[j][half * 8 + q], row_rstd[half * 8 + q], bias_r[j]);
                        if constexpr (GELU) gelu_erf_x8(y);
                        if constexpr (QGELU) quick_gelu_x8(y);
#pragma unroll
                        for (int q = 0; q < 8; ++q) {
                            const int v = half * 8 + q;
                            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, y[q]), c_rsrc, c_off, ((v & 3) + 8 * (v >> 2)) * c_row, ST_NT);
                        }
                    }
                }
            };
            if (center) {
                float b_op[TN];
#pragma unroll
                for (int j = 0; j < TN; ++j) b_op[j] = h == 0 ? fold.colsum[j] : 0.0f;
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const float mean = fold.preloaded ? fold.mean[i] : fold.rows[wm * WM + i * 32 + r].y;
                    const float a_op = h == 0 ? -mean : 0.0f;
                    f32x16 centered[TN];
#pragma unroll
                    for (int j = 0; j < TN; ++j) centered[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a_op, b_op[j], acc[i][j], 0, 0, 0);
                    float row_rstd[16];
                    rstd_of_block(i, row_rstd);
                    scale_and_store(i, centered, row_rstd);
                }
            } else {
                float row_rstd[TM][16];
#pragma unroll
                for (int i = 0; i < TM; ++i) rstd_of_block(i, row_rstd[i]);
#pragma unroll
                for (int i = 0; i < TM; ++i) scale_and_store(i, acc[i], row_rstd[i]);
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + wn * WN + j * 32 + r;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int mb = m0 + wm * WM + i * 32 + 4 * h;  // row of register 0
                if constexpr (AMODE == A_PATCHES) {
                    float add[16];
                    size_t orow[16];
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        const int m = mb + (v & 3) + 8 * (v >> 2);
                        const int im = m / p.patches, pp = m - im * p.patches;
                        add[v] = p.pos[(size_t)(pp + 1) * p.N + n];
                        orow[v] = (size_t)(m + (im + 1) * p.prefix);
                    }
#pragma unroll
                    for (int v = 0; v < 16; ++v) p.C[orow[v] * p.ldc + n] = acc[i][j][v] + bias_r[j] + add[v];
                } else {
                    // Buffer addressing: SGPR descriptor + ONE per-lane byte offset per accumulator + the row's offset as the
                    // instruction's scalar operand.  With 64-bit pointers every one of the 16 rows cost vector address
                    // arithmetic (matrix-pipe time on gfx950) and a register pair; the persistent residual kernel spilled.
                    // The launcher keeps C and the residual below 2 GiB.
                    const __amdgpu_buffer_rsrc_t c_rsrc = __builtin_amdgcn_make_buffer_rsrc(p.C, 0, 0x7fffffff, 0x00020000);
                    const int c_off = (mb * p.ldc + n) * 4, c_row = p.ldc * 4;
                    if constexpr (EPI == VITHIP_EPI_BIAS_RESIDUAL) {
                        const __amdgpu_buffer_rsrc_t r_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.R), 0, 0x7fffffff, 0x00020000);
                        const int r_off = (mb * p.ldr + n) * 4, r_row = p.ldr * 4;
                        // two batches of 8 loads-then-stores: enough in flight, half the registers
#pragma unroll
                        for (int half = 0; half < 2; ++half) {
                            float res[8];
#pragma unroll
                            for (int q = 0; q < 8; ++q) {
                                const int v = half * 8 + q;
                                res[q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r_rsrc, r_off, ((v & 3) + 8 * (v >> 2)) * r_row, 0));
                            }
#pragma unroll
                            for (int q = 0; q < 8; ++q) {
                                const int v = half * 8 + q;
                                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, acc[i][j][v] + bias_r[j] + res[q]), c_rsrc, c_off,
                                                                      ((v & 3) + 8 * (v >> 2)) * c_row, 0);
                            }
                        }
                    } else {
                        // two batches of 8: values first (eight erf chains in lock-step), then 8 stores
#pragma unroll
                        for (int half = 0; half < 2; ++half) {
                            float y[8];
#pragma unroll
                            for (int q = 0; q < 8; ++q) y[q] = acc[i][j][half * 8 + q] + bias_r[j];
                            if constexpr (GELU) gelu_erf_x8(y);
                        if constexpr (QGELU) quick_gelu_x8(y);
#pragma unroll
                            for (int q = 0; q < 8; ++q) {
                                const int v = half * 8 + q;
                                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, y[q]), c_rsrc, c_off, ((v & 3) + 8 * (v >> 2)) * c_row, ST_NT);
                            }
                        }
                    }
                }
            }
        }
    } else {
        // edge tiles (last partial M tile, N not a multiple of the tile): per-element guards
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + wn * WN + j * 32 + r;
            const bool n_ok = n < p.N;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int m = m0 + wm * WM + i * 32 + (v & 3) + 8 * (v >> 2) + 4 * h;
                    if (n_ok && m < p.M) {
                        float y;
                        if constexpr (FOLD) {
                            const f32x2 row = fold.rows[m - m0];
                            y = fold_scale(fold_center(acc[i][j][v], row.y, fold.colsum[j]), row.x, bias_r[j]);
                        }
                        else y = acc[i][j][v] + bias_r[j];
                        if constexpr (AMODE == A_PATCHES) {
                            const int im = m / p.patches, pp = m - im * p.patches;
                            y += p.pos[(size_t)(pp + 1) * p.N + n];
                            p.C[(size_t)(m + (im + 1) * p.prefix) * p.ldc + n] = y;
                        } else {
                            if constexpr (GELU) y = gelu_erf(y);
                            if constexpr (QGELU) y = quick_gelu(y);
                            if constexpr (EPI == VITHIP_EPI_BIAS_RESIDUAL) y += p.R[(size_t)m * p.ldr + n];
                            p.C[(size_t)m * p.ldc + n] = y;
                        }
                    }
                }
            }
        }
    }
}

// ---- bf16 GEMM (vit_gemm_bf16.hip: launcher + two-stage kernel; vit_gemm_bf16_pp.hip: ping-pong kernel)
struct Bf16Params {
    const unsigned short *A;
    const unsigned short *W;
    const float *bias;
    const float *R;
    void *C;
    int lda, ldw, ldr, ldc;
    int M, N, K;
    int tiles_m, tiles_n, group_m;
    unsigned long long *dbg;  // stamped probe build only
    int patches;              // F32_EMBED epilogue: patches per image
    int prefix;               // F32_EMBED epilogue: rows in front of an image's patch rows in C (1 + register tokens)
    // LayerNorm folded into the GEMMs either side of it (ping-pong kernel only; vithip_gemm_bf16_args has the contract):
    const float *ln_rows;     // consumer (BF16 / BF16_GELU): [M][2] = (rstd, mean * rstd) of every row of A
    const float *ln_colsum;   // consumer: [N] column sums of the gamma-folded weight
    unsigned short *x16;      // producer (F32_RESIDUAL): bf16 copy of C, row stride ldx16
    int ldx16;
    float *partials;          // producer: [4 * tiles_n][M][2] partial (sum, sum of squares) per row and 64-column strip
};
int launch_gemm_bf16_pp(hipStream_t stream, const Bf16Params &p, int epilogue, int cus);
int launch_gemm_bf16_w4(hipStream_t stream, const Bf16Params &p, int epilogue, int cus);  // probe build: tools/probes/vit_gemm_bf16_w4.hip
// vit_gemm_latency.hip: 32x32 workgroup tiles on v_mfma_f32_16x16x4_f32 (bit-identical to the 32x32x2 kernels); K % 128 == 0
int launch_gemm_f32_latency(hipStream_t stream, GemmParams &p, int epilogue);
// vit_patch_embed_bf16.hip: patch embedding on the bf16 pipe as one implicit GEMM over the NCHW fp32 images
int launch_patch_embed_bf16(hipStream_t s, const float *images, const unsigned short *conv_w16, const float *conv_b,
                            const float *cls, const float *pos, float *x, int n_images, int img_size, int patch_size,
                            int in_chans, int embed_dim);

// ---- residual epilogue that also leaves the row statistics' partial sums (LayerNorm fold, producer side) ---------------------
// 16 per-lane values -> lane r of each 32-lane half holds the total of value (r >> 1) & 15 over the half's lanes, added in the
// butterfly order 16, 8, 4, 2, 1 (own + partner at every level): the order of vithip_rowstats_f32, at 15 + 1 exchanges instead
// of 16 x 5.
__device__ __forceinline__ float reduce_scatter16(const float (&a)[16], int r) {
    float b[8], c[4], d[2], e;
    {
        const bool up = (r & 16) != 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) b[k] = (up ? a[k + 8] : a[k]) + __shfl_xor(up ? a[k] : a[k + 8], 16);
    }
    {
        const bool up = (r & 8) != 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) c[k] = (up ? b[k + 4] : b[k]) + __shfl_xor(up ? b[k] : b[k + 4], 8);
    }
    {
        const bool up = (r & 4) != 0;
#pragma unroll
        for (int k = 0; k < 2; ++k) d[k] = (up ? c[k + 2] : c[k]) + __shfl_xor(up ? c[k] : c[k + 2], 4);
    }
    {
        const bool up = (r & 2) != 0;
        e = (up ? d[1] : d[0]) + __shfl_xor(up ? d[0] : d[1], 2);
    }
    return e + __shfl_xor(e, 1);
}

// C = acc + bias + residual as epilogue_store<EPI_BIAS_RESIDUAL> stores it, and p.row_partials[strip][m] = (sum, sum of squares)
// of the stored values of row m over the wave's 64-column strip, in the documented order of vithip_rowstats_f32: column c + l and
// c + 32 + l first (the lane's two accumulator columns), then the butterfly.  WN = 64 (one strip per wave), N % BN == 0.
template <int BM, int BN, int WM, int WN>
__device__ __forceinline__ void epilogue_store_residual_stats(const GemmParams &p, const f32x16 (&acc)[WM / 32][WN / 32],
                                                              const float (&bias_r)[WN / 32], int m0, int n0, int wm, int wn,
                                                              int r, int h) {
    static_assert(WN == 64, "one 64-column strip per wave");
    constexpr int TM = WM / 32;
    const bool interior = m0 + BM <= p.M;  // workgroup-uniform
    const int strip = (n0 + wn * WN) >> 6;
    const __amdgpu_buffer_rsrc_t c_rsrc = __builtin_amdgcn_make_buffer_rsrc(p.C, 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t r_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.R), 0, 0x7fffffff, 0x00020000);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int mb = m0 + wm * WM + i * 32 + 4 * h;  // row of register 0
        float y[2][16];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + wn * WN + j * 32 + r;
            const int c_off = (mb * p.ldc + n) * 4, c_row = p.ldc * 4, r_off = (mb * p.ldr + n) * 4, r_row = p.ldr * 4;
            if (interior) {
#pragma unroll
                for (int half = 0; half < 2; ++half) {  // two batches of 8 loads-then-stores, as in epilogue_store
                    float res[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const int v = half * 8 + q;
                        res[q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r_rsrc, r_off, ((v & 3) + 8 * (v >> 2)) * r_row, 0));
                    }
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const int v = half * 8 + q;
                        y[j][v] = acc[i][j][v] + bias_r[j] + res[q];
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, y[j][v]), c_rsrc, c_off, ((v & 3) + 8 * (v >> 2)) * c_row, 0);
                    }
                }
            } else {
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int m = mb + (v & 3) + 8 * (v >> 2);
                    y[j][v] = 0.0f;
                    if (m < p.M) {
                        y[j][v] = acc[i][j][v] + bias_r[j] + p.R[(size_t)m * p.ldr + n];
                        p.C[(size_t)m * p.ldc + n] = y[j][v];
                    }
                }
            }
        }
        float u[16], w[16];
        {
#pragma clang fp contract(off)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                u[v] = y[0][v] + y[1][v];
                const float sq0 = y[0][v] * y[0][v];
                w[v] = __builtin_fmaf(y[1][v], y[1][v], sq0);
            }
        }
        const float us = reduce_scatter16(u, r), ws = reduce_scatter16(w, r);
        const int v = (r >> 1) & 15;
        const int m = mb + (v & 3) + 8 * (v >> 2);
        if (!(r & 1) && m < p.M) *reinterpret_cast<f32x2 *>(p.row_partials + ((size_t)strip * p.M + m) * 2) = f32x2{us, ws};
    }
}

}  // namespace vitgemm
