// csrc/vit_map_head.hip -- attention pooling with one constant query per head (SigLIP's head, timm global_pool='map'), folded.
//
// With y_t = LayerNorm(x_t) (gamma, beta, the statistics of csrc/vit_row.hpp), keys t = first_tok .. tokens-1, A [heads][dim] the
// folded queries a_h = s * Wk_h^T q_h and hd = dim / heads:
//
//     p[h][t] = softmax_t(y_t . a_h);   z_h = sum_t p[h][t] y_t  in R^dim;   out[i][h*hd .. (h+1)*hd) = Wv_h z_h + bv_h
//
// The K/V projection of every token never runs: the score of a token is ONE dot product per head against a constant, and V is applied
// to the pooled row.  x is read once, 16 bytes per lane; y is never stored to HBM.  Two more folds, exact in real arithmetic, keep
// gamma and beta out of the streaming pass: with n_t = (x_t - mean_t) * inv_std_t,
//     y_t . a_h = n_t . (gamma o a_h) + beta . a_h      the last term is the same for every t and leaves the softmax: dropped
//     z_h       = gamma o (sum_t p[h][t] n_t) + beta    because the weights sum to 1: applied once, by the finishing launch
//
// Three launches:
//   0. map_fold_queries: G = gamma o A, zero-padded to HP = 16 or 32 heads (the matrix instruction's N), written in the order the
//      segment launch's B operands are read (one float4 per lane and four instructions).  dim * HP floats at most: microseconds.
//   1. map_pool_partial, one workgroup of four waves per (image, segment of TS consecutive key rows).  The segment is walked in
//      sub-tiles of 16 rows with an online softmax, so TS costs no LDS and no registers: it only sets how often (m, l, z) go out.
//        rows     wave w loads rows w, w + 4, w + 8, w + 12 of the sub-tile, takes their statistics and writes n_t to the LDS tile
//                 [16][ld] (ld = dim rounded up to 32, + 4: the pad columns are zero, so K tails and ragged column blocks read zeros)
//        scores   S [16][HP] = tile . G^T on the matrix pipe: v_mfma_f32_16x16x4_f32 (heads <= 16) or v_mfma_f32_32x32x2_f32
//                 (rows 16..31 of its M repeat rows 0..15 and are not used).  K is split over the waves in groups of four
//                 instructions; the four partial tiles meet in LDS and are added ((w0 + w1) + w2) + w3.
//        softmax  one thread per head: m' = max(m, max_r S), alpha = exp(m - m'), P[r] = exp(S[r] - m'), l = l * alpha + sum_r P[r]
//                 in row order.  Every exponential sits behind a maximum subtraction.
//        z        Z [HP][dim] = alpha o Z + P^T . tile on the same instruction; the accumulators stay in registers for the whole
//                 segment, split over the waves by column blocks of HP (wave w: blocks w, w + 4, ..).
//      At the segment's end (m, l) per head and z [heads][dim] go to the workspace: heads rows per TS rows of x.
//   2. map_pool_finish, one workgroup per (head, block of 16 images): merges an image's segments in index order (maximum first, then
//      l and z scaled by exp(m_s - m) and added), divides by l, applies gamma / beta, and forms Z_h [16][dim] . Wv_h^T [dim][hd] + bv_h
//      on v_mfma_f32_16x16x4_f32: Wv is read once per 16 images.
//
// Every order of summation is a function of (tokens, first_tok, dim, heads) alone; no atomics; a row of a matrix product depends on
// its own operand row only.  So an image's output row has the same bits alone and at every place of every batch, and a non-finite
// row of x reaches its own image only (the rule of vit_pool.hip).
//
// Also here: vithip_gelu_tanh_rows_f32, the tanh approximation of GELU in place on a few rows (the head's MLP hidden rows).
#include <hip/hip_runtime.h>

#include "vit_device.hpp"
#include "vit_hip_kernels.h"
#include "vit_row.hpp"
#ifdef VIT_PROBES
#include "vit_probes.h"
#endif

namespace {

using vit_row::f32x4;
using vit_row::wave_sum;
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int MAP_THREADS = 256;
constexpr int MAP_WAVES = MAP_THREADS / 64;
constexpr int MAP_SUB = 16;   // rows of a sub-tile: the M of the scores, the K of the z product
constexpr int MAP_IMGS = 16;  // images of a finishing workgroup: the M of its product
constexpr int MAP_TS = 64;    // key rows per segment: the measured choice

// The matrix instruction for HP padded heads.  Lane l supplies A[l % HP][l / HP] and B[l / HP][l % HP] of a product with K = KPI =
// 64 / HP; element i of its accumulator is C[crow(l, i)][l % HP].
template <int HP> struct Mfma;
template <> struct Mfma<16> {
    using acc = f32x4;
    static __device__ __forceinline__ acc run(float a, float b, acc c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int crow(int lane, int i) { return 4 * (lane >> 4) + i; }
};
template <> struct Mfma<32> {
    using acc = f32x16;
    static __device__ __forceinline__ acc run(float a, float b, acc c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int crow(int lane, int i) { return 8 * (i >> 2) + 4 * (lane >> 5) + (i & 3); }
};

int map_hp(int heads) { return heads <= 16 ? 16 : 32; }
int map_ld(int dim) { return (dim + 31) / 32 * 32 + 4; }
// floats of the folded queries in fragment order: K rounded up to the 4 * KPI columns four instructions take
size_t map_gfrag_floats(int dim, int hp) {
    const int kb = 4 * (64 / hp);
    return (size_t)((dim + kb - 1) / kb) * 64 * 4;
}
size_t map_rec_floats(int dim, int heads, int hp) { return 2 * (size_t)hp + (size_t)heads * dim; }  // [m | l | z [heads][dim]]

#ifdef VIT_PROBES
int g_map_ts = 0;  // process-wide override of MAP_TS (0 = none): the sweep of tools/map_head_time.py
#endif
int map_ts(int tokens, int first_tok, int dim, int heads) {
    (void)tokens; (void)first_tok; (void)dim; (void)heads;  // one choice for every shape, as measured
#ifdef VIT_PROBES
    if (g_map_ts > 0) return g_map_ts;
#endif
    return MAP_TS;
}
int map_segs(int tokens, int first_tok, int ts) { return (tokens - first_tok + ts - 1) / ts; }

// Launch 0.  Four instructions j = 0..3 of group q contract columns kb*q .. kb*q + kb-1 (kb = 4 * KPI); lane l takes column
// kb*q + 4 * (l / hp) + j in instruction j -- a permutation of K that A and B share, so that both read four consecutive floats.
__global__ __launch_bounds__(MAP_THREADS) void map_fold_queries_kernel(const float *__restrict__ a, const float *__restrict__ gamma,
                                                                        float *__restrict__ gfrag, int dim, int heads, int hp, int groups) {
    const int idx = blockIdx.x * MAP_THREADS + threadIdx.x;
    if (idx >= groups * 64) return;
    const int q = idx >> 6, lane = idx & 63, head = lane % hp, k0 = 4 * (64 / hp) * q + 4 * (lane / hp);
    f32x4 g = {0.0f, 0.0f, 0.0f, 0.0f};
    if (head < heads && k0 < dim) {  // dim % 4 == 0: the four columns are inside together
        const f32x4 av = *reinterpret_cast<const f32x4 *>(a + (size_t)head * dim + k0);
        const f32x4 gv = *reinterpret_cast<const f32x4 *>(gamma + k0);
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = gv[j] * av[j];
    }
    *reinterpret_cast<f32x4 *>(gfrag + (size_t)idx * 4) = g;
}

// Launch 1.  grid.x = images * segs; dim <= 256 * NVEC.  Dynamic LDS: tile [16][ld] | sp [4][16][HP] | p [16][HP] | alpha, m, l [HP].
template <int HP, int NVEC>
__global__ __launch_bounds__(MAP_THREADS) void map_pool_partial_kernel(const float *__restrict__ x, size_t ldx, const float *__restrict__ gfrag,
                                                                        float *__restrict__ part, int tokens, int first_tok, int dim,
                                                                        int heads, int segs, int ts, int ld, double eps) {
    using M = Mfma<HP>;
    constexpr int KPI = 64 / HP, KB = 4 * KPI, NB = 64 * NVEC / HP, NE = HP * HP / 64, STEPS = MAP_SUB / KPI;
    constexpr int RB = NVEC <= 3 ? 4 : 2;  // rows a wave has in flight
    extern __shared__ __attribute__((aligned(16))) float map_lds[];
    float *tile = map_lds;
    float *sp = tile + MAP_SUB * ld;
    float *p = sp + MAP_WAVES * MAP_SUB * HP;
    float *alpha = p + MAP_SUB * HP;
    float *mrun = alpha + HP, *lrun = mrun + HP;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane % HP, grp = lane / HP;
    const int image = blockIdx.x / segs, seg = blockIdx.x - image * segs;
    const float *img = x + (size_t)image * tokens * ldx;
    const int t_lo = first_tok + seg * ts, t_hi = t_lo + ts < tokens ? t_lo + ts : tokens;
    const int cblocks = (dim + HP - 1) / HP, groups = (dim + KB - 1) / KB, pad = ld - dim;

    for (int i = tid; i < MAP_SUB * pad; i += MAP_THREADS) tile[(i / pad) * ld + dim + i % pad] = 0.0f;  // written once, read as zeros
    if (tid < HP) { mrun[tid] = -INFINITY; lrun[tid] = 0.0f; }
    typename M::acc z[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int i = 0; i < NE; ++i) z[b][i] = 0.0f;

    for (int t0 = t_lo; t0 < t_hi; t0 += MAP_SUB) {
        // rows: n_t = (x_t - mean_t) * inv_std_t into the tile; rows past the segment's end are zeros
#pragma unroll
        for (int r0 = 0; r0 < MAP_SUB / MAP_WAVES; r0 += RB) {
            f32x4 v[RB][NVEC];
#pragma unroll
            for (int k = 0; k < RB; ++k) {
                const int t = t0 + wave + MAP_WAVES * (r0 + k);
                const float *src = img + (size_t)(t < t_hi ? t : t_hi - 1) * ldx;  // clamped: always a key row of this segment
#pragma unroll
                for (int i = 0; i < NVEC; ++i) {
                    const int c = (i * 64 + lane) * 4;
                    v[k][i] = c < dim ? *reinterpret_cast<const f32x4 *>(src + c) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                }
            }
#pragma unroll
            for (int k = 0; k < RB; ++k) {
                const int r = wave + MAP_WAVES * (r0 + k);
                const bool live = t0 + r < t_hi;  // wave-uniform
                // the expressions of vit_row::row_stats, on rows already in registers (as csrc/vit_pool.hip takes them)
                float s = 0.0f, ss = 0.0f;
#pragma unroll
                for (int i = 0; i < NVEC; ++i) {
                    const int c = (i * 64 + lane) * 4;
                    if (c < dim) {
                        s += (v[k][i][0] + v[k][i][1]) + (v[k][i][2] + v[k][i][3]);
                        ss += (v[k][i][0] * v[k][i][0] + v[k][i][1] * v[k][i][1]) + (v[k][i][2] * v[k][i][2] + v[k][i][3] * v[k][i][3]);
                    }
                }
                s = wave_sum(s);
                ss = wave_sum(ss);
                const float mean = s / (float)dim;
                const float var = ss / (float)dim - mean * mean;
                const float inv_std = 1.0f / sqrtf((float)((double)var + eps));
#pragma unroll
                for (int i = 0; i < NVEC; ++i) {
                    const int c = (i * 64 + lane) * 4;
                    if (c < dim) {
                        f32x4 o = {0.0f, 0.0f, 0.0f, 0.0f};
                        if (live) {
#pragma unroll
                            for (int j = 0; j < 4; ++j) o[j] = (v[k][i][j] - mean) * inv_std;
                        }
                        *reinterpret_cast<f32x4 *>(tile + r * ld + c) = o;
                    }
                }
            }
        }
        __syncthreads();

        // scores: this wave's share of K
        typename M::acc s;
#pragma unroll
        for (int i = 0; i < NE; ++i) s[i] = 0.0f;
        for (int q = wave; q < groups; q += MAP_WAVES) {
            const f32x4 a = *reinterpret_cast<const f32x4 *>(tile + (col & (MAP_SUB - 1)) * ld + KB * q + 4 * grp);
            const f32x4 b = *reinterpret_cast<const f32x4 *>(gfrag + ((size_t)q * 64 + lane) * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) s = M::run(a[j], b[j], s);
        }
#pragma unroll
        for (int i = 0; i < NE; ++i) {
            const int r = M::crow(lane, i);
            if (r < MAP_SUB) sp[(wave * MAP_SUB + r) * HP + col] = s[i];
        }
        __syncthreads();

        // online softmax: thread h owns head h (padded heads see scores of zero and are never stored)
        if (tid < HP) {
            const int rows = t_hi - t0 < MAP_SUB ? t_hi - t0 : MAP_SUB;
            const float m_old = mrun[tid];
            float sc[MAP_SUB], mx = m_old;
#pragma unroll
            for (int r = 0; r < MAP_SUB; ++r) {
                sc[r] = ((sp[r * HP + tid] + sp[(MAP_SUB + r) * HP + tid]) + sp[(2 * MAP_SUB + r) * HP + tid]) + sp[(3 * MAP_SUB + r) * HP + tid];
                if (r < rows) mx = fmaxf(mx, sc[r]);
            }
            const float al = expf(m_old - mx);  // the first sub-tile: exp(-inf) = 0
            float l = lrun[tid] * al;
#pragma unroll
            for (int r = 0; r < MAP_SUB; ++r) {
                const float e = r < rows ? expf(sc[r] - mx) : 0.0f;
                p[r * HP + tid] = e;
                l += e;
            }
            alpha[tid] = al; mrun[tid] = mx; lrun[tid] = l;
        }
        __syncthreads();

        // z = alpha o z + P^T . tile, this wave's column blocks
        float pa[STEPS], al[NE];
#pragma unroll
        for (int st = 0; st < STEPS; ++st) pa[st] = p[(KPI * st + grp) * HP + col];
#pragma unroll
        for (int i = 0; i < NE; ++i) al[i] = alpha[M::crow(lane, i)];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const int cb = wave + MAP_WAVES * b;
            if (cb < cblocks) {
#pragma unroll
                for (int i = 0; i < NE; ++i) z[b][i] *= al[i];
#pragma unroll
                for (int st = 0; st < STEPS; ++st) z[b] = M::run(pa[st], tile[(KPI * st + grp) * ld + cb * HP + col], z[b]);
            }
        }
        __syncthreads();  // the tile, sp and p are free for the next sub-tile
    }

    float *rec = part + ((size_t)image * segs + seg) * (2 * (size_t)HP + (size_t)heads * dim);
    if (tid < heads) { rec[tid] = mrun[tid]; rec[HP + tid] = lrun[tid]; }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int c = (wave + MAP_WAVES * b) * HP + col;
#pragma unroll
        for (int i = 0; i < NE; ++i) {
            const int h = M::crow(lane, i);
            if (h < heads && c < dim) rec[2 * HP + (size_t)h * dim + c] = z[b][i];
        }
    }
}

// Launch 2.  grid = (heads, ceil(images / 16)).  Dynamic LDS: tile [16][ld], row r = image block * 16 + r's pooled y-space row of head h.
__global__ __launch_bounds__(MAP_THREADS) void map_pool_finish_kernel(const float *__restrict__ part, const float *__restrict__ gamma,
                                                                       const float *__restrict__ beta, const float *__restrict__ wv,
                                                                       const float *__restrict__ bv, float *__restrict__ out, size_t ldo,
                                                                       int images, int dim, int heads, int hp, int segs, int ld) {
    extern __shared__ __attribute__((aligned(16))) float map_lds[];
    float *tile = map_lds;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int h = blockIdx.x, i0 = blockIdx.y * MAP_IMGS, hd = dim / heads, pad = ld - dim;
    const size_t rec_floats = 2 * (size_t)hp + (size_t)heads * dim;

    for (int i = tid; i < MAP_IMGS * pad; i += MAP_THREADS) tile[(i / pad) * ld + dim + i % pad] = 0.0f;
    for (int r = wave; r < MAP_IMGS; r += MAP_WAVES) {  // wave-uniform
        const int image = i0 + r;
        if (image >= images) {
            for (int c = lane * 4; c < dim; c += 256) *reinterpret_cast<f32x4 *>(tile + r * ld + c) = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            continue;
        }
        const float *rec = part + (size_t)image * segs * rec_floats;
        float m = rec[h];
        for (int s = 1; s < segs; ++s) m = fmaxf(m, rec[s * rec_floats + h]);
        float l = 0.0f;
        for (int s = 0; s < segs; ++s) l += rec[s * rec_floats + hp + h] * expf(rec[s * rec_floats + h] - m);
        for (int c = lane * 4; c < dim; c += 256) {
            f32x4 a = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int s = 0; s < segs; ++s) {
                const float e = expf(rec[s * rec_floats + h] - m);
                const f32x4 zs = *reinterpret_cast<const f32x4 *>(rec + s * rec_floats + 2 * hp + (size_t)h * dim + c);
#pragma unroll
                for (int j = 0; j < 4; ++j) a[j] += zs[j] * e;
            }
            const f32x4 g = *reinterpret_cast<const f32x4 *>(gamma + c);
            const f32x4 b = *reinterpret_cast<const f32x4 *>(beta + c);
#pragma unroll
            for (int j = 0; j < 4; ++j) a[j] = a[j] / l * g[j] + b[j];
            *reinterpret_cast<f32x4 *>(tile + r * ld + c) = a;
        }
    }
    __syncthreads();

    // out[image][h * hd + j] = tile[image] . Wv[h * hd + j] + bv: 16 columns j per wave and pass, two accumulation chains
    const int col = lane & 15, grp = lane >> 4, groups = (dim + 15) / 16;
    for (int jb = wave; jb * 16 < hd; jb += MAP_WAVES) {
        const int j = jb * 16 + col;
        const float *wrow = wv + (size_t)(h * hd + (j < hd ? j : hd - 1)) * dim;
        f32x4 acc[2] = {{0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}};
#pragma unroll 4
        for (int q = 0; q < groups; ++q) {  // unrolled: four groups' loads of Wv in flight
            const int k0 = 16 * q + 4 * grp;
            const f32x4 a = *reinterpret_cast<const f32x4 *>(tile + col * ld + k0);
            const f32x4 b = j < hd && k0 < dim ? *reinterpret_cast<const f32x4 *>(wrow + k0) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[q & 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u], b[u], acc[q & 1], 0, 0, 0);
        }
        if (j < hd) {
            const float bias = bv[h * hd + j];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int image = i0 + 4 * grp + i;
                if (image < images) out[(size_t)image * ldo + h * hd + j] = (acc[0][i] + acc[1][i]) + bias;
            }
        }
    }
}

// x * sigmoid(2 * 0.7978845608 * (x + 0.044715 x^3)) = 0.5 x (1 + tanh(..)), the exponent through v_exp_f32 and v_rcp_f32 as the
// QuickGELU epilogue takes its own: t = u * fp32(-2 log2 e), e = 2^t, r = 1 / (1 + e), x * r.
__global__ __launch_bounds__(MAP_THREADS) void gelu_tanh_rows_kernel(float *__restrict__ x, size_t ldx, int cols) {
    float *row = x + (size_t)blockIdx.x * ldx;
    for (int c = threadIdx.x * 4; c < cols; c += MAP_THREADS * 4) {
        f32x4 v = *reinterpret_cast<f32x4 *>(row + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float y = v[j];
            const float u = 0.7978845608f * (y + 0.044715f * (y * y * y));
            const float e = __builtin_amdgcn_exp2f(u * -2.8853900817779268f);
            v[j] = y * __builtin_amdgcn_rcpf(1.0f + e);
        }
        *reinterpret_cast<f32x4 *>(row + c) = v;
    }
}

template <typename K>
int allow_lds(K kernel, vitdev::PerDeviceOnce &once) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return static_cast<int>(e);
    if (once.is_done(dev)) return 0;
    e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e == hipSuccess) once.set(dev);
    return static_cast<int>(e);
}

template <int HP, int NVEC>
int launch_partial(hipStream_t s, const float *x, size_t ldx, const float *gfrag, float *part, int images, int tokens, int first_tok, int dim,
                   int heads, int segs, int ts, double eps) {
    static vitdev::PerDeviceOnce once;  // the attribute belongs to this device's copy of the kernel
    const int ld = map_ld(dim);
    const size_t lds = ((size_t)MAP_SUB * ld + (MAP_WAVES + 1) * MAP_SUB * HP + 3 * HP) * sizeof(float);
    const int rc = allow_lds(map_pool_partial_kernel<HP, NVEC>, once);
    if (rc) return rc;
    hipLaunchKernelGGL((map_pool_partial_kernel<HP, NVEC>), dim3((unsigned)images * (unsigned)segs), dim3(MAP_THREADS), lds, s, x, ldx, gfrag,
                       part, tokens, first_tok, dim, heads, segs, ts, ld, eps);
    return static_cast<int>(hipGetLastError());
}

// f(std::integral_constant<int, NVEC>) for the register variant that holds a row of dim floats: 256, 768, 1280 or 2048 columns
template <typename F>
int dispatch_map_nvec(int dim, F &&f) {
    if (dim <= 256) return f(std::integral_constant<int, 1>{});
    if (dim <= 768) return f(std::integral_constant<int, 3>{});
    if (dim <= 1280) return f(std::integral_constant<int, 5>{});
    return f(std::integral_constant<int, 8>{});
}

}  // namespace

extern "C" {

size_t vithip_map_pool_f32_workspace_floats(int images, int tokens, int first_tok, int dim, int heads) {
    if (images <= 0 || dim <= 0 || dim % 4 || heads < 1 || heads > 32 || dim % heads || first_tok < 0 || tokens <= first_tok) return 0;
    const int hp = map_hp(heads), segs = map_segs(tokens, first_tok, map_ts(tokens, first_tok, dim, heads));
    return map_gfrag_floats(dim, hp) + (size_t)images * segs * map_rec_floats(dim, heads, hp);
}

int vithip_map_pool_f32(vithip_stream_t stream, const float *x, size_t ldx, const float *gamma, const float *beta, double eps, const float *a,
                        const float *wv, const float *bv, float *out, size_t ldo, int images, int tokens, int first_tok, int dim, int heads,
                        float *workspace) {
    if (!x || !gamma || !beta || !a || !wv || !bv || !out || !workspace || images <= 0 || first_tok < 0 || tokens <= first_tok ||
        heads < 1 || heads > 32 || dim <= 0 || dim % heads || !(eps > 0.0) || !(eps < 1.0e300))
        return static_cast<int>(hipErrorInvalidValue);
    if (!vit_row::rows_ok(x, ldx, dim) || !vit_row::rows_ok(out, ldo, dim) || !vit_row::aligned16(gamma) || !vit_row::aligned16(beta) ||
        !vit_row::aligned16(a) || !vit_row::aligned16(wv) || !vit_row::aligned16(bv) || !vit_row::aligned16(workspace))
        return static_cast<int>(hipErrorInvalidValue);
    const int hp = map_hp(heads), ts = map_ts(tokens, first_tok, dim, heads), segs = map_segs(tokens, first_tok, ts);
    if ((size_t)images * segs > (size_t)0x7fffffff || (images + MAP_IMGS - 1) / MAP_IMGS > 65535) return static_cast<int>(hipErrorInvalidValue);
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *gfrag = workspace, *part = workspace + map_gfrag_floats(dim, hp);
    const int groups = (int)(map_gfrag_floats(dim, hp) / 256);
    hipLaunchKernelGGL(map_fold_queries_kernel, dim3((groups * 64 + MAP_THREADS - 1) / MAP_THREADS), dim3(MAP_THREADS), 0, s, a, gamma, gfrag,
                       dim, heads, hp, groups);
    int rc = static_cast<int>(hipGetLastError());
    if (rc) return rc;
    rc = dispatch_map_nvec(dim, [&](auto nvec) {
        constexpr int NVEC = decltype(nvec)::value;
        return hp == 16 ? launch_partial<16, NVEC>(s, x, ldx, gfrag, part, images, tokens, first_tok, dim, heads, segs, ts, eps)
                        : launch_partial<32, NVEC>(s, x, ldx, gfrag, part, images, tokens, first_tok, dim, heads, segs, ts, eps);
    });
    if (rc) return rc;
    static vitdev::PerDeviceOnce once;
    rc = allow_lds(map_pool_finish_kernel, once);
    if (rc) return rc;
    const int ld = map_ld(dim);
    hipLaunchKernelGGL(map_pool_finish_kernel, dim3(heads, (images + MAP_IMGS - 1) / MAP_IMGS), dim3(MAP_THREADS),
                       (size_t)MAP_IMGS * ld * sizeof(float), s, part, gamma, beta, wv, bv, out, ldo, images, dim, heads, hp, segs, ld);
    return static_cast<int>(hipGetLastError());
}

int vithip_gelu_tanh_rows_f32(vithip_stream_t stream, float *x, size_t ldx, int rows, int cols) {
    if (!x || rows <= 0 || cols <= 0 || cols % 4 || ldx % 4 || ldx < (size_t)cols || !vit_row::aligned16(x))
        return static_cast<int>(hipErrorInvalidValue);
    hipLaunchKernelGGL(gelu_tanh_rows_kernel, dim3(rows), dim3(MAP_THREADS), 0, static_cast<hipStream_t>(stream), x, ldx, cols);
    return static_cast<int>(hipGetLastError());
}

#ifdef VIT_PROBES
int vithip_map_pool_set_ts(int ts) {
    if (ts < 0 || ts % MAP_SUB) return static_cast<int>(hipErrorInvalidValue);
    g_map_ts = ts;
    return 0;
}
#endif

}  // extern "C"
