// csrc/vit_cls_attention.hip -- the class token's attention over the tokens of its image: one query row of the softmax, stored.
//
//   s_t = (q . k_t) / sqrtf(hd)           q = Q[i*T + 0][hd*h..], k_t = K[i*T + t][hd*h..]          (ViT_seq.c:156-190, one query row)
//   p_t = expf(s_t - max_t s) / sum_t expf(s_t - max)      t = 0..T-1, the class key included
//
// One kernel, cls_attention_kernel<BF16, HD64>, and one launcher behind the four entries vithip_cls_attention_f32 / _bf16 (head_dim 64)
// and _f32_hd / _bf16_hd (head_dim 64, or a multiple of 8 from 72 to 128).  HD64 chooses between two schedules of the same three
// passes (struct Sched); what follows describes head_dim 64, the differences of the other one stand at Sched.
//
// Every other attention kernel here keeps P in registers or LDS and stores P.V; this one stores P and never reads V.  It is bound by
// reading K once, n * T * heads * 64 elements, so the layout follows the bytes: a head's slice of a K row is 256 B (fp32) or 128 B
// (bf16) = GROUP lanes x 16 bytes.  A group of GROUP = 16 (fp32) / 8 (bf16) adjacent lanes takes one key: each lane loads 16 bytes,
// multiplies them with its own 4 / 8 elements of q (registers, loaded once per head), and a butterfly over the group (xor 8, 4, 2, 1)
// leaves the score in all its lanes.  A workgroup of 256 threads takes 16 / 32 keys per step and one (image, head) at a time:
//
//   pass 1  scores of all keys, group per key; kept in LDS for the first CA_CACHE keys; per-thread maxima, reduced over the workgroup
//   pass 2  sum of expf(s - max): thread per key from LDS; keys past the cache are recomputed, group per key
//   pass 3  p = expf(s - max) / sum, stored by the same mapping as pass 2
//
// Keys past the cache (T > 4096) cost two more dot products, read from L2: the same code with a cache miss, not another kernel --
// score() is one function of (image, head, key) and gives the same bits wherever it is called.  No thresholds at 224 / 704 tokens:
// one query row needs no K/V residency.
//
// head_mean = 0: grid = images * heads, out[i][h][t].  head_mean = 1: grid = images, the workgroup walks the heads in order and the
// thread that owns out[i][t] (the mapping of pass 3 depends on t alone) adds p[h][t] to it, head after head, and divides by
// (float)heads behind the last: ((p0 + p1) + p2 ...) / heads of exactly the bits head_mean = 0 stores.  No atomics, nothing depends
// on arrival order, and an image's row does not depend on where the image sits in the batch.
//
// q_scaled (bf16 fold engines): the Q columns hold vithip_qscale(hd) * q, the exponent of 2 of the softmax: p = exp2f(q.k - max) / sum.
#include <hip/hip_runtime.h>

#include <math.h>

#include "vit_attention.hpp"
#include "vit_hip_kernels.h"
#include "vit_row.hpp"

namespace {

using vit_row::wave_max;
using vit_row::wave_sum;
using vitattn::f32x4;
using vitattn::u32x4;

constexpr int CA_THREADS = 256;
constexpr int CA_WAVES = CA_THREADS / 64;
constexpr int CA_CACHE = 4096;  // scores kept in LDS (16 KB); keys past it are recomputed

// 16 bytes of a row as fp32: 4 floats, or 8 bf16 widened (element 2j in the low half of word j)
template <bool BF16> struct Piece;
template <> struct Piece<false> {
    static constexpr int VEC = 4;
    typedef float elem;
    static __device__ __forceinline__ void load(const float *p, float (&v)[4]) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(p);
        v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
    }
};
template <> struct Piece<true> {
    static constexpr int VEC = 8;
    typedef unsigned short elem;
    static __device__ __forceinline__ void load(const unsigned short *p, float (&v)[8]) {
        const u32x4 a = *reinterpret_cast<const u32x4 *>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[2 * j] = __uint_as_float(a[j] << 16);
            v[2 * j + 1] = __uint_as_float(a[j] & 0xffff0000u);
        }
    }
};

// The two schedules.  HD64: a head's slice of a row is exactly one 16-byte piece per lane of the group.  Otherwise (72..128): a group
// of 16 lanes for both element types, a lane takes the pieces sub, sub + 16 of the slice (fp32: 18..32 pieces, two rounds; bf16:
// 9..16 pieces, one round); a piece past head_dim is not loaded and adds nothing.
template <bool BF16, bool HD64> struct Sched {
    static constexpr int VEC = Piece<BF16>::VEC;
    static constexpr int GROUP = HD64 ? 64 / VEC : 16;        // lanes per key
    static constexpr int ROUNDS = HD64 || BF16 ? 1 : 2;       // pieces per lane
    static constexpr int AHEAD = HD64 ? 4 : 2;                // keys a group loads ahead in pass 1
    static constexpr int KEYS = CA_THREADS / GROUP;           // keys per workgroup step
};

// max / sum over the workgroup, the waves' values combined in wave order; every thread gets the result
template <bool MAX>
__device__ __forceinline__ float block_reduce(float v, float *red) {
    v = MAX ? wave_max(v) : wave_sum(v);
    __syncthreads();  // red may still be read from the reduction before
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int w = 1; w < CA_WAVES; ++w) r = MAX ? fmaxf(r, red[w]) : r + red[w];
    return r;
}

// scale: 1 / sqrtf(head_dim), or 1 with q_scaled.  HD64: head_dim_arg is 64 and is not read.
template <bool BF16, bool HD64>
__global__ __launch_bounds__(CA_THREADS) void cls_attention_kernel(const typename Piece<BF16>::elem *__restrict__ qkv, size_t row_stride,
                                                                    float *__restrict__ out, size_t ld_out, int tokens, int heads,
                                                                    int head_dim_arg, int head_mean, int q_scaled, float scale) {
    typedef Piece<BF16> E;
    typedef Sched<BF16, HD64> S;
    constexpr int VEC = S::VEC, GROUP = S::GROUP, ROUNDS = S::ROUNDS, AHEAD = S::AHEAD, KEYS = S::KEYS;
    __shared__ float cache[CA_CACHE];
    __shared__ float red[CA_WAVES];

    const int head_dim = HD64 ? 64 : head_dim_arg;
    const int tid = threadIdx.x, sub = tid % GROUP, grp = tid / GROUP;
    const int image = head_mean ? blockIdx.x : blockIdx.x / heads;
    const int h_lo = head_mean ? 0 : blockIdx.x - image * heads, h_hi = head_mean ? heads : h_lo + 1;
    const size_t D = (size_t)heads * head_dim;
    const typename E::elem *rows = qkv + (size_t)image * tokens * row_stride;  // the image's token rows: [Q | K | V]
    const int cached = tokens < CA_CACHE ? tokens : CA_CACHE;
    bool mine[ROUNDS];  // this lane has a piece in round i
#pragma unroll
    for (int i = 0; i < ROUNDS; ++i) mine[i] = HD64 || (sub + GROUP * i) * VEC < head_dim;

    for (int h = h_lo; h < h_hi; ++h) {
        float q[ROUNDS][VEC];
#pragma unroll
        for (int i = 0; i < ROUNDS; ++i) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) q[i][j] = 0.0f;
            if (mine[i]) E::load(rows + (size_t)h * head_dim + (sub + GROUP * i) * VEC, q[i]);
        }
        const typename E::elem *kh = rows + D + (size_t)h * head_dim + sub * VEC;  // this lane's first 16 bytes of key 0

        auto load_key = [&](int t, float (&k)[ROUNDS][VEC]) {
#pragma unroll
            for (int i = 0; i < ROUNDS; ++i) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) k[i][j] = 0.0f;
                if (mine[i]) E::load(kh + (size_t)t * row_stride + GROUP * i * VEC, k[i]);
            }
        };
        // the score of a key whose pieces are in k, in every lane of the group: products in element order, pieces in order, then the
        // butterfly
        auto dot = [&](const float (&k)[ROUNDS][VEC]) -> float {
            float a = q[0][0] * k[0][0];
#pragma unroll
            for (int i = 0; i < ROUNDS; ++i)
#pragma unroll
                for (int j = (i == 0 ? 1 : 0); j < VEC; ++j) a = fmaf(q[i][j], k[i][j], a);
#pragma unroll
            for (int off = GROUP / 2; off > 0; off >>= 1) a += __shfl_xor(a, off);
            return a * scale;
        };
        auto score = [&](int t) -> float {
            float k[ROUNDS][VEC];
            load_key(t, k);
            return dot(k);
        };
        auto weight = [&](float s, float m) -> float { return q_scaled ? exp2f(s - m) : expf(s - m); };

        __syncthreads();  // the cache of the head before has been read
        float m = -INFINITY;
        for (int t0 = grp; t0 < tokens; t0 += AHEAD * KEYS) {  // AHEAD keys of the group in flight before the first is used
            float k[AHEAD][ROUNDS][VEC];
#pragma unroll
            for (int u = 0; u < AHEAD; ++u) {
                const int t = t0 + u * KEYS;
                load_key(t < tokens ? t : tokens - 1, k[u]);  // clamped: always a row of this image
            }
#pragma unroll
            for (int u = 0; u < AHEAD; ++u) {
                const int t = t0 + u * KEYS;
                const float s = dot(k[u]);
                if (t < tokens) {
                    if (sub == 0 && t < CA_CACHE) cache[t] = s;
                    m = fmaxf(m, s);
                }
            }
        }
        m = block_reduce<true>(m, red);  // its barriers also publish the cache

        float l = 0.0f;
        for (int t = tid; t < cached; t += CA_THREADS) l += weight(cache[t], m);
        for (int t = CA_CACHE + grp; t < tokens; t += KEYS) {  // past the cache: the group recomputes, its first lane counts
            const float w = weight(score(t), m);
            if (sub == 0) l += w;
        }
        l = block_reduce<false>(l, red);

        float *dst = out + (size_t)image * ld_out + (head_mean ? 0 : (size_t)h * tokens);
        const int first = h == 0, last = h == heads - 1;
        auto emit = [&](int t, float p) {  // the owner of dst[t] is the same thread for every head
            if (head_mean) {
                if (!first) p = dst[t] + p;
                if (last) p = p / (float)heads;
            }
            dst[t] = p;
        };
        for (int t = tid; t < cached; t += CA_THREADS) emit(t, weight(cache[t], m) / l);
        for (int t = CA_CACHE + grp; t < tokens; t += KEYS) {
            const float p = weight(score(t), m) / l;
            if (sub == 0) emit(t, p);
        }
    }
}

// The one launcher behind the four entries.
template <bool BF16>
int launch(vithip_stream_t stream, const typename Piece<BF16>::elem *qkv, size_t q_row_stride, float *out, size_t ld_out, int n_images,
           int tokens, int heads, int head_dim, int head_mean, int q_scaled) {
    if (!vitattn::hd_accepted(head_dim) || !qkv || !out || n_images <= 0 || tokens <= 0 || heads <= 0 ||
        (head_mean != 0 && head_mean != 1) || (q_scaled != 0 && q_scaled != 1))
        return static_cast<int>(hipErrorInvalidValue);
    const size_t width = 3 * (size_t)heads * head_dim, row = head_mean ? (size_t)tokens : (size_t)heads * tokens;
    if (q_row_stride < width || q_row_stride % Piece<BF16>::VEC || ld_out < row) return static_cast<int>(hipErrorInvalidValue);
    if (!vit_row::aligned16(qkv) || (reinterpret_cast<size_t>(out) & 3)) return static_cast<int>(hipErrorInvalidValue);
    const size_t blocks = (size_t)n_images * (head_mean ? 1 : (size_t)heads);
    if (blocks > (size_t)0x7fffffff) return static_cast<int>(hipErrorInvalidValue);
    const float scale = q_scaled ? 1.0f : 1.0f / sqrtf((float)head_dim);  // head_dim 64: 0.125f, exact
    const auto kernel = head_dim == 64 ? cls_attention_kernel<BF16, true> : cls_attention_kernel<BF16, false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(CA_THREADS), 0, static_cast<hipStream_t>(stream), qkv, q_row_stride, out,
                       ld_out, tokens, heads, head_dim, head_mean, q_scaled, scale);
    return static_cast<int>(hipGetLastError());
}

}  // namespace

extern "C" {

int vithip_cls_attention_f32(vithip_stream_t stream, const float *qkv, size_t q_row_stride, float *out, size_t ld_out, int n_images,
                             int tokens, int heads, int head_mean) {
    return launch<false>(stream, qkv, q_row_stride, out, ld_out, n_images, tokens, heads, 64, head_mean, 0);
}

int vithip_cls_attention_bf16(vithip_stream_t stream, const unsigned short *qkv, size_t q_row_stride, float *out, size_t ld_out,
                              int n_images, int tokens, int heads, int head_mean, int q_scaled) {
    return launch<true>(stream, qkv, q_row_stride, out, ld_out, n_images, tokens, heads, 64, head_mean, q_scaled);
}

int vithip_cls_attention_f32_hd(vithip_stream_t stream, const float *qkv, size_t q_row_stride, float *out, size_t ld_out, int n_images,
                                int tokens, int heads, int head_dim, int head_mean) {
    return launch<false>(stream, qkv, q_row_stride, out, ld_out, n_images, tokens, heads, head_dim, head_mean, 0);
}

int vithip_cls_attention_bf16_hd(vithip_stream_t stream, const unsigned short *qkv, size_t q_row_stride, float *out, size_t ld_out,
                                 int n_images, int tokens, int heads, int head_dim, int head_mean, int q_scaled) {
    return launch<true>(stream, qkv, q_row_stride, out, ld_out, n_images, tokens, heads, head_dim, head_mean, q_scaled);
}

}  // extern "C"
