// csrc/vit_row.hpp -- the row schedule: what every kernel that gives a 64-lane wave one fp32 row shares, device and host side.
//
// One wave holds the row: lane `lane` keeps float4 number i * 64 + lane of it in v[i] (dim <= 64 * 4 * NVEC; lanes past the end hold
// nothing).  Four waves make a workgroup of THREADS = 256, a row each; a launch has at most 256 x 16 workgroups and walks further
// rows with a grid stride.  NVEC is a template argument chosen from dim by dispatch_nvec.
//
// LayerNorm of a row (row_stats, row_affine; every kernel that must give the bits of vithip_layernorm_f32 calls these two): the
// two sums are added per lane in vector order, then across the wave by xor shuffles from 32 down to 1;
//   mean = sum / dim, var = sum_sq / dim - mean * mean, inv_std = 1 / sqrtf((float)((double)var + eps))       (ViT_seq.c:103-121)
// with eps a DOUBLE the caller passes (VITHIP_LN_EPS = the double 1e-6 of the reference; added in double before the cast)
// and an element becomes (x - mean) * inv_std * gamma + beta.  Whoever changes an expression here changes every caller alike.
//
// Softmax of a row by a whole workgroup (softmax_row_stats): the one order of operations behind vithip_softmax_top1_f32 and the
// PROB scores of vithip_softmax_topk_f32.
#ifndef VIT_ROW_HPP
#define VIT_ROW_HPP

#include <hip/hip_runtime.h>

#include <type_traits>

namespace vit_row {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int THREADS = 256;  // four waves, a row each
constexpr int MAX_VEC = 8;    // float4 per lane: dim <= 64*4*8 = 2048

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

// Reads the row at src into v and leaves its statistics; every lane of the wave must call it.
template <int NVEC>
__device__ __forceinline__ void row_stats(const float *__restrict__ src, int dim, int lane, f32x4 (&v)[NVEC], float &mean,
                                          float &inv_std, double eps) {
    float s = 0.0f, ss = 0.0f;
#pragma unroll
    for (int i = 0; i < NVEC; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < dim) {
            v[i] = *reinterpret_cast<const f32x4 *>(src + c);
            s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
            ss += (v[i][0] * v[i][0] + v[i][1] * v[i][1]) + (v[i][2] * v[i][2] + v[i][3] * v[i][3]);
        }
    }
    s = wave_sum(s);
    ss = wave_sum(ss);
    mean = s / (float)dim;
    const float var = ss / (float)dim - mean * mean;
    inv_std = 1.0f / sqrtf((float)((double)var + eps));
}

// Four normalised elements from four of the row's, with the gamma and beta of their columns.
__device__ __forceinline__ f32x4 row_affine(const f32x4 v, float mean, float inv_std, const f32x4 g, const f32x4 b) {
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (v[j] - mean) * inv_std * g[j] + b[j];
    return o;
}

// The maximum mx of a row of logits and the sum of e_c = expf(src[c] - mx), by a workgroup of THREADS whose every thread calls it and
// gets both; store_e(c, e_c) is called once per class by the thread that owns it (thread t: classes t, t + THREADS, ...).
//   mx   thread t folds its classes with fmaxf from -INFINITY, the wave's 64 values meet in wave_max, the four waves' are folded 0..3
//   sum  thread t adds its e_c in ascending c from 0.0f, wave_sum, the four waves are added 0..3 from 0.0f
// red is the caller's LDS; nothing of it is read behind the second barrier except by the returning threads themselves, so the caller
// may write red[0] again at once and red[1] behind its next barrier.
template <typename STORE>
__device__ __forceinline__ void softmax_row_stats(const float *__restrict__ src, int classes, float (&red)[2][THREADS / 64], float &mx,
                                                  float &sum, STORE store_e) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    mx = -INFINITY;
    for (int c = tid; c < classes; c += THREADS) mx = fmaxf(mx, src[c]);
    mx = wave_max(mx);
    if (lane == 0) red[0][wave] = mx;
    __syncthreads();
    mx = red[0][0];
#pragma unroll
    for (int w = 1; w < THREADS / 64; ++w) mx = fmaxf(mx, red[0][w]);

    sum = 0.0f;
    for (int c = tid; c < classes; c += THREADS) {
        const float e = expf(src[c] - mx);
        store_e(c, e);
        sum += e;
    }
    sum = wave_sum(sum);
    if (lane == 0) red[1][wave] = sum;
    __syncthreads();
    sum = 0.0f;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) sum += red[1][w];
}

// ---- host side: what a launcher of a wave-per-row kernel needs ----

inline bool aligned16(const void *p) { return (reinterpret_cast<size_t>(p) & 15) == 0; }

// A matrix of rows the schedule can take: 16-byte loads of whole float4, the row in at most MAX_VEC of them per lane.
inline bool rows_ok(const void *p, size_t ld, int dim) {
    return aligned16(p) && dim > 0 && dim % 4 == 0 && dim <= 64 * 4 * MAX_VEC && ld % 4 == 0 && ld >= (size_t)dim;
}

// Workgroups of THREADS for `rows` rows, a wave per row: grid-stride beyond 16 workgroups per CU.
inline int grid_for_rows(int rows) {
    const int blocks = (rows + THREADS / 64 - 1) / (THREADS / 64);
    return blocks > 256 * 16 ? 256 * 16 : blocks;
}

// f(std::integral_constant<int, NVEC>) for the NVEC that holds a row of dim floats.
template <typename F>
auto dispatch_nvec(int dim, F &&f) {
    switch ((dim + 255) / 256) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        case 4: return f(std::integral_constant<int, 4>{});
        default: return f(std::integral_constant<int, MAX_VEC>{});
    }
}

}  // namespace vit_row

#endif  // VIT_ROW_HPP
