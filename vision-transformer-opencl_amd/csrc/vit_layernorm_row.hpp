// csrc/vit_layernorm_row.hpp -- the arithmetic of one LayerNorm row, shared by every kernel that must give the bits of
// vithip_layernorm_f32 (csrc/vit_rowops.hip, csrc/vit_tap.hip).
//
// One 64-lane wave holds the row: lane `lane` keeps float4 number i * 64 + lane of it in v[i] (dim <= 64 * 4 * NVEC; lanes past the
// end hold nothing).  The two sums are added per lane in vector order, then across the wave by xor shuffles from 32 down to 1;
//   mean = sum / dim, var = sum_sq / dim - mean * mean, inv_std = 1 / sqrtf((float)((double)var + 1e-6))      (ViT_seq.c:103-121)
// and an element becomes (x - mean) * inv_std * gamma + beta.  Whoever changes an expression here changes every caller alike.
#ifndef VIT_LAYERNORM_ROW_HPP
#define VIT_LAYERNORM_ROW_HPP

#include <hip/hip_runtime.h>

namespace vit_ln {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int MAX_VEC = 8;  // float4 per lane: dim <= 64*4*8 = 2048

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// Reads the row at src into v and leaves its statistics; every lane of the wave must call it.
template <int NVEC>
__device__ __forceinline__ void row_stats(const float *__restrict__ src, int dim, int lane, f32x4 (&v)[NVEC], float &mean,
                                          float &inv_std) {
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
    inv_std = 1.0f / sqrtf((float)((double)var + 1e-6));
}

// Four normalised elements from four of the row's, with the gamma and beta of their columns.
__device__ __forceinline__ f32x4 row_affine(const f32x4 v, float mean, float inv_std, const f32x4 g, const f32x4 b) {
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = (v[j] - mean) * inv_std * g[j] + b[j];
    return o;
}

}  // namespace vit_ln

#endif  // VIT_LAYERNORM_ROW_HPP
