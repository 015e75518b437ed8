// csrc/vit_swiglu.hip -- the gate of a SwiGLU MLP: h[r][j] = silu(u[r][j]) * u[r][H + j]  (include/vit_hip_kernels.h, "SwiGLU").
//
// The fc1 GEMM in front writes u = [gate | value] with its plain bias epilogue and the fc2 GEMM behind reads h; neither knows about
// the gate.  This pass is HBM-bound: 12 bytes of traffic per hidden element in fp32 (6 in bf16) against ~25 VALU instructions.
//   * every lane moves 16 bytes per access: the gate group and the value group of one (row, column group) are two 16-byte loads,
//     h is one 16-byte store; consecutive lanes take consecutive groups of a row, so a wave reads two runs of 1 KiB;
//   * a grid-stride walk over (row, column group) with at most 2,048 workgroups of 256; a lane takes two positions per trip so that
//     four loads are in flight before the first exp, and the position advances by (row step, column step) -- no 64-bit division;
//   * the exp and divide chains of the 8 (fp32) or 16 (bf16) elements of a trip advance in lock-step (the fences keep hipcc from
//     running one chain after the other, as in gelu_erf_x8 of csrc/vit_gemm_common.hpp);
//   * h is stored non-temporally, the policy the GEMMs give to rows the NEXT launch reads.
// In place (h == u, ldh == ldu) is safe because a lane reads both of its groups before it stores and no other lane reads them.
#include <hip/hip_runtime.h>

#include "vit_hip_kernels.h"

namespace {

constexpr int SG_THREADS = 256;
constexpr int SG_MAX_BLOCKS = 2048;
constexpr int SG_TRIP = 2;  // positions per lane and trip

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr float SG_TAIL = -87.0f;  // below it exp(-g) nears the end of the fp32 range: the tail form takes over

// N elements at once.  Per element, all fp32, one rounding per step (the header states it):
//   g >= -87 (and NaN):  e = expf(-g);  s = 1 + e;  q = g / s;  h = q * v
//   g <  -87:            t = expf(g / 2);  h = ((g * t) * v) * t       (1 + exp(g) rounds to 1 there)
// One expf per element either way: its argument is selected, and so is the result.
template <int N>
__device__ __forceinline__ void swiglu_xN(const float (&g)[N], const float (&v)[N], float (&h)[N]) {
    float e[N], main_h[N], tail_h[N];
#pragma unroll
    for (int i = 0; i < N; ++i) e[i] = g[i] < SG_TAIL ? 0.5f * g[i] : -g[i];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < N; ++i) e[i] = expf(e[i]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < N; ++i) main_h[i] = g[i] / (1.0f + e[i]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        main_h[i] = main_h[i] * v[i];
        tail_h[i] = ((g[i] * e[i]) * v[i]) * e[i];
        h[i] = g[i] < SG_TAIL ? tail_h[i] : main_h[i];
    }
}

template <typename T> struct sg_traits;
template <> struct sg_traits<float> { static constexpr int VEC = 4; };
template <> struct sg_traits<unsigned short> { static constexpr int VEC = 8; };

// 16 bytes -> VEC floats (bf16 -> fp32 is exact: the bits move to the upper half)
__device__ __forceinline__ void widen(const f32x4 &p, float (&o)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = p[i];
}
__device__ __forceinline__ void widen(const u32x4 &p, float (&o)[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        o[2 * i] = __builtin_bit_cast(float, p[i] << 16);
        o[2 * i + 1] = __builtin_bit_cast(float, p[i] & 0xffff0000u);
    }
}
__device__ __forceinline__ f32x4 narrow(const float (&x)[4]) { return f32x4{x[0], x[1], x[2], x[3]}; }
__device__ __forceinline__ u32x4 narrow(const float (&x)[8]) {
    u32x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const bf16x2 b = bf16x2{(__bf16)x[2 * i], (__bf16)x[2 * i + 1]};  // v_cvt_pk_bf16_f32: round to nearest even
        r[i] = __builtin_bit_cast(unsigned, b);
    }
    return r;
}

// groups = H / VEC column groups per row; a position is (row, group)
template <typename T>
__global__ __launch_bounds__(SG_THREADS) void swiglu_kernel(const T *u, size_t ldu, T *h, size_t ldh, unsigned rows, unsigned H,
                                                            unsigned groups) {
    constexpr int VEC = sg_traits<T>::VEC;
    using V = typename std::conditional<sizeof(T) == 4, f32x4, u32x4>::type;
    const unsigned tid = blockIdx.x * SG_THREADS + threadIdx.x, step = gridDim.x * SG_THREADS;
    const unsigned drow = step / groups, dgrp = step % groups;
    unsigned row = tid / groups, grp = tid % groups;
    while (row < rows) {
        unsigned r[SG_TRIP], c[SG_TRIP];
        bool live[SG_TRIP];
#pragma unroll
        for (int k = 0; k < SG_TRIP; ++k) {
            r[k] = row; c[k] = grp; live[k] = row < rows;
            if (live[k]) {  // a finished walk stays where it is: row never wraps
                row += drow; grp += dgrp;
                if (grp >= groups) { grp -= groups; ++row; }
            }
        }
        V gate[SG_TRIP], val[SG_TRIP];
#pragma unroll
        for (int k = 0; k < SG_TRIP; ++k) {
            gate[k] = V{}; val[k] = V{};
            if (live[k]) {
                const T *src = u + (size_t)r[k] * ldu + (size_t)c[k] * VEC;
                gate[k] = *reinterpret_cast<const V *>(src);
                val[k] = *reinterpret_cast<const V *>(src + H);
            }
        }
        float g[SG_TRIP * VEC], v[SG_TRIP * VEC], o[SG_TRIP * VEC];
#pragma unroll
        for (int k = 0; k < SG_TRIP; ++k) {
            float gk[VEC], vk[VEC];
            widen(gate[k], gk);
            widen(val[k], vk);
#pragma unroll
            for (int i = 0; i < VEC; ++i) { g[k * VEC + i] = gk[i]; v[k * VEC + i] = vk[i]; }
        }
        swiglu_xN<SG_TRIP * VEC>(g, v, o);
#pragma unroll
        for (int k = 0; k < SG_TRIP; ++k) {
            if (live[k]) {
                float ok[VEC];
#pragma unroll
                for (int i = 0; i < VEC; ++i) ok[i] = o[k * VEC + i];
                __builtin_nontemporal_store(narrow(ok), reinterpret_cast<V *>(h + (size_t)r[k] * ldh + (size_t)c[k] * VEC));
            }
        }
    }
}

template <typename T>
int swiglu_dispatch(vithip_stream_t stream, const T *u, size_t ldu, T *h, size_t ldh, int rows, int H) {
    constexpr int VEC = sg_traits<T>::VEC;
    if (!u || !h || rows < 1 || H < VEC || H % VEC) return static_cast<int>(hipErrorInvalidValue);
    if (ldu < 2 * (size_t)H || ldh < (size_t)H || ldu % VEC || ldh % VEC) return static_cast<int>(hipErrorInvalidValue);
    if ((reinterpret_cast<size_t>(u) & 15) || (reinterpret_cast<size_t>(h) & 15)) return static_cast<int>(hipErrorInvalidValue);
    // exactly in place, or disjoint address ranges (first element .. one past the last element touched)
    const bool in_place = u == h && ldu == ldh;
    if (!in_place) {
        const size_t u0 = reinterpret_cast<size_t>(u), u1 = u0 + ((size_t)(rows - 1) * ldu + 2 * (size_t)H) * sizeof(T);
        const size_t h0 = reinterpret_cast<size_t>(h), h1 = h0 + ((size_t)(rows - 1) * ldh + (size_t)H) * sizeof(T);
        if (u0 < h1 && h0 < u1) return static_cast<int>(hipErrorInvalidValue);
    }
    const unsigned groups = (unsigned)(H / VEC);
    const size_t positions = (size_t)rows * groups, per_block = (size_t)SG_THREADS * SG_TRIP;
    const size_t want = (positions + per_block - 1) / per_block;
    const int blocks = (int)(want < (size_t)SG_MAX_BLOCKS ? want : (size_t)SG_MAX_BLOCKS);
    hipLaunchKernelGGL((swiglu_kernel<T>), dim3(blocks), dim3(SG_THREADS), 0, static_cast<hipStream_t>(stream), u, ldu, h, ldh,
                       (unsigned)rows, (unsigned)H, groups);
    return static_cast<int>(hipGetLastError());
}

}  // namespace

extern "C" {

int vithip_swiglu_f32(vithip_stream_t stream, const float *u, size_t ldu, float *h, size_t ldh, int rows, int H) {
    return swiglu_dispatch<float>(stream, u, ldu, h, ldh, rows, H);
}

int vithip_swiglu_bf16(vithip_stream_t stream, const unsigned short *u, size_t ldu, unsigned short *h, size_t ldh, int rows, int H) {
    return swiglu_dispatch<unsigned short>(stream, u, ldu, h, ldh, rows, H);
}

}  // extern "C"
