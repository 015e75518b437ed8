// csrc/vit_rowops.hip -- row-wise kernels: LayerNorm and the final softmax + top-1.
//
// LayerNorm follows ViT_seq.c:103-121 (NOT kernel.cl:6-80, which drops the epsilon):
//   mean = sum/dim, var = sum_sq/dim - mean*mean, inv_std = 1/sqrtf((double)var + 1e-6),
//   y = (x - mean) * inv_std * gamma + beta.
// One 64-lane wave per row: the row is read once as float4 (dim <= 2048 stays in registers),
// the two sums are reduced with wave shuffles, no LDS and no barrier.  HBM-bound by design.
// The row's arithmetic is csrc/vit_row.hpp, which csrc/vit_tap.hip shares bit for bit.
//
// softmax_top1 follows ViT_seq.c:304-324 and the argmax of Main.c:62-70 (first maximum wins).
#include <hip/hip_runtime.h>

#include "vit_hip_kernels.h"
#include "vit_row.hpp"

namespace {

using vit_row::f32x4;

constexpr int LN_THREADS = vit_row::THREADS;
constexpr int SM_THREADS = vit_row::THREADS;

typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;

// OUT = float, or unsigned short (bf16 bits) for the bf16 variant of the forward: statistics and the
// affine map are fp32 either way, only the store rounds.
template <int NVEC, typename OUT>
// x and y carry no __restrict__: y may BE x (same base, ldy == ldx, OUT = float).  A wave reads its whole row into registers in
// row_stats before row_affine stores any of it, and rows do not overlap each other, so the in-place form is structurally safe.
__global__ __launch_bounds__(LN_THREADS) void layernorm_f32_kernel(const float *x, size_t ldx,
                                                                   OUT *y, size_t ldy,
                                                                   const float *__restrict__ gamma,
                                                                   const float *__restrict__ beta,
                                                                   int rows, int dim, double eps) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * LN_THREADS + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * LN_THREADS) >> 6;
    for (int row = wave; row < rows; row += nwaves) {
        const float *src = x + (size_t)row * ldx;
        f32x4 v[NVEC];
        float mean, inv_std;
        vit_row::row_stats<NVEC>(src, dim, lane, v, mean, inv_std, eps);
        OUT *dst = y + (size_t)row * ldy;
#pragma unroll
        for (int i = 0; i < NVEC; ++i) {
            const int c = (i * 64 + lane) * 4;
            if (c < dim) {
                const f32x4 g = *reinterpret_cast<const f32x4 *>(gamma + c);
                const f32x4 b = *reinterpret_cast<const f32x4 *>(beta + c);
                const f32x4 o = vit_row::row_affine(v[i], mean, inv_std, g, b);
                if constexpr (sizeof(OUT) == 4) {
                    *reinterpret_cast<f32x4 *>(dst + c) = o;
                } else {
                    bf16x4 ob;
#pragma unroll
                    for (int j = 0; j < 4; ++j) ob[j] = (__bf16)o[j];
                    *reinterpret_cast<bf16x4 *>(dst + c) = ob;
                }
            }
        }
    }
}

// One workgroup per row.
__global__ __launch_bounds__(SM_THREADS) void softmax_top1_f32_kernel(const float *__restrict__ logits, int ld_logits,
                                                                      float *__restrict__ probs, int ld_probs,
                                                                      int *__restrict__ top1_label,
                                                                      float *__restrict__ top1_prob, int classes) {
    __shared__ float red_f[2][SM_THREADS / 64];
    __shared__ int red_i[SM_THREADS / 64];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *src = logits + (size_t)row * ld_logits;
    float *dst = probs + (size_t)row * ld_probs;

    float mx, sum;
    vit_row::softmax_row_stats(src, classes, red_f, mx, sum, [&](int c, float e) { dst[c] = e; });

    // normalise (each thread re-reads only its own writes) and track the first maximum probability
    float best = -1.0f;
    int arg = 0x7fffffff;
    for (int c = tid; c < classes; c += SM_THREADS) {
        const float pr = dst[c] / sum;
        dst[c] = pr;
        if (pr > best) { best = pr; arg = c; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_xor(best, off);
        const int oa = __shfl_xor(arg, off);
        if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
    // red_f[0] held the maxima: every wave read them in front of the barrier behind which it got here
    if (lane == 0) { red_f[0][wave] = best; red_i[wave] = arg; }
    __syncthreads();
    if (tid == 0) {
        best = red_f[0][0]; arg = red_i[0];
        for (int w = 1; w < SM_THREADS / 64; ++w)
            if (red_f[0][w] > best || (red_f[0][w] == best && red_i[w] < arg)) { best = red_f[0][w]; arg = red_i[w]; }
        if (top1_label) top1_label[row] = arg;
        if (top1_prob) top1_prob[row] = best;
    }
}

template <typename OUT>
int layernorm_dispatch(vithip_stream_t stream, const float *x, size_t ldx, OUT *y, size_t ldy, const float *gamma,
                       const float *beta, int rows, int dim, double eps) {
    // y is held to the rule of x whatever OUT is: a bf16 destination too is 16-byte aligned with ldy % 4 == 0
    if (!x || !y || !gamma || !beta || rows <= 0 || !vit_row::rows_ok(x, ldx, dim) || !vit_row::rows_ok(y, ldy, dim) ||
        !vit_row::aligned16(gamma) || !vit_row::aligned16(beta) || !(eps > 0.0) || !(eps < 1.0e300))
        return static_cast<int>(hipErrorInvalidValue);
    // in place (y == x, ldy == ldx, fp32 out) or disjoint: anything in between would read rows another wave has written
    {
        const char *xb = reinterpret_cast<const char *>(x), *yb = reinterpret_cast<const char *>(y);
        const size_t xs = ((size_t)(rows - 1) * ldx + dim) * sizeof(float), ys = ((size_t)(rows - 1) * ldy + dim) * sizeof(OUT);
        const bool in_place = xb == yb && ldx == ldy && sizeof(OUT) == sizeof(float);
        if (!in_place && xb < yb + ys && yb < xb + xs) return static_cast<int>(hipErrorInvalidValue);
    }
    return vit_row::dispatch_nvec(dim, [&](auto nvec) {
        hipLaunchKernelGGL((layernorm_f32_kernel<decltype(nvec)::value, OUT>), dim3(vit_row::grid_for_rows(rows)), dim3(LN_THREADS), 0,
                           static_cast<hipStream_t>(stream), x, ldx, y, ldy, gamma, beta, rows, dim, eps);
        return static_cast<int>(hipGetLastError());
    });
}

}  // namespace

extern "C" {

int vithip_layernorm_f32_eps(vithip_stream_t stream, const float *x, size_t ldx, float *y, size_t ldy,
                             const float *gamma, const float *beta, int rows, int dim, double eps) {
    return layernorm_dispatch<float>(stream, x, ldx, y, ldy, gamma, beta, rows, dim, eps);
}
int vithip_layernorm_f32(vithip_stream_t stream, const float *x, size_t ldx, float *y, size_t ldy,
                         const float *gamma, const float *beta, int rows, int dim) {
    return vithip_layernorm_f32_eps(stream, x, ldx, y, ldy, gamma, beta, rows, dim, VITHIP_LN_EPS);
}

int vithip_layernorm_f32_bf16out_eps(vithip_stream_t stream, const float *x, size_t ldx, unsigned short *y, size_t ldy,
                                     const float *gamma, const float *beta, int rows, int dim, double eps) {
    return layernorm_dispatch<unsigned short>(stream, x, ldx, y, ldy, gamma, beta, rows, dim, eps);
}
int vithip_layernorm_f32_bf16out(vithip_stream_t stream, const float *x, size_t ldx, unsigned short *y, size_t ldy,
                                 const float *gamma, const float *beta, int rows, int dim) {
    return vithip_layernorm_f32_bf16out_eps(stream, x, ldx, y, ldy, gamma, beta, rows, dim, VITHIP_LN_EPS);
}

int vithip_softmax_top1_f32(vithip_stream_t stream, const float *logits, int ld_logits, float *probs,
                            int ld_probs, int *top1_label, float *top1_prob, int rows, int classes) {
    if (!logits || !probs || rows <= 0 || classes <= 0 || ld_logits < classes || ld_probs < classes)
        return static_cast<int>(hipErrorInvalidValue);
    hipLaunchKernelGGL(softmax_top1_f32_kernel, dim3(rows), dim3(SM_THREADS), 0, static_cast<hipStream_t>(stream),
                       logits, ld_logits, probs, ld_probs, top1_label, top1_prob, classes);
    return static_cast<int>(hipGetLastError());
}

}  // extern "C"
