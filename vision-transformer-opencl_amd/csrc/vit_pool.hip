// csrc/vit_pool.hip -- embedding outputs: LayerNorm + mean over tokens in one pass, and the L2 normalisation of output rows.
//
//   out[i][:] = gamma * ( 1/(tokens - first_tok) * sum_{t = first_tok}^{tokens-1} (x[i][t][:] - mean_t) * inv_std_t ) + beta
//
// with the per-row statistics of layernorm_f32_kernel (csrc/vit_rowops.hip) to the bit: the same lanes add the same elements in
// the same order, mean = s / dim, var = ss / dim - mean * mean, inv_std = 1 / sqrtf((double)var + eps)
// (tests/test_gpu_pool_kernel.py::test_one_pooled_row_is_the_layernorm_row_bit_for_bit).  gamma and beta are
// applied ONCE, to the pooled (x - mean) * inv_std: the mean over tokens is linear, so this is the mean of the LayerNorm rows
// with two fewer operations per element in the streaming pass and nothing but x read there.  One choice for every shape.
//
// x is read once and the [images][tokens][dim] LayerNorm output never exists.  Two launches:
//
//   1. pool_partial: the token rows of an image are cut into segments of POOL_SEG = 16 consecutive rows; one workgroup of four
//      waves takes one segment of one image.  Wave w normalises rows seg*16 + w, + 4, + 8, + 12 (all four loaded before any is
//      used: 4 x dim/64 floats per lane in flight) and adds them in that order into registers; the four waves' sums meet in LDS
//      and wave 0 adds them as ((w0 + w1) + w2) + w3 and stores one partial row [dim] to the workspace.
//   2. pool_finish: one workgroup per image adds the image's partial rows in segment order, divides by the row count, applies
//      gamma / beta and stores the output row.
//
// The summation order over tokens is thereby a function of (tokens, first_tok, dim) alone: not of the image count, of the image's
// index, of the grid or of scheduling.  No atomics, no arrival order.  Rows past the end of a ragged last segment contribute
// nothing (their loads are clamped to the image's last row and the result is not added).
// The partial rows are 1/16 of x's bytes written and read again: the pass moves 1.125 x the bytes of x.
//
// l2_normalize_rows: row /= max(||row||_2, 1e-12) (torch.nn.functional.normalize), one workgroup per row, the sum of squares
// reduced in a fixed order -- the bits of a row do not depend on how many rows the launch has.
//
// pool_layernorm: the other order, for heads that pool first and normalise the pooled row (timm fc_norm):
//
//   m[i][:] = 1/(tokens - first_tok) * sum_{t = first_tok}^{tokens-1} x[i][t][:];   out[i] = LayerNorm(m[i])   (or m[i] itself)
//
// The same two launches and the same streaming kernel, pool_partial, with NORM = false: it adds raw rows.  pool_layernorm_finish
// (ONE wave per image, which holds the row as vit_row.hpp wants it) adds the partial rows in segment order, divides by the row
// count and normalises the row with the arithmetic of vithip_layernorm_f32 -- the pooled row passes through LDS, so the statistics
// are taken from the stored fp32 values exactly as a vithip_layernorm_f32 launch would take them from memory.
#include <hip/hip_runtime.h>

#include "vit_hip_kernels.h"
#include "vit_row.hpp"

namespace {

using vit_row::f32x4;
using vit_row::wave_sum;

constexpr int POOL_THREADS = 256;
constexpr int POOL_WAVES = POOL_THREADS / 64;
constexpr int POOL_ROWS_PER_WAVE = 4;
constexpr int POOL_SEG = POOL_WAVES * POOL_ROWS_PER_WAVE;  // token rows per workgroup

// grid.x = images * segs; partial [images][segs][dim].  NORM: a row contributes (v - mean) * inv_std of its own statistics, else v.
template <int NVEC, bool NORM>
__global__ __launch_bounds__(POOL_THREADS) void pool_partial_kernel(const float *__restrict__ x, size_t ldx, float *__restrict__ partial,
                                                                     int tokens, int first_tok, int dim, int segs, double eps) {
    __shared__ f32x4 red[POOL_WAVES - 1][NVEC * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int image = blockIdx.x / segs, seg = blockIdx.x - image * segs;
    const float *img = x + (size_t)image * tokens * ldx;
    const int t0 = first_tok + seg * POOL_SEG + wave;

    f32x4 v[POOL_ROWS_PER_WAVE][NVEC];
#pragma unroll
    for (int k = 0; k < POOL_ROWS_PER_WAVE; ++k) {
        const int t = t0 + k * POOL_WAVES;
        const float *src = img + (size_t)(t < tokens ? t : tokens - 1) * ldx;  // clamped: always a row of this image
#pragma unroll
        for (int i = 0; i < NVEC; ++i) {
            const int c = (i * 64 + lane) * 4;
            v[k][i] = c < dim ? *reinterpret_cast<const f32x4 *>(src + c) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
    }
    f32x4 acc[NVEC];
#pragma unroll
    for (int i = 0; i < NVEC; ++i) acc[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int k = 0; k < POOL_ROWS_PER_WAVE; ++k) {
        const bool live = t0 + k * POOL_WAVES < tokens;  // wave-uniform
        if constexpr (NORM) {
            // the expressions of vit_row::row_stats, on rows already in registers (clamped rows take part in the shuffles).  A copy on
            // purpose: a load-free function split out of row_stats changes which products layernorm_f32_kernel contracts
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
            if (live) {
#pragma unroll
                for (int i = 0; i < NVEC; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] += (v[k][i][j] - mean) * inv_std;
            }
        } else if (live) {
#pragma unroll
            for (int i = 0; i < NVEC; ++i) acc[i] += v[k][i];
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int i = 0; i < NVEC; ++i) red[wave - 1][i * 64 + lane] = acc[i];
    }
    __syncthreads();
    if (wave == 0) {
        float *dst = partial + ((size_t)image * segs + seg) * dim;
#pragma unroll
        for (int i = 0; i < NVEC; ++i) {
            const int c = (i * 64 + lane) * 4;
            if (c < dim) {
                f32x4 a = acc[i];
#pragma unroll
                for (int w = 0; w < POOL_WAVES - 1; ++w) a += red[w][i * 64 + lane];
                *reinterpret_cast<f32x4 *>(dst + c) = a;
            }
        }
    }
}

// one workgroup per image; thread q takes float4 q, q + 256
__global__ __launch_bounds__(POOL_THREADS) void layernorm_pool_finish_kernel(const float *__restrict__ partial, float *__restrict__ out,
                                                                              size_t ldo, const float *__restrict__ gamma,
                                                                              const float *__restrict__ beta, int dim, int segs,
                                                                              float count) {
    const float *src = partial + (size_t)blockIdx.x * segs * dim;
    float *dst = out + (size_t)blockIdx.x * ldo;
    for (int c = threadIdx.x * 4; c < dim; c += POOL_THREADS * 4) {
        f32x4 a = *reinterpret_cast<const f32x4 *>(src + c);
        for (int s = 1; s < segs; ++s) a += *reinterpret_cast<const f32x4 *>(src + (size_t)s * dim + c);
        const f32x4 g = *reinterpret_cast<const f32x4 *>(gamma + c);
        const f32x4 b = *reinterpret_cast<const f32x4 *>(beta + c);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = a[j] / count * g[j] + b[j];
        *reinterpret_cast<f32x4 *>(dst + c) = o;
    }
}

// one workgroup per row, in place
__global__ __launch_bounds__(POOL_THREADS) void l2_normalize_rows_kernel(float *__restrict__ x, size_t ldx, int dim) {
    __shared__ float red[POOL_WAVES];
    float *row = x + (size_t)blockIdx.x * ldx;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float ss = 0.0f;
    for (int c = threadIdx.x * 4; c < dim; c += POOL_THREADS * 4) {
        const f32x4 v = *reinterpret_cast<const f32x4 *>(row + c);
        ss += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
    }
    ss = wave_sum(ss);
    if (lane == 0) red[wave] = ss;
    __syncthreads();
    ss = red[0];
#pragma unroll
    for (int w = 1; w < POOL_WAVES; ++w) ss += red[w];
    const float norm = fmaxf(sqrtf(ss), 1e-12f);
    for (int c = threadIdx.x * 4; c < dim; c += POOL_THREADS * 4) {
        f32x4 v = *reinterpret_cast<const f32x4 *>(row + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = v[j] / norm;
        *reinterpret_cast<f32x4 *>(row + c) = v;
    }
}

// pool_layernorm, launch 2: one workgroup of ONE wave per image; lane q holds float4 q, q + 64, ... of the row (vit_row.hpp).
// gamma == NULL (then beta is too; workgroup-uniform): the pooled mean itself is the output.
template <int NVEC>
__global__ __launch_bounds__(64) void pool_layernorm_finish_kernel(const float *__restrict__ partial, float *__restrict__ out, size_t ldo,
                                                                   const float *__restrict__ gamma, const float *__restrict__ beta, int dim,
                                                                   int segs, float count, double eps) {
    __shared__ f32x4 pooled[NVEC * 64];
    const int lane = threadIdx.x;
    const float *src = partial + (size_t)blockIdx.x * segs * dim;
    float *dst = out + (size_t)blockIdx.x * ldo;
    // segments outermost: the lane's NVEC loads of a segment are independent, so the chain of dependent loads is segs long
    f32x4 a[NVEC];
#pragma unroll
    for (int i = 0; i < NVEC; ++i) {
        const int c = (i * 64 + lane) * 4;
        a[i] = c < dim ? *reinterpret_cast<const f32x4 *>(src + c) : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    for (int s = 1; s < segs; ++s) {
#pragma unroll
        for (int i = 0; i < NVEC; ++i) {
            const int c = (i * 64 + lane) * 4;
            if (c < dim) a[i] += *reinterpret_cast<const f32x4 *>(src + (size_t)s * dim + c);
        }
    }
#pragma unroll
    for (int i = 0; i < NVEC; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < dim) {
#pragma unroll
            for (int j = 0; j < 4; ++j) a[i][j] = a[i][j] / count;
            if (gamma) pooled[i * 64 + lane] = a[i];
            else *reinterpret_cast<f32x4 *>(dst + c) = a[i];
        }
    }
    if (!gamma) return;
    __syncthreads();
    f32x4 v[NVEC];
    float mean, inv_std;
    vit_row::row_stats<NVEC>(reinterpret_cast<const float *>(pooled), dim, lane, v, mean, inv_std, eps);
#pragma unroll
    for (int i = 0; i < NVEC; ++i) {
        const int c = (i * 64 + lane) * 4;
        if (c < dim) {
            const f32x4 g = *reinterpret_cast<const f32x4 *>(gamma + c);
            const f32x4 b = *reinterpret_cast<const f32x4 *>(beta + c);
            *reinterpret_cast<f32x4 *>(dst + c) = vit_row::row_affine(v[i], mean, inv_std, g, b);
        }
    }
}

int pool_segs(int tokens, int first_tok) { return (tokens - first_tok + POOL_SEG - 1) / POOL_SEG; }

// What both pooling launchers ask of their arguments; affine_optional: gamma == beta == NULL is allowed.
bool pool_args_ok(const float *x, size_t ldx, const float *out, size_t ldo, const float *gamma, const float *beta, bool affine_optional,
                  int images, int tokens, int first_tok, int dim, const float *workspace) {
    if (!x || !out || !workspace || images <= 0 || first_tok < 0 || tokens < 2 || tokens <= first_tok) return false;
    if (affine_optional ? (gamma == nullptr) != (beta == nullptr) : !gamma || !beta) return false;
    if (!vit_row::rows_ok(x, ldx, dim) || !vit_row::rows_ok(out, ldo, dim)) return false;
    if (!vit_row::aligned16(gamma) || !vit_row::aligned16(beta) || !vit_row::aligned16(workspace)) return false;
    return (size_t)images * pool_segs(tokens, first_tok) <= (size_t)0x7fffffff;  // grid.x of the partial launch
}

template <int NVEC, bool NORM>
int launch_partial(hipStream_t s, const float *x, size_t ldx, float *partial, int images, int tokens, int first_tok, int dim, int segs,
                   double eps) {
    hipLaunchKernelGGL((pool_partial_kernel<NVEC, NORM>), dim3((unsigned)images * (unsigned)segs), dim3(POOL_THREADS), 0, s, x, ldx,
                       partial, tokens, first_tok, dim, segs, eps);
    return static_cast<int>(hipGetLastError());
}

int l2_launch(hipStream_t s, float *x, size_t ldx, int rows, int dim) {
    hipLaunchKernelGGL(l2_normalize_rows_kernel, dim3(rows), dim3(POOL_THREADS), 0, s, x, ldx, dim);
    return static_cast<int>(hipGetLastError());
}

}  // namespace

extern "C" {

size_t vithip_layernorm_pool_f32_workspace_floats(int images, int tokens, int first_tok, int dim) {
    if (images <= 0 || dim <= 0 || first_tok < 0 || tokens <= first_tok) return 0;
    return (size_t)images * pool_segs(tokens, first_tok) * dim;
}

int vithip_l2_normalize_rows_f32(vithip_stream_t stream, float *x, size_t ldx, int rows, int dim) {
    // not vit_row::rows_ok: the workgroup strides over the row, so dim has no upper bound
    if (!x || rows <= 0 || dim <= 0 || dim % 4 || ldx % 4 || ldx < (size_t)dim || !vit_row::aligned16(x))
        return static_cast<int>(hipErrorInvalidValue);
    return l2_launch(static_cast<hipStream_t>(stream), x, ldx, rows, dim);
}

int vithip_layernorm_pool_f32_eps(vithip_stream_t stream, const float *x, size_t ldx, float *out, size_t ldo, const float *gamma,
                                  const float *beta, int images, int tokens, int first_tok, int dim, int l2_normalize, float *workspace,
                                  double eps) {
    if (!pool_args_ok(x, ldx, out, ldo, gamma, beta, false, images, tokens, first_tok, dim, workspace) ||
        (l2_normalize != 0 && l2_normalize != 1) || !(eps > 0.0) || !(eps < 1.0e300))
        return static_cast<int>(hipErrorInvalidValue);
    const int segs = pool_segs(tokens, first_tok);
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = vit_row::dispatch_nvec(dim, [&](auto nvec) {
        return launch_partial<decltype(nvec)::value, true>(s, x, ldx, workspace, images, tokens, first_tok, dim, segs, eps);
    });
    if (rc) return rc;
    hipLaunchKernelGGL(layernorm_pool_finish_kernel, dim3(images), dim3(POOL_THREADS), 0, s, workspace, out, ldo, gamma, beta, dim, segs,
                       (float)(tokens - first_tok));
    rc = static_cast<int>(hipGetLastError());
    if (rc || !l2_normalize) return rc;
    return l2_launch(s, out, ldo, images, dim);
}
int vithip_layernorm_pool_f32(vithip_stream_t stream, const float *x, size_t ldx, float *out, size_t ldo, const float *gamma,
                              const float *beta, int images, int tokens, int first_tok, int dim, int l2_normalize, float *workspace) {
    return vithip_layernorm_pool_f32_eps(stream, x, ldx, out, ldo, gamma, beta, images, tokens, first_tok, dim, l2_normalize, workspace,
                                         VITHIP_LN_EPS);
}

size_t vithip_pool_layernorm_f32_workspace_floats(int images, int tokens, int first_tok, int dim) {
    return vithip_layernorm_pool_f32_workspace_floats(images, tokens, first_tok, dim);  // the same partial rows
}

int vithip_pool_layernorm_f32_eps(vithip_stream_t stream, const float *x, size_t ldx, float *out, size_t ldo, const float *gamma,
                                  const float *beta, int images, int tokens, int first_tok, int dim, float *workspace, double eps) {
    if (!pool_args_ok(x, ldx, out, ldo, gamma, beta, true, images, tokens, first_tok, dim, workspace) || !(eps > 0.0) || !(eps < 1.0e300))
        return static_cast<int>(hipErrorInvalidValue);
    const int segs = pool_segs(tokens, first_tok);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return vit_row::dispatch_nvec(dim, [&](auto nvec) {
        constexpr int NVEC = decltype(nvec)::value;
        const int rc = launch_partial<NVEC, false>(s, x, ldx, workspace, images, tokens, first_tok, dim, segs, eps);
        if (rc) return rc;
        hipLaunchKernelGGL(pool_layernorm_finish_kernel<NVEC>, dim3(images), dim3(64), 0, s, workspace, out, ldo, gamma, beta, dim, segs,
                           (float)(tokens - first_tok), eps);
        return static_cast<int>(hipGetLastError());
    });
}
int vithip_pool_layernorm_f32(vithip_stream_t stream, const float *x, size_t ldx, float *out, size_t ldo, const float *gamma,
                              const float *beta, int images, int tokens, int first_tok, int dim, float *workspace) {
    return vithip_pool_layernorm_f32_eps(stream, x, ldx, out, ldo, gamma, beta, images, tokens, first_tok, dim, workspace, VITHIP_LN_EPS);
}

}  // extern "C"
