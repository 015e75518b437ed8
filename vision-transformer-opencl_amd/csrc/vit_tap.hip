// csrc/vit_tap.hip -- rows of the residual stream as an output: the class row, every token, the patch tokens, or the patch tokens as
// a channel-major map [dim][patches], each optionally through a LayerNorm of exactly the bits of vithip_layernorm_f32
// (csrc/vit_row.hpp holds the row arithmetic of both).
//
// CLS / TOKENS / PATCHES keep rows as rows: the LayerNorm kernel's schedule (one 64-lane wave per row, the row in registers, 16-byte
// loads and stores) with a source row and a destination that are computed per (image, token) instead of from one leading dimension.
//
// MAP transposes.  Stored from the row schedule a wave would write 64 channels = 64 different output rows per instruction, the
// scattered shape; here a wave stores runs along the token axis instead.  A workgroup of 16 waves (8 above dim 1024) owns a tile of consecutive patch
// tokens of one image -- 32 of them up to dim 1024, 16 above (the tile is [tokens][dim + 4] floats of LDS, 131 KB at most):
//   pass 1  a wave per row, EXACTLY the body of the row kernel (statistics and affine map on the row in registers, 16-byte loads),
//           with the LDS tile as its destination.  x is read once.  The statistics must be computed in this shape: the compiler
//           decides per use which of the products of the sum of squares it fuses into an FMA, and a statistics-only pass over the
//           same shared function came out of it with other last bits than the LayerNorm kernel's (measured: 4 rows of 48).
//   pass 2  behind one barrier, a lane collects four consecutive tokens of one channel from the tile and stores them as 16 bytes; a
//           wave takes 16 channels x 4 quads per instruction, then the next 4 quads of the same channels: a channel's run is the
//           tile's tokens (128 bytes, 64 above dim 1024).
// The row length dim + 4 keeps the 16-byte LDS stores of pass 1 aligned and, for dim % 16 == 0, makes pass 2 conflict-free:
// element (4q + j, c) lies at (4q + j) * (dim + 4) + c = 16 q + c + const (mod 64), 64 different banks for 4 q x 16 c.
// Where the runs cannot be 16-byte aligned (patches % 4 != 0: channel d starts at element d * patches) the tile is stored with one
// token per lane, 4 bytes each: a wave writes one channel's run per instruction.
// MAP and PATCHES run the same row body: the map is the transpose of the rows bit for bit.
#include <hip/hip_runtime.h>

#include "vit_device.hpp"
#include "vit_hip_kernels.h"
#include "vit_row.hpp"

namespace {

using vit_row::f32x4;

constexpr int TAP_THREADS = vit_row::THREADS;
// 16 waves per workgroup; 8 where a lane holds 8 vectors of its row (dim > 1024): 16 waves leave a lane 128 registers, too few for those
constexpr int map_threads(int nvec) { return nvec > 4 ? 512 : 1024; }
constexpr int MAP_PAD = 4;
__host__ __device__ constexpr int map_tile_tokens(int dim) { return dim <= 1024 ? 32 : 16; }

// One row: source -> destination, normalised with the row's own statistics (NORM) or copied.  Every lane of the wave calls it.
template <int NVEC, bool NORM>
__device__ __forceinline__ void tap_row(const float *__restrict__ src, float *__restrict__ dst, const float *__restrict__ gamma,
                                        const float *__restrict__ beta, int dim, int lane, double eps) {
    f32x4 v[NVEC];
    if constexpr (NORM) {
        float mean, inv_std;
        vit_row::row_stats<NVEC>(src, dim, lane, v, mean, inv_std, eps);
#pragma unroll
        for (int i = 0; i < NVEC; ++i) {
            const int c = (i * 64 + lane) * 4;
            if (c < dim) {
                const f32x4 g = *reinterpret_cast<const f32x4 *>(gamma + c);
                const f32x4 b = *reinterpret_cast<const f32x4 *>(beta + c);
                *reinterpret_cast<f32x4 *>(dst + c) = vit_row::row_affine(v[i], mean, inv_std, g, b);
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < NVEC; ++i) {
            const int c = (i * 64 + lane) * 4;
            if (c < dim) *reinterpret_cast<f32x4 *>(dst + c) = *reinterpret_cast<const f32x4 *>(src + c);
        }
    }
}

// rows = images * rows_per_image output rows; output row r is token first_tok + r % rows_per_image of image r / rows_per_image.
template <int NVEC, bool NORM>
__global__ __launch_bounds__(TAP_THREADS) void tap_rows_kernel(const float *__restrict__ x, size_t ldx, float *__restrict__ out,
                                                               size_t out_image_stride, const float *__restrict__ gamma,
                                                               const float *__restrict__ beta, int rows, int rows_per_image,
                                                               int first_tok, int tokens, int dim, double eps) {
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * TAP_THREADS + threadIdx.x) >> 6;
    const int nwaves = (gridDim.x * TAP_THREADS) >> 6;
    // (image, r) of the wave's row, advanced by the grid's step without a division per row: a wave's rows follow each other with
    // nothing to overlap, so what stands in front of a row's loads is paid in full
    const int step_images = nwaves / rows_per_image, step_rows = nwaves - step_images * rows_per_image;
    int image = wave / rows_per_image, r = wave - image * rows_per_image;
    for (int row = wave; row < rows; row += nwaves, image += step_images, r += step_rows) {
        if (r >= rows_per_image) { r -= rows_per_image; ++image; }
        const float *src = x + ((size_t)image * tokens + first_tok + r) * ldx;
        float *dst = out + (size_t)image * out_image_stride + (size_t)r * dim;
        tap_row<NVEC, NORM>(src, dst, gamma, beta, dim, lane, eps);
    }
}

// grid (images, token tiles), dynamic LDS = map_tile_tokens(dim) * (dim + MAP_PAD) floats; VEC: patches % 4 == 0, runs stored as 16 bytes
template <int NVEC, bool NORM, bool VEC>
__global__ __launch_bounds__(map_threads(NVEC)) void tap_map_kernel(const float *__restrict__ x, size_t ldx, float *__restrict__ out,
                                                              size_t out_image_stride, const float *__restrict__ gamma,
                                                              const float *__restrict__ beta, int tokens, int prefix, int dim,
                                                              double eps) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    constexpr int NWAVES = map_threads(NVEC) / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tt = map_tile_tokens(dim), ld = dim + MAP_PAD;
    const int patches = tokens - prefix, t0 = blockIdx.y * tt;
    const int valid = patches - t0 < tt ? patches - t0 : tt;  // tokens of this tile
    const float *rows = x + ((size_t)blockIdx.x * tokens + prefix + t0) * ldx;
    float *dst = out + (size_t)blockIdx.x * out_image_stride + t0;

    for (int k = wave; k < valid; k += NWAVES) tap_row<NVEC, NORM>(rows + (size_t)k * ldx, tile + k * ld, gamma, beta, dim, lane, eps);
    __syncthreads();

    if constexpr (VEC) {
        // lane -> channel cb * 16 + lane % 16, tokens 4 * q .. + 3 with q = qg * 4 + lane / 16 (all four valid or none: valid % 4 == 0)
        const int cl = lane & 15, ql = lane >> 4, cbs = (dim + 15) >> 4, qgs = tt >> 4;
        for (int cb = wave; cb < cbs; cb += NWAVES) {
            const int c = cb * 16 + cl;
            for (int qg = 0; qg < qgs; ++qg) {
                const int k = (qg * 4 + ql) * 4;
                if (k < valid && c < dim) {
                    const float *t = tile + k * ld + c;
                    f32x4 o;
                    o[0] = t[0]; o[1] = t[ld]; o[2] = t[2 * ld]; o[3] = t[3 * ld];
                    *reinterpret_cast<f32x4 *>(dst + (size_t)c * patches + k) = o;
                }
            }
        }
    } else {
        // a wave per channel, lane = token
        for (int c = wave; c < dim; c += NWAVES)
            if (lane < valid) dst[(size_t)c * patches + lane] = tile[lane * ld + c];
    }
}

template <int NVEC, bool NORM>
int launch_tap(hipStream_t s, const float *x, size_t ldx, float *out, size_t out_image_stride, const float *gamma, const float *beta,
               int images, int tokens, int prefix, int dim, int layout, double eps) {
    if (layout == VITHIP_TAP_MAP) {
        const int patches = tokens - prefix, tt = map_tile_tokens(dim);
        const dim3 grid(images, (patches + tt - 1) / tt);
        const size_t lds = (size_t)tt * (dim + MAP_PAD) * sizeof(float);
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return static_cast<int>(e);
        if (patches % 4 == 0) {
            static vitdev::PerDeviceOnce attr_set;  // the attribute belongs to this device's copy of the kernel
            if (!attr_set.is_done(dev)) {
                e = hipFuncSetAttribute(reinterpret_cast<const void *>(tap_map_kernel<NVEC, NORM, true>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
                if (e != hipSuccess) return static_cast<int>(e);
                attr_set.set(dev);
            }
            hipLaunchKernelGGL((tap_map_kernel<NVEC, NORM, true>), grid, dim3(map_threads(NVEC)), lds, s, x, ldx, out, out_image_stride, gamma,
                               beta, tokens, prefix, dim, eps);
        } else {
            static vitdev::PerDeviceOnce attr_set;
            if (!attr_set.is_done(dev)) {
                e = hipFuncSetAttribute(reinterpret_cast<const void *>(tap_map_kernel<NVEC, NORM, false>),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
                if (e != hipSuccess) return static_cast<int>(e);
                attr_set.set(dev);
            }
            hipLaunchKernelGGL((tap_map_kernel<NVEC, NORM, false>), grid, dim3(map_threads(NVEC)), lds, s, x, ldx, out, out_image_stride, gamma,
                               beta, tokens, prefix, dim, eps);
        }
        return static_cast<int>(hipGetLastError());
    }
    const int first_tok = layout == VITHIP_TAP_PATCHES ? prefix : 0;
    const int per_image = layout == VITHIP_TAP_CLS ? 1 : tokens - first_tok;
    const int rows = images * per_image;
    hipLaunchKernelGGL((tap_rows_kernel<NVEC, NORM>), dim3(vit_row::grid_for_rows(rows)), dim3(TAP_THREADS), 0, s, x, ldx, out,
                       out_image_stride, gamma, beta, rows, per_image, first_tok, tokens, dim, eps);
    return static_cast<int>(hipGetLastError());
}

}  // namespace

// prefix: the rows in front of an image's patch rows (the class token, then a register model's register tokens)
extern "C" int vithip_tap_f32_prefix_eps(vithip_stream_t stream, const float *x, size_t ldx, float *out, size_t out_image_stride,
                                         const float *gamma, const float *beta, int images, int tokens, int prefix, int dim, int layout,
                                         double eps) {
    const int bad = static_cast<int>(hipErrorInvalidValue);
    const bool patch_rows = layout == VITHIP_TAP_PATCHES || layout == VITHIP_TAP_MAP;
    if (!x || !out || !gamma != !beta || images <= 0 || tokens <= 0 || dim <= 0 || !(eps > 0.0) || !(eps < 1.0e300)) return bad;
    if (layout != VITHIP_TAP_CLS && layout != VITHIP_TAP_TOKENS && layout != VITHIP_TAP_PATCHES && layout != VITHIP_TAP_MAP) return bad;
    if (prefix < 1 || prefix > tokens || (patch_rows && prefix == tokens)) return bad;
    if (!vit_row::rows_ok(x, ldx, dim)) return bad;
    if ((long long)images * tokens > 0x7fffffffLL) return bad;                                     // row numbers are ints
    if (layout == VITHIP_TAP_MAP && (tokens - prefix + 15) / 16 > 65535) return bad;      // MAP: token tiles in grid.y
    const size_t per_image = layout == VITHIP_TAP_CLS ? 1 : layout == VITHIP_TAP_TOKENS ? (size_t)tokens : (size_t)(tokens - prefix);
    // out is not a matrix of rows with one leading dimension: an image's rows are dense, its stride covers them
    if (!vit_row::aligned16(out) || out_image_stride % 4 || out_image_stride < per_image * (size_t)dim) return bad;
    if (!vit_row::aligned16(gamma) || !vit_row::aligned16(beta)) return bad;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return vit_row::dispatch_nvec(dim, [&](auto nvec) {
        constexpr int NVEC = decltype(nvec)::value;
        return gamma ? launch_tap<NVEC, true>(s, x, ldx, out, out_image_stride, gamma, beta, images, tokens, prefix, dim, layout, eps)
                     : launch_tap<NVEC, false>(s, x, ldx, out, out_image_stride, gamma, beta, images, tokens, prefix, dim, layout, eps);
    });
}
extern "C" int vithip_tap_f32_eps(vithip_stream_t stream, const float *x, size_t ldx, float *out, size_t out_image_stride, const float *gamma,
                                  const float *beta, int images, int tokens, int dim, int layout, double eps) {
    return vithip_tap_f32_prefix_eps(stream, x, ldx, out, out_image_stride, gamma, beta, images, tokens, 1, dim, layout, eps);
}
extern "C" int vithip_tap_f32(vithip_stream_t stream, const float *x, size_t ldx, float *out, size_t out_image_stride, const float *gamma,
                              const float *beta, int images, int tokens, int dim, int layout) {
    return vithip_tap_f32_eps(stream, x, ldx, out, out_image_stride, gamma, beta, images, tokens, dim, layout, VITHIP_LN_EPS);
}
