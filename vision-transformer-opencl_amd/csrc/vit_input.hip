// csrc/vit_input.hip -- the model input from 8-bit pixels: u8 HWC images -> normalised fp32 CHW.
//
//   dst[i][c][h][w] = ((float)src[i][h][w][c] / 255.0f - mean[c]) / std[c]
//
// torchvision's ToTensor() + Normalize(mean, std) (img.float().div(255), then sub_(mean).div_(std)), every step one fp32 IEEE
// operation: the divisions are true divisions (HIP device code divides correctly rounded unless fast-math is asked for; the gfx950
// code is v_div_scale / v_div_fmas / v_div_fixup), so the result is the bits a CPU computes from the same formula.
//
// One thread takes 4 consecutive pixels of a row (S % 4 == 0, so they never cross a row): one 4*C-byte load of the interleaved
// bytes, C 16-byte stores, one per channel plane.  Elementwise and memory-bound: 1 byte read, 4 written per element; the two
// divisions per element cost far less than the bytes.
#include <hip/hip_runtime.h>

#include <cmath>

#include "vit_hip_kernels.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int IN_THREADS = 256;
constexpr int IN_MAX_CHANS = 4;
constexpr int IN_MAX_Y = 65535;  // images per grid row; more loop

struct norm_consts {
    float mean[IN_MAX_CHANS], std[IN_MAX_CHANS];
};

// grid: x over the pixel quads of one image, y over the images
template <int C>
__global__ __launch_bounds__(IN_THREADS) void images_u8_hwc_to_f32_chw_kernel(const unsigned char *__restrict__ src,
                                                                              float *__restrict__ dst, int n, int quads,
                                                                              norm_consts k) {
    const int q = blockIdx.x * IN_THREADS + threadIdx.x;
    if (q >= quads) return;
    const size_t plane = (size_t)quads * 4;  // S * S
    for (int i = blockIdx.y; i < n; i += gridDim.y) {
        // 4 pixels x C bytes = C dwords, dword aligned (src is, and 4 * C * q is a multiple of 4)
        const unsigned int *p = reinterpret_cast<const unsigned int *>(src + ((size_t)i * plane + (size_t)q * 4) * C);
        unsigned int w[C];
#pragma unroll
        for (int d = 0; d < C; ++d) w[d] = p[d];
        float *o = dst + (size_t)i * C * plane + (size_t)q * 4;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            f32x4 v;
#pragma unroll
            for (int px = 0; px < 4; ++px) {
                const int b = px * C + c;  // byte of the quad: pixel px, channel c
                const float u = (float)((w[b >> 2] >> ((b & 3) * 8)) & 0xffu);
                v[px] = (u / 255.0f - k.mean[c]) / k.std[c];
            }
            *reinterpret_cast<f32x4 *>(o + (size_t)c * plane) = v;
        }
    }
}

template <int C>
int launch(hipStream_t s, const unsigned char *src, float *dst, int n, int quads, const norm_consts &k) {
    const dim3 grid((quads + IN_THREADS - 1) / IN_THREADS, n < IN_MAX_Y ? n : IN_MAX_Y);
    hipLaunchKernelGGL(images_u8_hwc_to_f32_chw_kernel<C>, grid, dim3(IN_THREADS), 0, s, src, dst, n, quads, k);
    return static_cast<int>(hipGetLastError());
}

}  // namespace

extern "C" {

int vithip_images_u8_to_f32(vithip_stream_t stream, const unsigned char *src, float *dst, int n, int img_size, int chans,
                            const float *mean, const float *std) {
    if (!src || !dst || !mean || !std || n < 1 || chans < 1 || chans > IN_MAX_CHANS || img_size < 4 || img_size % 4)
        return static_cast<int>(hipErrorInvalidValue);
    if ((reinterpret_cast<size_t>(src) & 3) || (reinterpret_cast<size_t>(dst) & 15)) return static_cast<int>(hipErrorInvalidValue);
    if ((size_t)img_size * img_size / 4 > (size_t)0x7fffffff - IN_THREADS) return static_cast<int>(hipErrorInvalidValue);
    norm_consts k = {};
    for (int c = 0; c < chans; ++c) {
        if (!std::isfinite(mean[c]) || !std::isfinite(std[c]) || std[c] == 0.0f) return static_cast<int>(hipErrorInvalidValue);
        k.mean[c] = mean[c];
        k.std[c] = std[c];
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int quads = (int)((size_t)img_size * img_size / 4);
    switch (chans) {
        case 1: return launch<1>(s, src, dst, n, quads, k);
        case 2: return launch<2>(s, src, dst, n, quads, k);
        case 3: return launch<3>(s, src, dst, n, quads, k);
        default: return launch<4>(s, src, dst, n, quads, k);
    }
}

}  // extern "C"
