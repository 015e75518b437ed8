// csrc/vit_split_weights.hip -- the pre-split weight image of the three-piece split (vithip_gemm_args.w_split).
//
// The persistent split walk stages W as three bf16 pieces per value.  The weights are constant across forwards, yet the walk
// re-split them in every workgroup that visited a column tile: half the split's vector instructions.  This kernel makes the
// pieces once, in the image layout of vit_gemm_common.hpp (one 12 KB block per 128-row panel and 16-deep K step), with the
// split's own code (split3_piece8): the same bits the on-the-fly split puts into LDS, +-Inf, NaN and subnormals included.
//
// One thread makes one 16-byte chunk of each plane: 8 consecutive k of one row, i.e. thread t of block b is the thread t of the
// walk's staging that copies the chunk.  Rows past N read as zeros.  Elementwise, memory-bound, once per weight upload.
#include "vit_gemm_common.hpp"

namespace {

using namespace vitgemm;

__global__ __launch_bounds__(256) void split3_weights_kernel(const float *__restrict__ W, int ldw, int N, int nk,
                                                             unsigned char *__restrict__ out) {
    const size_t blk = blockIdx.x;  // panel * nk + K step
    const int t = threadIdx.x, row = t >> 1, half = t & 1;
    const int panel = (int)(blk / nk), step = (int)(blk - (size_t)panel * nk);
    const int n = panel * WIMG_ROWS + row;
    f32x4 x0 = {0.f, 0.f, 0.f, 0.f}, x1 = {0.f, 0.f, 0.f, 0.f};
    if (n < N) {
        const float *src = W + (size_t)n * ldw + step * SPLIT_BK + 8 * half;
        x0 = *reinterpret_cast<const f32x4 *>(src);
        x1 = *reinterpret_cast<const f32x4 *>(src + 4);
    }
    unsigned char *dst = out + blk * WIMG_BLOCK_BYTES + (size_t)t * 16;
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) *reinterpret_cast<u32x4 *>(dst + pl * 256 * 16) = split3_piece8(x0, x1, pl);
}

}  // namespace

extern "C" {

size_t vithip_split3_weights_bytes(int N, int K) {
    if (N <= 0 || K <= 0 || K % KALIGN) return 0;
    return (size_t)((N + WIMG_ROWS - 1) / WIMG_ROWS) * WIMG_ROWS * (size_t)K * 6;
}

int vithip_split3_weights_f32(vithip_stream_t stream, const float *W, int ldw, int N, int K, void *out) {
    if (!W || !out || N <= 0 || K <= 0 || K % KALIGN || ldw < K || ldw % 4) return static_cast<int>(hipErrorInvalidValue);
    if ((reinterpret_cast<size_t>(W) & 15) || (reinterpret_cast<size_t>(out) & 15)) return static_cast<int>(hipErrorInvalidValue);
    // the walk addresses the image through 32-bit buffer offsets
    if (vithip_split3_weights_bytes(N, K) >= 0x7fffffffull) return static_cast<int>(hipErrorInvalidValue);
    const int panels = (N + WIMG_ROWS - 1) / WIMG_ROWS, nk = K / SPLIT_BK;
    hipLaunchKernelGGL(split3_weights_kernel, dim3((unsigned)((size_t)panels * nk)), dim3(256), 0, static_cast<hipStream_t>(stream), W, ldw,
                       N, nk, static_cast<unsigned char *>(out));
    return static_cast<int>(hipGetLastError());
}

}  // extern "C"
