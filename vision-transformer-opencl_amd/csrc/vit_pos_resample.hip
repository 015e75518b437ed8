// csrc/vit_pos_resample.hip -- a ViT position embedding resampled to another patch grid, so that a checkpoint runs at an input size
// other than the one it was trained at.
//
//   src [1 + g_src^2][dim] -> dst [1 + g_dst^2][dim]: row 0 (the class token's embedding) is copied, rows 1.. are a g_src x g_src
//   raster of dim-vectors, resampled separably to g_dst x g_dst.
//
// Two modes, pinned to PyTorch (include/vit_hip_kernels.h states the arithmetic; tests/pos_resample_model.py restates it in numpy):
//   VITHIP_POS_BICUBIC     F.interpolate(mode="bicubic", align_corners=False)                    4 taps, A = -0.75, clamped indices
//   VITHIP_POS_BICUBIC_AA  the same with antialias=True (timm's resample_abs_pos_embed)          A = -0.5, support grows with in / out
//
// An axis is a table, built on the HOST in fp32 (vithip_pos_resample_table: callable without a device): per output index a first
// source index, a tap count and the weights; the source index of tap k is clamp(first + k, 0, in - 1).  The grids are square, so one
// table serves both axes.  The launcher uploads it (a few KB) and launches one kernel:
//   a workgroup per output row of dst -- block 0 copies the class row, block 1 + y * g_dst + x computes position (y, x);
//   the lanes spread across dim, four channels each, 16-byte loads and stores;
//   row_j = sum_i wx_i * src[iy_j][ix_i], then out = sum_j wy_j * row_j: accumulators start at 0.0f, taps in order, a product and a
//   sum are two roundings.
// Every element of dst is written exactly once, by plain vector stores.  No atomics, no LDS, nothing depends on the grid of the launch.
//
// Floating-point contraction: this file is compiled with -ffp-contract=off (FLAGS_vit_pos_resample in the package Makefile) and says
// so itself below, for the host table and the kernel alike.  A fused multiply-add anywhere here changes last bits, and the weights and
// the result are compared bit for bit with the numpy restatement.  No fast-math: the fp32 divisions are the correctly rounded ones.
//
// This runs once per weight load (ViT-B/16 at 384: 577 rows of 768 floats, at most 8 x 8 taps each) and is no hot path.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "vit_hip_kernels.h"

#pragma clang fp contract(off)

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int PR_THREADS = 256;
constexpr int PR_MAX_GRID = 256;   // patches per side, source and destination
constexpr int PR_MAX_DIM = 2048;

// ---- the axis table (host) ------------------------------------------------------------------------------------------------------

float cubic1(float x, float A) { return ((A + 2.0f) * x - (A + 3.0f)) * x * x + 1.0f; }
float cubic2(float x, float A) { return ((A * x - 5.0f * A) * x + 8.0f * A) * x - 4.0f * A; }

float aa_filter(float x) {
    const float A = -0.5f;
    x = fabsf(x);
    if (x < 1.0f) return ((A + 2.0f) * x - (A + 3.0f)) * x * x + 1.0f;
    if (x < 2.0f) return (((x - 5.0f) * x + 8.0f) * x - 4.0f) * A;
    return 0.0f;
}

// one output index; w has room for `cap` weights.  Returns the tap count, or -1 when it would not fit (never: the caller's cap is
// max(in, 4), and an antialiased index has xmax - xmin <= in taps).
int table_entry(int mode, int in, int out, int o, int *first, float *w, int cap) {
    const float scale = (float)in / (float)out;
    if (mode == VITHIP_POS_BICUBIC) {
        if (cap < 4) return -1;
        const float A = -0.75f;
        const float r = scale * ((float)o + 0.5f) - 0.5f;
        const float b = floorf(r);
        const float t = r - b;
        w[0] = cubic2(t + 1.0f, A);
        w[1] = cubic1(t, A);
        w[2] = cubic1(1.0f - t, A);
        w[3] = cubic2(2.0f - t, A);
        *first = (int)b - 1;
        return 4;
    }
    const float support = scale >= 1.0f ? 2.0f * scale : 2.0f;
    const float inv = scale >= 1.0f ? 1.0f / scale : 1.0f;
    const float center = scale * ((float)o + 0.5f);
    int xmin = (int)(center - support + 0.5f);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5f);
    if (xmax > in) xmax = in;
    const int cnt = xmax - xmin;
    if (cnt < 1 || cnt > cap) return -1;
    float tot = 0.0f;
    for (int j = 0; j < cnt; ++j) {
        w[j] = aa_filter(((float)(j + xmin) - center + 0.5f) * inv);
        tot = tot + w[j];
    }
    for (int j = 0; j < cnt; ++j) w[j] = w[j] / tot;
    *first = xmin;
    return cnt;
}

// ---- the kernel -----------------------------------------------------------------------------------------------------------------

// table: [first g_dst ints | count g_dst ints | weights g_dst x taps floats]
__global__ __launch_bounds__(PR_THREADS) void pos_resample_kernel(const float *__restrict__ src, int g_src, float *__restrict__ dst,
                                                                  int g_dst, int dim, const int *__restrict__ table, int taps) {
    const int quads = dim / 4;
    float *const out = dst + (size_t)blockIdx.x * dim;
    if (blockIdx.x == 0) {  // the class row: the bits of the source
        for (int q = threadIdx.x; q < quads; q += PR_THREADS)
            *reinterpret_cast<f32x4 *>(out + 4 * q) = *reinterpret_cast<const f32x4 *>(src + 4 * q);
        return;
    }
    const int p = (int)blockIdx.x - 1, y = p / g_dst, x = p % g_dst;
    const int *first = table, *count = table + g_dst;
    const float *weights = reinterpret_cast<const float *>(table + 2 * g_dst);
    const int fy = first[y], ny = count[y], fx = first[x], nx = count[x];
    const float *wy = weights + (size_t)y * taps, *wx = weights + (size_t)x * taps;
    const float *grid = src + dim;  // behind the class row
    for (int q = threadIdx.x; q < quads; q += PR_THREADS) {
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int j = 0; j < ny; ++j) {
            int iy = fy + j;
            iy = iy < 0 ? 0 : (iy > g_src - 1 ? g_src - 1 : iy);
            const float *line = grid + (size_t)iy * g_src * dim + 4 * q;
            f32x4 row = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int i = 0; i < nx; ++i) {
                int ix = fx + i;
                ix = ix < 0 ? 0 : (ix > g_src - 1 ? g_src - 1 : ix);
                const f32x4 v = *reinterpret_cast<const f32x4 *>(line + (size_t)ix * dim);
                const float w = wx[i];
#pragma unroll
                for (int c = 0; c < 4; ++c) row[c] = __fadd_rn(row[c], __fmul_rn(w, v[c]));
            }
            const float w = wy[j];
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = __fadd_rn(acc[c], __fmul_rn(w, row[c]));
        }
        *reinterpret_cast<f32x4 *>(out + 4 * q) = acc;
    }
}

bool mode_ok(int mode) { return mode == VITHIP_POS_BICUBIC || mode == VITHIP_POS_BICUBIC_AA; }
bool grid_ok(int g) { return g >= 1 && g <= PR_MAX_GRID; }

}  // namespace

extern "C" {

int vithip_pos_resample_table(int mode, int in, int out, int *first, int *count, float *weights, int max_taps) {
    if (!mode_ok(mode) || !grid_ok(in) || !grid_ok(out)) return -1;
    const int sizing = !first && !count && !weights;
    if (!sizing && (!first || !count || !weights || max_taps < 1)) return -1;
    const int bound = in > 4 ? in : 4;
    std::vector<float> w((size_t)bound);
    int widest = 0;
    for (int o = 0; o < out; ++o) {
        int f = 0;
        const int n = table_entry(mode, in, out, o, &f, w.data(), bound);
        if (n < 1 || (!sizing && n > max_taps)) return -1;
        if (n > widest) widest = n;
        if (sizing) continue;
        first[o] = f;
        count[o] = n;
        for (int k = 0; k < max_taps; ++k) weights[(size_t)o * max_taps + k] = k < n ? w[k] : 0.0f;
    }
    return widest;
}

int vithip_pos_resample_f32(vithip_stream_t stream, const float *src, int g_src, float *dst, int g_dst, int dim, int mode) {
    const int bad = static_cast<int>(hipErrorInvalidValue);
    if (!src || !dst || !mode_ok(mode) || !grid_ok(g_src) || !grid_ok(g_dst) || dim < 4 || dim > PR_MAX_DIM || dim % 4) return bad;
    if ((reinterpret_cast<size_t>(src) & 15) || (reinterpret_cast<size_t>(dst) & 15)) return bad;
    const int taps = vithip_pos_resample_table(mode, g_src, g_dst, nullptr, nullptr, nullptr, 0);
    if (taps < 1) return bad;
    std::vector<int> table((size_t)g_dst * (2 + taps));
    if (vithip_pos_resample_table(mode, g_src, g_dst, table.data(), table.data() + g_dst,
                                  reinterpret_cast<float *>(table.data() + 2 * g_dst), taps) != taps)
        return bad;
    hipStream_t s = static_cast<hipStream_t>(stream);
    int *d_table = nullptr;
    const size_t bytes = table.size() * sizeof(int);
    hipError_t rc = hipMalloc(reinterpret_cast<void **>(&d_table), bytes);
    if (rc != hipSuccess) return static_cast<int>(rc);
    rc = hipMemcpyAsync(d_table, table.data(), bytes, hipMemcpyHostToDevice, s);
    if (rc == hipSuccess) {
        hipLaunchKernelGGL(pos_resample_kernel, dim3(1 + g_dst * g_dst), dim3(PR_THREADS), 0, s, src, g_src, dst, g_dst, dim, d_table, taps);
        rc = hipGetLastError();
    }
    // the table lives for this call only: wait for the kernel that reads it (once per weight load, nothing to overlap with)
    const hipError_t rc_sync = hipStreamSynchronize(s);
    (void)hipFree(d_table);
    return static_cast<int>(rc != hipSuccess ? rc : rc_sync);
}

}  // extern "C"
