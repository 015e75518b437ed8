// csrc/vit_depth.hip -- the tail of a linear depth head (DINOv2 BNHead for depth: classify, "linear" normalisation, bins): per-pixel
// depth from the token-major logits [P][bins] of a g x g patch grid (P = g * g) and an optional per-image bias z [bins] (the class
// token's columns of the 1x1 conv), without a bin value at the upsampled resolution anywhere in memory.
//
// vithip_dense_depth_f32: cell = logits + z; stage 1 on the U x U map (U = upsample * g): every bin map interpolated bilinearly
// (align_corners=False), r_b = relu(v_b) + 0.1, d = sum_b r_b * centre_b / sum_b r_b, clamped; stage 2: d interpolated bilinearly to
// out_h x out_w.  The arithmetic is stated in vit_hip_kernels.h; every product and sum below is one rounded fp32 operation (this file
// is compiled with -ffp-contract=off, host side included: the launcher checks the blocks with the kernel's own expressions).
//
// Stage 1, depth_expect_kernel<u>.  With an integer factor u the up-pixels of one axis fall into g + 1 BLOCKS of u consecutive
// pixels, block j = pixels u*j - (u+1)/2 .. + u - 1 (clipped to the map: the first and the last block are partial), whose pixels all
// read the same two source cells (i0, i1) = (j - 1, j), clamped at the edges: their source coordinates lie in [j - 1, j), and the
// block boundaries sit where rounding cannot move a pixel across them (even u: 1 / 2u away from an integer; odd u: the first pixel
// sits on the integer and fl(1 / u) >= 1 / u for u = 3, 5, 7, so its product never rounds below -- the launcher walks every pixel of
// the axis with the kernel's own expression and refuses a factor for which that does not hold).  One LANE owns one u x u block of
// the map: per bin it reads the block's 2 x 2 cells from LDS ONCE (4 reads for u * u pixels -- 16 at u = 4), forms the 2u horizontal
// sums with its u column weights, the u * u values with its u row weights, and keeps a running (s, t) = (sum r, sum r * centre) per
// pixel in registers: 2 * u * u accumulators (32 at u = 4).  The per-pixel weights are the stated l0 / l1 of that pixel, not phases
// assumed periodic, so the bits are the contract's for every u.  Sums run over the bins in ascending order, s and t side by side.
//
// The (g + 1)^2 blocks are cut into strips of nearly equal width, at most 256 block columns (one strip whenever g <= 255), and
// numbered row-major inside a strip; a workgroup of 256 lanes takes 256 consecutive numbers, so a 17 x 17 or 38 x 38 block grid fills
// its workgroups but for the last.  The cells those blocks read -- a few whole rows of the strip -- are staged through LDS cell-major
// with the bins of a cell contiguous at the odd stride BS + 1 floats, z added while staging (one rounding); consecutive lanes read
// the same bin of the same or of consecutive cells: equal addresses broadcast, consecutive cells fall on different banks.  The bins
// are walked in slices of BS = a power of two (the largest that fits DEPTH_LDS_FLOATS, at most 64; (s, t) carry over, two barriers
// per slice), and the bin centres lie in LDS beside the window, read as a broadcast.  A window stays below 1600 cells, so BS >= 4
// always: every g, every bins in 2..256 and every u in 1..8 runs.  At g = 16 / 37, 256 bins, u = 4 the window is 256 / 333 cells, BS
// = 32, 34 / 44 KB with the centres: four workgroups per CU at g = 16 (what 119 VGPRs allow), three at g = 37 (LDS).  The kernel is
// bound by VALU work: per bin and lane 4 + 1 LDS reads against 6u + 9u^2 fp32 operations (168 at u = 4; nothing is contracted, so a
// multiply-add is two), far above its HBM floor of logits read once per workgroup.
//
// Stage 2, depth_resize_kernel: one thread per output pixel, four reads of the U x U map (87 KB per image at 518: L2 resident) and
// one coalesced store.  Its floor is the output write itself (4 bytes per pixel), which a fusion into stage 1 would not remove; a
// fused tile with a halo would recompute the halo's 256-bin expectations instead.  When out_h = out_w = U the resize is the
// identity on every non-NaN value (weights exactly 1 and 0) and stage 1 stores straight into `out`; a NaN stays a NaN either way.
//
// No atomics; a pixel's depth depends on its image's logits alone, whatever the grid.  Non-finite logits travel through the
// arithmetic as IEEE says: (v < 0 ? 0 : v) keeps a NaN, the clamp's comparisons are false for one.
#include <hip/hip_runtime.h>

#include <cmath>

#include "vit_hip_kernels.h"

namespace {

constexpr int DEPTH_THREADS = 256;
constexpr int DEPTH_LDS_FLOATS = 12032;  // the window at most; with 256 centres 48 KB: never fewer than three workgroups per CU
constexpr int DEPTH_MAX_BINS = 256;
constexpr int DEPTH_MAX_SLICE = 64;
constexpr int DEPTH_MAX_OUT = 4096;

// One axis of F.interpolate(bilinear, align_corners=False): the two source indices and weights of destination index dst.
struct Tap { int i0, i1; float l0, l1; };
__host__ __device__ inline Tap axis_tap(int dst, float scale, int g) {
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    if (src < 0.0f) src = 0.0f;
    Tap t;
    t.i0 = (int)src;
    if (t.i0 > g - 1) t.i0 = g - 1;  // never taken (src < g - 0.5): keeps a wrong scale from becoming a wrong address
    t.i1 = t.i0 + (t.i0 < g - 1);
    t.l1 = src - (float)t.i0;
    t.l0 = 1.0f - t.l1;
    return t;
}

// block j of an axis: the pixels lo .. lo + u - 1 with lo = u * j - (u + 1) / 2, clipped to 0 .. U - 1
__host__ __device__ inline int block_lo(int j, int u) { return u * j - (u + 1) / 2; }

// SW block columns per strip, WGS workgroups per strip; a window is at most WH x WW cells; slices of 1 << LOG_BS bins
struct DepthPlan { int SW, WGS, WH, WW, LOG_BS; };

template <int BU>
__global__ __launch_bounds__(DEPTH_THREADS) void depth_expect_kernel(const float *__restrict__ logits, int ld_logits, size_t image_stride,
                                                                     const float *__restrict__ cls, int ld_cls,
                                                                     const float *__restrict__ centres, float *__restrict__ dmap,
                                                                     size_t dmap_image_stride, int images, int g, int bins, float min_depth,
                                                                     float max_depth, DepthPlan pl) {
    extern __shared__ float lds[];
    float *cen = lds, *win = lds + DEPTH_MAX_BINS;
    const int tid = threadIdx.x, U = BU * g, nb = g + 1;
    const int strip = blockIdx.x / pl.WGS, bx_lo = strip * pl.SW, sw = min(pl.SW, nb - bx_lo);
    const long long id_lo = (long long)(blockIdx.x % pl.WGS) * DEPTH_THREADS, ids = (long long)sw * nb;
    if (id_lo >= ids) return;  // a narrower last strip needs fewer workgroups: the whole workgroup leaves
    const long long id = id_lo + tid;
    const bool active = id < ids;
    const int by = active ? (int)(id / sw) : 0, bx = bx_lo + (active ? (int)(id % sw) : 0);
    // the window: the cell rows and columns of the workgroup's blocks (a block reads cells j - 1 and j; the first block 0 and 1)
    const int by_first = (int)(id_lo / sw), by_last = (int)((min(id_lo + DEPTH_THREADS, ids) - 1) / sw);
    const int r_lo = max(by_first - 1, 0), c_lo = max(bx_lo - 1, 0);
    const int wh = min(min(max(by_last, 1), g - 1) - r_lo + 1, pl.WH), ww = min(min(max(bx_lo + sw - 1, 1), g - 1) - c_lo + 1, pl.WW);
    const int cells = wh * ww;
    // this lane's block: per row and column the stated weights; the cells are those of its first pixel inside the map
    const float scale = (float)g / (float)U;
    const int y_lo = block_lo(by, BU), x_lo = block_lo(bx, BU);
    float ly0[BU], ly1[BU], lx0[BU], lx1[BU];
#pragma unroll
    for (int k = 0; k < BU; ++k) {
        const Tap ty = axis_tap(min(max(y_lo + k, 0), U - 1), scale, g), tx = axis_tap(min(max(x_lo + k, 0), U - 1), scale, g);
        ly0[k] = ty.l0; ly1[k] = ty.l1; lx0[k] = tx.l0; lx1[k] = tx.l1;
    }
    const Tap fy = axis_tap(max(y_lo, 0), scale, g), fx = axis_tap(max(x_lo, 0), scale, g);
    const int ra = min(max(fy.i0 - r_lo, 0), wh - 1), rb = min(max(fy.i1 - r_lo, 0), wh - 1);
    const int ca = min(max(fx.i0 - c_lo, 0), ww - 1), cb = min(max(fx.i1 - c_lo, 0), ww - 1);
    const int BS = 1 << pl.LOG_BS, csp = BS + 1;
    const float *p00 = win + (ra * ww + ca) * csp, *p01 = win + (ra * ww + cb) * csp;
    const float *p10 = win + (rb * ww + ca) * csp, *p11 = win + (rb * ww + cb) * csp;
    const int sb = tid & (BS - 1), scell = tid >> pl.LOG_BS, scells = DEPTH_THREADS >> pl.LOG_BS;

    for (int img = blockIdx.y; img < images; img += gridDim.y) {
        const float *src = logits + (size_t)img * image_stride;
        const float *z = cls ? cls + (size_t)img * ld_cls : nullptr;
        float s[BU][BU], t[BU][BU];
#pragma unroll
        for (int ky = 0; ky < BU; ++ky)
#pragma unroll
            for (int kx = 0; kx < BU; ++kx) s[ky][kx] = t[ky][kx] = 0.0f;
        for (int b_lo = 0; b_lo < bins; b_lo += BS) {
            const int bs = min(BS, bins - b_lo);
            __syncthreads();  // the previous slice (or image) has been read
            if (b_lo == 0 && img == (int)blockIdx.y)
                for (int b = tid; b < bins; b += DEPTH_THREADS) cen[b] = centres[b];
            if (sb < bs) {
                const float zb = z ? z[b_lo + sb] : 0.0f;
                for (int cell = scell; cell < cells; cell += scells) {
                    const int wr = cell / ww, wc = cell - wr * ww;
                    const float v = src[((size_t)(r_lo + wr) * g + (c_lo + wc)) * ld_logits + b_lo + sb];
                    win[cell * csp + sb] = z ? v + zb : v;
                }
            }
            __syncthreads();
            if (!active) continue;
            for (int b = 0; b < bs; ++b) {
                const float v00 = p00[b], v01 = p01[b], v10 = p10[b], v11 = p11[b], c = cen[b_lo + b];
                float h0[BU], h1[BU];
#pragma unroll
                for (int kx = 0; kx < BU; ++kx) {
                    h0[kx] = lx0[kx] * v00 + lx1[kx] * v01;
                    h1[kx] = lx0[kx] * v10 + lx1[kx] * v11;
                }
#pragma unroll
                for (int ky = 0; ky < BU; ++ky)
#pragma unroll
                    for (int kx = 0; kx < BU; ++kx) {
                        const float v = ly0[ky] * h0[kx] + ly1[ky] * h1[kx];
                        const float r = (v < 0.0f ? 0.0f : v) + 0.1f;  // a NaN stays a NaN
                        s[ky][kx] = s[ky][kx] + r;
                        t[ky][kx] = t[ky][kx] + r * c;
                    }
            }
        }
        if (!active) continue;
        float *dst = dmap + (size_t)img * dmap_image_stride;
#pragma unroll
        for (int ky = 0; ky < BU; ++ky) {
            const int y = y_lo + ky;
            if (y < 0 || y >= U) continue;
#pragma unroll
            for (int kx = 0; kx < BU; ++kx) {
                const int x = x_lo + kx;
                if (x < 0 || x >= U) continue;
                float d = t[ky][kx] / s[ky][kx];
                d = d < min_depth ? min_depth : d > max_depth ? max_depth : d;
                dst[(size_t)y * U + x] = d;
            }
        }
    }
}

// stage 2: out[y][x] = the bilinear interpolation of the U x U depth map, one thread per output pixel, the images along grid.y
__global__ __launch_bounds__(DEPTH_THREADS) void depth_resize_kernel(const float *__restrict__ dmap, size_t dmap_image_stride, int U,
                                                                     float *__restrict__ out, size_t out_image_stride, int images, int out_h,
                                                                     int out_w) {
    const int idx = blockIdx.x * DEPTH_THREADS + threadIdx.x;  // out_h * out_w <= 2^24
    if (idx >= out_h * out_w) return;
    const int y = idx / out_w, x = idx - y * out_w;
    const Tap ty = axis_tap(y, (float)U / (float)out_h, U), tx = axis_tap(x, (float)U / (float)out_w, U);
    const size_t o00 = (size_t)ty.i0 * U + tx.i0, o01 = (size_t)ty.i0 * U + tx.i1, o10 = (size_t)ty.i1 * U + tx.i0, o11 = (size_t)ty.i1 * U + tx.i1;
    for (int img = blockIdx.y; img < images; img += gridDim.y) {
        const float *src = dmap + (size_t)img * dmap_image_stride;
        out[(size_t)img * out_image_stride + idx] = ty.l0 * (tx.l0 * src[o00] + tx.l1 * src[o01]) + ty.l1 * (tx.l0 * src[o10] + tx.l1 * src[o11]);
    }
}

// every pixel of block j reads the cells of the block's first pixel inside the map: the kernel's premise, with its own expressions
bool blocks_share_cells(int g, int u) {
    const int U = u * g;
    const float scale = (float)g / (float)U;
    for (int j = 0; j <= g; ++j) {
        const int lo = block_lo(j, u) < 0 ? 0 : block_lo(j, u), hi = block_lo(j, u) + u - 1 < U - 1 ? block_lo(j, u) + u - 1 : U - 1;
        if (lo > hi) continue;  // u = 1: block 0 is empty
        const Tap f = axis_tap(lo, scale, g);
        for (int p = lo + 1; p <= hi; ++p) {
            const Tap t = axis_tap(p, scale, g);
            if (t.i0 != f.i0 || t.i1 != f.i1) return false;
        }
    }
    return true;
}

// the most cells a workgroup's window holds in a strip `w` block columns wide (an upper bound)
long long strip_cells(int w, int g, int *wh, int *ww) {
    int rows = (DEPTH_THREADS - 2 + w) / w + 1;  // block rows that 256 consecutive numbers touch
    if (rows > g + 1) rows = g + 1;
    const int h = rows + 1 < g ? rows + 1 : g, c = w + 1 < g ? w + 1 : g;
    if (h > *wh) *wh = h;
    if (c > *ww) *ww = c;
    return (long long)h * c;
}

}  // namespace

extern "C" {

int vithip_dense_depth_f32(vithip_stream_t stream, const float *logits, int ld_logits, size_t image_stride, const float *cls_logits, int ld_cls,
                           const float *centres, float *out, size_t out_image_stride, float *scratch, int images, int g, int bins, int upsample,
                           float min_depth, float max_depth, int out_h, int out_w) {
    const int bad = static_cast<int>(hipErrorInvalidValue);
    if (!logits || !centres || !out || images < 1 || g < 1 || g > 46340 /* g * g is an int */) return bad;
    if (bins < 2 || bins > DEPTH_MAX_BINS || upsample < 1 || upsample > 8) return bad;
    if (out_h < 1 || out_h > DEPTH_MAX_OUT || out_w < 1 || out_w > DEPTH_MAX_OUT || ld_logits < bins || (cls_logits && ld_cls < bins)) return bad;
    if (!std::isfinite(min_depth) || !std::isfinite(max_depth) || !(0.0f < min_depth && min_depth < max_depth)) return bad;
    const size_t P = (size_t)g * g;
    if (image_stride < (P - 1) * (size_t)ld_logits + (size_t)bins || out_image_stride < (size_t)out_h * out_w) return bad;
    const int U = upsample * g;
    const bool direct = out_h == U && out_w == U;  // stage 2 is the identity: stage 1 stores the rows of `out`
    if (!direct && !scratch) return bad;
    if (!blocks_share_cells(g, upsample)) return bad;  // not reached for u = 1..8 (see the head of this file)

    DepthPlan pl;
    const int nb = g + 1;
    const int strips = (nb + DEPTH_THREADS - 1) / DEPTH_THREADS;  // of nearly equal widths: none is narrow enough to span many rows
    pl.SW = (nb + strips - 1) / strips;
    pl.WGS = (int)(((long long)pl.SW * nb + DEPTH_THREADS - 1) / DEPTH_THREADS);
    pl.WH = pl.WW = 1;
    long long cells = strip_cells(pl.SW, g, &pl.WH, &pl.WW);  // sets WH and WW
    if (nb - (strips - 1) * pl.SW != pl.SW) strip_cells(nb - (strips - 1) * pl.SW, g, &pl.WH, &pl.WW);
    cells = (long long)pl.WH * pl.WW;
    pl.LOG_BS = 0;
    while ((2 << pl.LOG_BS) <= DEPTH_MAX_SLICE && (1 << pl.LOG_BS) < bins && cells * ((2 << pl.LOG_BS) + 1) <= DEPTH_LDS_FLOATS) ++pl.LOG_BS;
    if (cells * ((1 << pl.LOG_BS) + 1) > DEPTH_LDS_FLOATS) return bad;  // a window stays below 1600 cells: not reached
    const size_t lds = ((size_t)DEPTH_MAX_BINS + (size_t)cells * ((1 << pl.LOG_BS) + 1)) * sizeof(float);
    const long long wgs = (long long)strips * pl.WGS;
    if (wgs > 0x7fffffffLL) return bad;  // 46341^2 blocks are 2^23 workgroups
    const unsigned gy = (unsigned)(images < 65535 ? images : 65535);
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *dmap = direct ? out : scratch;
    const size_t dmap_stride = direct ? out_image_stride : (size_t)U * U;
#define DEPTH_LAUNCH(BU)                                                                                                                   \
    case BU:                                                                                                                               \
        hipLaunchKernelGGL((depth_expect_kernel<BU>), dim3((unsigned)wgs, gy), dim3(DEPTH_THREADS), lds, s, logits, ld_logits, image_stride, \
                           cls_logits, ld_cls, centres, dmap, dmap_stride, images, g, bins, min_depth, max_depth, pl);                     \
        break
    switch (upsample) {
        DEPTH_LAUNCH(1); DEPTH_LAUNCH(2); DEPTH_LAUNCH(3); DEPTH_LAUNCH(4); DEPTH_LAUNCH(5); DEPTH_LAUNCH(6); DEPTH_LAUNCH(7); DEPTH_LAUNCH(8);
    }
#undef DEPTH_LAUNCH
    int rc = static_cast<int>(hipGetLastError());
    if (rc || direct) return rc;
    const unsigned gx = (unsigned)((out_h * out_w + DEPTH_THREADS - 1) / DEPTH_THREADS);
    hipLaunchKernelGGL(depth_resize_kernel, dim3(gx, gy), dim3(DEPTH_THREADS), 0, s, scratch, (size_t)U * U, U, out, out_image_stride, images,
                       out_h, out_w);
    return static_cast<int>(hipGetLastError());
}

}  // extern "C"
