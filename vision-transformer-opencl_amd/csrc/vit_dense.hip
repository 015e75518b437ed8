// csrc/vit_dense.hip -- the dense linear head's tail: per-pixel labels from the token-major logits [P][classes] of a g x g patch
// grid (P = g * g), without a full-resolution logit anywhere in memory; and the channel-major grid [classes][P] of the same logits.
//
// vithip_dense_upsample_argmax_f32: F.interpolate(mode="bilinear", align_corners=False) of every class map to out_h x out_w, then
// the argmax over the classes, as one byte per pixel.  The arithmetic is stated in vit_hip_kernels.h; every product and sum below is
// one rounded fp32 operation (this file is compiled with -ffp-contract=off, host side included: the launcher sizes the windows with
// the kernel's own expressions).
//
// Structure.  One workgroup of 256 threads per output tile, looping over the images of its grid row.  A tile is TH x TW pixels:
// thread t handles column t % TW and R consecutive rows (t / TW) * R .., TH = RB * R for RB row groups, TW * RB <= 256.  The source
// cells a tile reads form a window of wh x ww cells -- the rows i0(first row) .. i1(last row), the columns likewise: i0 and i1 are
// monotone in the pixel index.  The window is staged through LDS cell-major with the classes of a cell contiguous, cell stride
// CSP = an odd number of floats: lanes of a wave are neighbouring pixels, which read the same class of the same or of neighbouring
// cells -- equal addresses broadcast, different cells fall on different banks.  A thread then walks the classes once, keeps a running
// best (value, label) per pixel in registers and stores one byte per pixel; the lanes of a wave store consecutive bytes.  The R rows
// of a thread mostly share their two source rows when the map is upsampled: the four corner reads and the two horizontal sums of a
// class are taken once per pair of source rows, not once per pixel (the same expressions, so the same bits).
//
// What bounds it.  The window grows as out / g shrinks: at out <= g a tile touches four cells per pixel.  The launcher computes the
// exact largest window of the chosen tile shape (two short host loops over the tile rows and columns) and fits it into DENSE_LDS_FLOATS
// of LDS first by walking the classes in slices of CS (the running best carries over from slice to slice, two barriers per slice) and,
// once a slice would hold fewer than 8 classes, by halving the tile along its larger window side -- down to one pixel, whose window is
// 2 x 2 cells: every g, every output size up to 4096 x 4096 and every class count up to 255 runs.  At the sizes the head is for (g =
// 16 -> 224, g = 37 -> 518, 150 classes) the tile is 16 x 64 pixels and the whole window with all classes is ~13 KB: four workgroups
// per CU.  The kernel is bound by its LDS reads and VALU work (4 reads, 9 fp32 operations and a compare per pixel and class at
// worst), far above its HBM floor of logits read once per tile and one byte written per pixel.
//
// No atomics; a pixel's label depends on its image's logits alone, whatever the grid.  Non-finite logits travel through the
// arithmetic as IEEE says (0 * Inf = NaN); a NaN value is no candidate, a pixel without candidates gets DENSE_NONE = 255.
#include <hip/hip_runtime.h>

#include "vit_hip_kernels.h"

namespace {

constexpr int DENSE_THREADS = 256;
constexpr int DENSE_LDS_FLOATS = 10240;  // 40 KB: four workgroups per CU
constexpr int DENSE_MIN_SLICE = 8;       // classes per slice below which the tile shrinks instead
constexpr int DENSE_NONE = 255;
constexpr int DENSE_MAX_OUT = 4096;

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

// the largest number of source indices between i0(first) and i1(last) over the tiles of `tile` destination indices
int axis_window(int out, int tile, float scale, int g) {
    int w = 1;
    for (int lo = 0; lo < out; lo += tile) {
        const int hi = (lo + tile < out ? lo + tile : out) - 1;
        const int n = axis_tap(hi, scale, g).i1 - axis_tap(lo, scale, g).i0 + 1;
        if (n > w) w = n;
    }
    return w;
}

struct DenseTile { int TW, RB, R, WH, WW, CS; };  // tile = (RB * R) x TW pixels; window <= WH x WW cells; CS classes per slice

template <int R>
__global__ __launch_bounds__(DENSE_THREADS) void dense_upsample_argmax_kernel(const float *__restrict__ logits, int ld_logits,
                                                                              size_t image_stride, unsigned char *__restrict__ out,
                                                                              size_t out_image_stride, int images, int g, int classes,
                                                                              int out_h, int out_w, DenseTile tl) {
    extern __shared__ float win[];
    const int tid = threadIdx.x, TW = tl.TW, TH = tl.RB * R;
    const int tiles_x = (out_w + TW - 1) / TW;
    const int x_lo = (blockIdx.x % tiles_x) * TW, y_lo = (blockIdx.x / tiles_x) * TH;
    const int x_hi = min(x_lo + TW, out_w) - 1, y_hi = min(y_lo + TH, out_h) - 1;
    const float scale_y = (float)g / (float)out_h, scale_x = (float)g / (float)out_w;
    // the tile's window of source cells
    const int cy_lo = axis_tap(y_lo, scale_y, g).i0, cx_lo = axis_tap(x_lo, scale_x, g).i0;
    const int wh = min(axis_tap(y_hi, scale_y, g).i1 - cy_lo + 1, tl.WH), ww = min(axis_tap(x_hi, scale_x, g).i1 - cx_lo + 1, tl.WW);
    // this thread's pixels: column x, rows y0 .. y0 + R - 1
    const int tx = tid % TW, tg = tid / TW;
    const int x = x_lo + tx, y0 = y_lo + tg * R;
    const bool col_on = tg < tl.RB && x <= x_hi;
    const Tap cx = axis_tap(col_on ? x : x_lo, scale_x, g);
    const int c0 = min(cx.i0 - cx_lo, ww - 1), c1 = min(cx.i1 - cx_lo, ww - 1);
    int r0[R], r1[R];
    float l0y[R], l1y[R];
    bool on[R], fresh[R];
#pragma unroll
    for (int k = 0; k < R; ++k) {
        on[k] = col_on && y0 + k <= y_hi;
        const Tap ry = axis_tap(on[k] ? y0 + k : y_lo, scale_y, g);
        r0[k] = min(ry.i0 - cy_lo, wh - 1); r1[k] = min(ry.i1 - cy_lo, wh - 1);
        l0y[k] = ry.l0; l1y[k] = ry.l1;
        fresh[k] = k == 0 || r0[k] != r0[k - 1] || r1[k] != r1[k - 1];
    }
    const int cells = wh * ww;

    for (int img = blockIdx.y; img < images; img += gridDim.y) {
        const float *src = logits + (size_t)img * image_stride;
        float best[R];
        int label[R];
#pragma unroll
        for (int k = 0; k < R; ++k) { best[k] = -INFINITY; label[k] = DENSE_NONE; }
        for (int c_lo = 0; c_lo < classes; c_lo += tl.CS) {
            const int cs = min(tl.CS, classes - c_lo), csp = cs | 1;
            __syncthreads();  // the previous slice (or image) has been read
            for (int i = tid; i < cells * cs; i += DENSE_THREADS) {
                const int cell = i / cs, c = i - cell * cs;
                const int wr = cell / ww, wc = cell - wr * ww;
                win[cell * csp + c] = src[((size_t)(cy_lo + wr) * g + (cx_lo + wc)) * ld_logits + c_lo + c];
            }
            __syncthreads();
            if (!col_on) continue;
            for (int c = 0; c < cs; ++c) {
                float h0 = 0.0f, h1 = 0.0f;
#pragma unroll
                for (int k = 0; k < R; ++k) {
                    if (fresh[k]) {
                        const float *a = win + (r0[k] * ww) * csp + c, *b = win + (r1[k] * ww) * csp + c;
                        h0 = cx.l0 * a[c0 * csp] + cx.l1 * a[c1 * csp];
                        h1 = cx.l0 * b[c0 * csp] + cx.l1 * b[c1 * csp];
                    }
                    const float v = l0y[k] * h0 + l1y[k] * h1;
                    // higher wins; classes come in ascending order, so an equal value never replaces; NaN compares false twice
                    if (v > best[k] || (label[k] == DENSE_NONE && v == v)) { best[k] = v; label[k] = c_lo + c; }
                }
            }
        }
        unsigned char *dst = out + (size_t)img * out_image_stride;
#pragma unroll
        for (int k = 0; k < R; ++k)
            if (on[k]) dst[(size_t)(y0 + k) * out_w + x] = (unsigned char)label[k];
    }
}

// [P][classes] (ld) -> [classes][P] per image, through a 32 x 33 LDS tile: reads run along the classes, writes along the cells
__global__ __launch_bounds__(DENSE_THREADS) void dense_transpose_kernel(const float *__restrict__ logits, int ld_logits, size_t image_stride,
                                                                        float *__restrict__ out, size_t out_image_stride, int images,
                                                                        int cells, int classes) {
    __shared__ float tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int p_lo = blockIdx.x * 32;
    for (int img = blockIdx.y; img < images; img += gridDim.y) {
        const float *src = logits + (size_t)img * image_stride;
        float *dst = out + (size_t)img * out_image_stride;
        for (int c_lo = 0; c_lo < classes; c_lo += 32) {
            __syncthreads();
            for (int r = ty; r < 32; r += 8)
                if (p_lo + r < cells && c_lo + tx < classes) tile[r][tx] = src[(size_t)(p_lo + r) * ld_logits + c_lo + tx];
            __syncthreads();
            for (int r = ty; r < 32; r += 8)
                if (c_lo + r < classes && p_lo + tx < cells) dst[(size_t)(c_lo + r) * cells + p_lo + tx] = tile[tx][r];
        }
    }
}

bool dense_sizes_ok(int images, int g, int classes) {
    return images > 0 && g >= 1 && g <= 46340 /* g * g is an int */ && classes >= 1 && classes <= 255;
}

}  // namespace

extern "C" {

int vithip_dense_upsample_argmax_f32(vithip_stream_t stream, const float *logits, int ld_logits, size_t image_stride, unsigned char *out,
                                     size_t out_image_stride, int images, int g, int classes, int out_h, int out_w) {
    const int bad = static_cast<int>(hipErrorInvalidValue);
    if (!logits || !out || !dense_sizes_ok(images, g, classes)) return bad;
    if (out_h < 1 || out_h > DENSE_MAX_OUT || out_w < 1 || out_w > DENSE_MAX_OUT || ld_logits < classes) return bad;
    const size_t P = (size_t)g * g;
    if (image_stride < (P - 1) * (size_t)ld_logits + (size_t)classes || out_image_stride < (size_t)out_h * out_w) return bad;
    const float scale_y = (float)g / (float)out_h, scale_x = (float)g / (float)out_w;

    // the tile: as wide as the output needs (a power of two up to 64), 4 rows per thread where the output has them
    DenseTile t;
    t.TW = 1;
    while (t.TW < 64 && t.TW < out_w) t.TW *= 2;
    t.RB = DENSE_THREADS / t.TW;
    while (t.RB > 1 && t.RB / 2 >= out_h) t.RB /= 2;
    t.R = out_h >= 4 * t.RB ? 4 : out_h >= 2 * t.RB ? 2 : 1;
    for (;;) {
        t.WH = axis_window(out_h, t.RB * t.R, scale_y, g);
        t.WW = axis_window(out_w, t.TW, scale_x, g);
        const int cells = t.WH * t.WW;  // at most g * g, an int
        // the largest slice whose padded cells fit: cells * (CS | 1) <= DENSE_LDS_FLOATS
        int cs = DENSE_LDS_FLOATS / cells;
        if (cs > 0 && cs % 2 == 0) --cs;
        if (cs > classes) cs = classes;
        const int want = classes < DENSE_MIN_SLICE ? classes : DENSE_MIN_SLICE;
        if (cs >= want || (t.TW == 1 && t.RB == 1 && t.R == 1 && cs >= 1)) { t.CS = cs; break; }
        if (t.TW == 1 && t.RB == 1 && t.R == 1) return bad;  // a 2 x 2 window always fits: not reached
        if (t.WH >= t.WW && t.RB * t.R > 1) { if (t.R > 1) t.R /= 2; else t.RB /= 2; }
        else if (t.TW > 1) t.TW /= 2;
        else if (t.R > 1) t.R /= 2;
        else t.RB /= 2;
    }
    const size_t lds = (size_t)t.WH * t.WW * (size_t)(t.CS | 1) * sizeof(float);
    const long long tiles = (long long)((out_w + t.TW - 1) / t.TW) * ((out_h + t.RB * t.R - 1) / (t.RB * t.R));
    if (tiles > 0x7fffffffLL) return bad;  // 4096 x 4096 one-pixel tiles are 2^24
    const dim3 grid((unsigned)tiles, (unsigned)(images < 65535 ? images : 65535));
    hipStream_t s = static_cast<hipStream_t>(stream);
#define DENSE_LAUNCH(RR)                                                                                                          \
    hipLaunchKernelGGL((dense_upsample_argmax_kernel<RR>), grid, dim3(DENSE_THREADS), lds, s, logits, ld_logits, image_stride, out, \
                       out_image_stride, images, g, classes, out_h, out_w, t)
    if (t.R == 4) DENSE_LAUNCH(4);
    else if (t.R == 2) DENSE_LAUNCH(2);
    else DENSE_LAUNCH(1);
#undef DENSE_LAUNCH
    return static_cast<int>(hipGetLastError());
}

int vithip_dense_grid_f32(vithip_stream_t stream, const float *logits, int ld_logits, size_t image_stride, float *out,
                          size_t out_image_stride, int images, int g, int classes) {
    const int bad = static_cast<int>(hipErrorInvalidValue);
    if (!logits || !out || !dense_sizes_ok(images, g, classes) || ld_logits < classes) return bad;
    const size_t P = (size_t)g * g;
    if (image_stride < (P - 1) * (size_t)ld_logits + (size_t)classes || out_image_stride < P * (size_t)classes) return bad;
    const dim3 grid((unsigned)((P + 31) / 32), (unsigned)(images < 65535 ? images : 65535));
    hipLaunchKernelGGL(dense_transpose_kernel, grid, dim3(DENSE_THREADS), 0, static_cast<hipStream_t>(stream), logits, ld_logits,
                       image_stride, out, out_image_stride, images, (int)P, classes);
    return static_cast<int>(hipGetLastError());
}

}  // extern "C"
