// csrc/vit_preproc.hip -- decoded 8-bit images of any size -> the model's normalised fp32 input, in one kernel:
//
//   Resize(R) -> CenterCrop(S) -> ToTensor() -> Normalize(mean, std)
//
// torchvision's evaluation transform on the images a dataset hands it, i.e. Pillow's Image.resize(..., BILINEAR) on 8 bits per
// channel, bit for bit (include/vit_hip_kernels.h states the arithmetic; tests/preproc_model.py restates it in numpy):
//   * per axis a coefficient table in IEEE double (no fused multiply-add, true divisions), turned into 2^22 fixed point;
//   * a pass is an int32 sum 2^21 + sum pixel * k, shifted right by 22 and clamped to a byte (from above; bicubic: from below too);
//   * the horizontal pass is rounded to bytes BEFORE the vertical pass reads it; an axis that keeps its size is skipped;
//   * the byte of the vertical pass goes through the formula of csrc/vit_input.hip into dst [n][C][S][S].
// Only the S x S pixels of the crop are computed, and no resized 8-bit image is stored in HBM.
//
// Structure: a workgroup per image and tile of the crop (tw columns x th rows, all channels).
//   1. the tile's coefficients, one thread per output column / row, fp64, into LDS (a few dozen operations each);
//   2. horizontal pass of the source rows the tile's vertical supports touch, crop columns only, as bytes into LDS, one plane per
//      channel ([row][channel][column], so that four neighbouring columns of a channel are one dword);
//   3. vertical pass out of LDS: a thread takes four neighbouring columns of one channel of one output row -- one dword read per
//      tap -- normalises them and stores 16 bytes into the channel plane, as csrc/vit_input.hip does.
// Every source byte of the tile's window is read once per channel-tap from global memory (byte loads: a source has no alignment
// beyond a byte), nothing of the horizontal pass is repeated inside a tile; tiles of one image repeat the rows their vertical supports
// share (2 * support of ~th * scale rows).  The tile adapts to the scale (tile_shape): its width so that the column coefficients fit
// their LDS table, its height so that the rows of the horizontal pass fit theirs, for every size the launcher accepts.
//
// The filter is a template parameter F next to the channel count: VITHIP_RESIZE_BILINEAR is the kernel above, VITHIP_RESIZE_BICUBIC
// (Pillow's BICUBIC, the evaluation transform of DINOv2, DINO, DeiT, MAE and timm's vit_* configs; tests/preproc_filter_model.py) has
// twice the support, signed coefficients (rounded away from zero), a pass that can leave [0, 255] on both sides and therefore
// clamps on both, and coefficient tables of twice the size, so that both filters take the same sources and the production shapes
// keep a tile as wide as the crop.  Nothing of the bilinear instantiation depends on the other one.
//
// Images of one call differ in size, so each has a record (pointer, sizes, crop origin).  The records travel BY VALUE as kernel
// arguments, PP_RECS per launch: the call stays asynchronous, borrows the caller's array only for its duration, and needs neither
// a device table nor an ordering against the caller's next call.
//
// Floating-point contraction: this file is compiled with -ffp-contract=off (FLAGS_vit_preproc in the package Makefile).  A fused
// multiply-add in `center - support + 0.5` or `(x + xmin - center + 0.5) * ss` changes a last bit and, now and then, a truncation.
// No fast-math: the fp64 and fp32 divisions are the correctly rounded ones.
#include <hip/hip_runtime.h>

#include <cmath>

#include "vit_hip_kernels.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int PP_THREADS = 256;
constexpr int PP_MAX_CHANS = 4;
constexpr int PP_RECS = 64;        // images per launch: 64 records of 32 bytes in the kernel arguments
constexpr int PP_MAX_TILE = 256;   // columns / rows of a tile at most (the xmin / count tables)
constexpr int PP_KCAP = 1024;      // coefficients per axis of a tile (ints in LDS), bilinear ...
constexpr int PP_KCAP_CUBIC = 2048;  // ... and bicubic, which has twice the taps
constexpr int PP_HBYTES = 32768;   // bytes of the horizontal pass a tile keeps in LDS
constexpr int PP_MAX_GRID_X = 4096;
constexpr int PP_PRECISION = 22;

struct pp_rec {
    const unsigned char *src;
    int h, w;       // source
    int oh, ow;     // resized
    int top, left;  // crop origin inside the resized image
};
static_assert(sizeof(pp_rec) == 32, "record size");

struct pp_batch {
    pp_rec r[PP_RECS];
};

struct pp_consts {
    float mean[PP_MAX_CHANS], std[PP_MAX_CHANS];
};

__host__ __device__ constexpr int kcap_of(int filter) { return filter == VITHIP_RESIZE_BICUBIC ? PP_KCAP_CUBIC : PP_KCAP; }

// most taps an output index of this axis can have: xmax - xmin < 2 * support + 1, support = fs (bilinear) or 2 * fs (bicubic)
__host__ __device__ inline int tap_bound(int in, int out, int filter) {
    if (in == out) return 1;
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    return filter == VITHIP_RESIZE_BICUBIC ? (int)(4.0 * fs) + 2 : (int)(2.0 * fs) + 2;
}

struct pp_tile {
    int tw, th;  // columns (a multiple of 4) and rows of a tile
    int cx, cy;  // tap bounds = strides of the coefficient tables
    int rows;    // source rows the LDS image holds for this width
};

// The tile of one image.  Width: the column coefficients fit the filter's table (kcap_of), and at least cy + 1 rows of that width fit
// PP_HBYTES.  Height: th output rows read at most (th - 1) * scale + cy source rows, which must fit too, as must the row coefficients.
// The launcher bounds the scale (a source's shorter side is at most 64 x resize_shorter, so the scale of either axis stays below
// 64 * (R + 1) / R <= 80), so cx, cy <= 162 (bilinear) or 322 (bicubic: 2048 / 322 = 6 columns, 32768 / (323 * 4) = 25 columns) and
// every limit leaves tw >= 4, th >= 1.
__host__ __device__ inline pp_tile tile_shape(const pp_rec &r, int S, int C, int filter) {
    const int kcap = kcap_of(filter);
    pp_tile t;
    t.cx = tap_bound(r.w, r.ow, filter);
    t.cy = tap_bound(r.h, r.oh, filter);
    int tw = S < PP_MAX_TILE ? S : PP_MAX_TILE;
    int lim = (kcap / t.cx) & ~3;
    if (tw > lim) tw = lim;
    lim = (PP_HBYTES / ((t.cy + 1) * C)) & ~3;
    if (tw > lim) tw = lim;
    if (tw < 4) tw = 4;
    t.tw = tw;
    t.rows = PP_HBYTES / (tw * C);
    const double scale = r.h == r.oh ? 1.0 : (double)r.h / (double)r.oh;
    const double fit = (double)(t.rows - t.cy - 1) / scale;
    int th = fit < 0.0 ? 1 : (fit > (double)PP_MAX_TILE ? PP_MAX_TILE : 1 + (int)fit);
    if (th > PP_MAX_TILE) th = PP_MAX_TILE;
    if (th > kcap / t.cy) th = kcap / t.cy;
    if (th > S) th = S;
    if (th < 1) th = 1;
    t.th = th;
    return t;
}

__host__ __device__ inline int tiles_of(const pp_tile &t, int S) { return ((S + t.tw - 1) / t.tw) * ((S + t.th - 1) / t.th); }

// Pillow's filters: the weight of a tap at signed distance d (in units of the filter's scale) from the centre
template <int F>
__device__ inline double filter_weight(double d) {
    const double t = fabs(d);
    if (F == VITHIP_RESIZE_BICUBIC) {  // Keys' cubic, a = -0.5
        const double a = -0.5;
        if (t < 1.0) return ((a + 2.0) * t - (a + 3.0)) * t * t + 1;
        if (t < 2.0) return (((t - 5) * t + 8) * t - 4) * a;
        return 0.0;
    }
    return t < 1.0 ? 1.0 - t : 0.0;
}

// Pillow's precompute_coeffs + normalize_coeffs_8bpc for output index xx of one axis (support = max(scale, 1), bicubic twice that).
template <int F>
__device__ inline void coefficients(int in, int out, int xx, int bound, int *k, int *pmin, int *pcnt) {
    if (in == out) {  // the axis is skipped: the byte passes through
        *pmin = xx;
        *pcnt = 1;
        k[0] = 1 << PP_PRECISION;
        return;
    }
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = F == VITHIP_RESIZE_BICUBIC ? 2.0 * fs : fs, ss = 1.0 / fs;
    const double center = ((double)xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    int cnt = xmax - xmin;
    if (cnt > bound) cnt = bound;  // never taken (tap_bound); keeps the table writes inside the tile's slot whatever happens
    if (cnt < 0) cnt = 0;
    double ww = 0.0;
    for (int x = 0; x < cnt; ++x) ww += filter_weight<F>(((double)(x + xmin) - center + 0.5) * ss);
    for (int x = 0; x < cnt; ++x) {
        double w = filter_weight<F>(((double)(x + xmin) - center + 0.5) * ss);
        if (ww != 0.0) w /= ww;
        k[x] = F == VITHIP_RESIZE_BICUBIC && w < 0.0 ? (int)(-0.5 + w * 4194304.0) : (int)(0.5 + w * 4194304.0);
    }
    *pmin = xmin;
    *pcnt = cnt;
}

// the byte of a pass: bilinear sums cannot fall below 0, bicubic ones can
template <int F>
__device__ inline int clamp_byte(int v) {
    if (F == VITHIP_RESIZE_BICUBIC && v < 0) return 0;
    return v > 255 ? 255 : v;
}

// grid: x over the tiles of an image (a workgroup loops when an image has more), y over the records of the launch
template <int C, int F>
__global__ __launch_bounds__(PP_THREADS) void images_u8_resize_crop_kernel(pp_batch batch, float *__restrict__ dst, int S, pp_consts nk) {
    __shared__ unsigned int hb[PP_HBYTES / 4];  // horizontal pass: [row][channel][tw bytes]
    __shared__ int kx[kcap_of(F)], ky[kcap_of(F)];
    __shared__ int xmin[PP_MAX_TILE], xcnt[PP_MAX_TILE], ymin[PP_MAX_TILE], ycnt[PP_MAX_TILE];

    const pp_rec rec = batch.r[blockIdx.y];
    const pp_tile t = tile_shape(rec, S, C, F);
    const int tiles_x = (S + t.tw - 1) / t.tw, ntiles = tiles_of(t, S);
    const int twq = t.tw / 4;  // dwords per channel row of the LDS image
    float *const out = dst + (size_t)blockIdx.y * C * S * S;
    const int tid = threadIdx.x;

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int i0 = (tile / tiles_x) * t.th, j0 = (tile % tiles_x) * t.tw;
        const int th = S - i0 < t.th ? S - i0 : t.th, tw = S - j0 < t.tw ? S - j0 : t.tw;  // tw stays a multiple of 4: S and t.tw are

        // 1. coefficients of the tile's columns and rows
        for (int e = tid; e < tw + th; e += PP_THREADS) {
            if (e < tw) coefficients<F>(rec.w, rec.ow, rec.left + j0 + e, t.cx, kx + e * t.cx, xmin + e, xcnt + e);
            else coefficients<F>(rec.h, rec.oh, rec.top + i0 + (e - tw), t.cy, ky + (e - tw) * t.cy, ymin + (e - tw), ycnt + (e - tw));
        }
        __syncthreads();

        // 2. horizontal pass of source rows [r0, r1): a thread takes four columns of one channel of one row
        const int r0 = ymin[0];
        int r1 = ymin[th - 1] + ycnt[th - 1];
        if (r1 > r0 + t.rows) r1 = r0 + t.rows;  // never taken (tile_shape); keeps the image inside hb whatever happens
        const int nrows = r1 - r0, quads = tw / 4;
        for (int e = tid; e < nrows * C * quads; e += PP_THREADS) {
            const int q = e % quads, c = (e / quads) % C, r = e / (quads * C);
            const unsigned char *row = rec.src + ((size_t)(r0 + r) * rec.w) * C + c;
            unsigned int packed = 0;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int j = 4 * q + p, n = xcnt[j];
                const int *k = kx + j * t.cx;
                const unsigned char *s = row + (size_t)xmin[j] * C;
                int acc = 1 << (PP_PRECISION - 1);
                for (int x = 0; x < n; ++x) acc += (int)s[x * C] * k[x];
                acc >>= PP_PRECISION;
                packed |= (unsigned int)clamp_byte<F>(acc) << (8 * p);
            }
            hb[(r * C + c) * twq + q] = packed;
        }
        __syncthreads();

        // 3. vertical pass, normalisation, 16-byte stores into the channel planes
        for (int e = tid; e < th * C * quads; e += PP_THREADS) {
            const int q = e % quads, c = (e / quads) % C, i = e / (quads * C);
            int n = ycnt[i];
            const int y0 = ymin[i] - r0;
            if (y0 + n > nrows) n = nrows - y0;  // never taken
            const int *k = ky + i * t.cy;
            int acc[4] = {1 << (PP_PRECISION - 1), 1 << (PP_PRECISION - 1), 1 << (PP_PRECISION - 1), 1 << (PP_PRECISION - 1)};
            for (int y = 0; y < n; ++y) {
                const unsigned int d = hb[((y0 + y) * C + c) * twq + q];
                const int kk = k[y];
#pragma unroll
                for (int p = 0; p < 4; ++p) acc[p] += (int)((d >> (8 * p)) & 0xffu) * kk;
            }
            f32x4 v;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const float u = (float)clamp_byte<F>(acc[p] >> PP_PRECISION);
                v[p] = (u / 255.0f - nk.mean[c]) / nk.std[c];
            }
            *reinterpret_cast<f32x4 *>(out + ((size_t)c * S + (i0 + i)) * S + j0 + 4 * q) = v;
        }
        __syncthreads();  // the next tile overwrites the tables
    }
}

template <int C>
int launch(hipStream_t s, const pp_batch &b, int count, int grid_x, float *dst, int S, const pp_consts &nk, int filter) {
    if (filter == VITHIP_RESIZE_BICUBIC)
        hipLaunchKernelGGL((images_u8_resize_crop_kernel<C, VITHIP_RESIZE_BICUBIC>), dim3(grid_x, count), dim3(PP_THREADS), 0, s, b, dst, S, nk);
    else
        hipLaunchKernelGGL((images_u8_resize_crop_kernel<C, VITHIP_RESIZE_BILINEAR>), dim3(grid_x, count), dim3(PP_THREADS), 0, s, b, dst, S, nk);
    return static_cast<int>(hipGetLastError());
}

// round half to even of d / 2, d >= 0 (Python's round((o - S) / 2.0))
int half_rne(int d) {
    const int m = d / 2;
    return (d & 1) ? m + (m & 1) : m;
}

// torchvision's Resize(R) + CenterCrop(S) geometry of one source; false when the launcher refuses it
bool make_record(const vithip_image_u8 &im, int S, int R, pp_rec *r) {
    if (!im.pixels || im.height < 1 || im.height > 16384 || im.width < 1 || im.width > 16384) return false;
    const int h = im.height, w = im.width, shorter = w <= h ? w : h, longer = w <= h ? h : w;
    if ((long long)shorter > 64LL * R) return false;
    const int L = (int)(((long long)R * longer) / shorter);
    r->src = im.pixels;
    r->h = h;
    r->w = w;
    r->oh = w <= h ? L : R;
    r->ow = w <= h ? R : L;
    r->top = half_rne(r->oh - S);
    r->left = half_rne(r->ow - S);
    return true;
}

}  // namespace

extern "C" {

int vithip_images_u8_resize_crop_check_filter(const vithip_image_u8 *images, int n, int img_size, int chans, int resize_shorter, int filter) {
    if (filter != VITHIP_RESIZE_BILINEAR && filter != VITHIP_RESIZE_BICUBIC) return -1;
    if (!images || n < 1 || chans < 1 || chans > PP_MAX_CHANS || img_size < 4 || img_size % 4 || resize_shorter < img_size ||
        resize_shorter > 4096)
        return -1;
    for (int i = 0; i < n; ++i) {
        pp_rec r;
        if (!make_record(images[i], img_size, resize_shorter, &r)) return i + 1;
    }
    return 0;
}

int vithip_images_u8_resize_crop_check(const vithip_image_u8 *images, int n, int img_size, int chans, int resize_shorter) {
    return vithip_images_u8_resize_crop_check_filter(images, n, img_size, chans, resize_shorter, VITHIP_RESIZE_BILINEAR);
}

int vithip_images_u8_resize_crop_to_f32_filter(vithip_stream_t stream, const vithip_image_u8 *images, int n, float *dst, int img_size,
                                               int chans, int resize_shorter, int filter, const float *mean, const float *std) {
    if (!dst || !mean || !std || (reinterpret_cast<size_t>(dst) & 15)) return static_cast<int>(hipErrorInvalidValue);
    if (vithip_images_u8_resize_crop_check_filter(images, n, img_size, chans, resize_shorter, filter) != 0)
        return static_cast<int>(hipErrorInvalidValue);
    pp_consts nk = {};
    for (int c = 0; c < chans; ++c) {
        if (!std::isfinite(mean[c]) || !std::isfinite(std[c]) || std[c] == 0.0f) return static_cast<int>(hipErrorInvalidValue);
        nk.mean[c] = mean[c];
        nk.std[c] = std[c];
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t img = (size_t)chans * img_size * img_size;
    for (int first = 0; first < n; first += PP_RECS) {
        const int count = n - first < PP_RECS ? n - first : PP_RECS;
        pp_batch b = {};
        int grid_x = 1;
        for (int i = 0; i < count; ++i) {
            make_record(images[first + i], img_size, resize_shorter, &b.r[i]);
            const int tiles = tiles_of(tile_shape(b.r[i], img_size, chans, filter), img_size);
            if (tiles > grid_x) grid_x = tiles;
        }
        if (grid_x > PP_MAX_GRID_X) grid_x = PP_MAX_GRID_X;
        float *d = dst + (size_t)first * img;
        int rc;
        switch (chans) {
            case 1: rc = launch<1>(s, b, count, grid_x, d, img_size, nk, filter); break;
            case 2: rc = launch<2>(s, b, count, grid_x, d, img_size, nk, filter); break;
            case 3: rc = launch<3>(s, b, count, grid_x, d, img_size, nk, filter); break;
            default: rc = launch<4>(s, b, count, grid_x, d, img_size, nk, filter); break;
        }
        if (rc) return rc;
    }
    return 0;
}

int vithip_images_u8_resize_crop_to_f32(vithip_stream_t stream, const vithip_image_u8 *images, int n, float *dst, int img_size, int chans,
                                        int resize_shorter, const float *mean, const float *std) {
    return vithip_images_u8_resize_crop_to_f32_filter(stream, images, n, dst, img_size, chans, resize_shorter, VITHIP_RESIZE_BILINEAR, mean,
                                                      std);
}

}  // extern "C"
