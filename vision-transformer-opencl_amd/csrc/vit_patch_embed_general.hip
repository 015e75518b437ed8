// csrc/vit_patch_embed_general.hip -- fp32 patch embedding for any EVEN patch and image size (DINOv2's 14 x 14 patches:
// K = 3 * 14 * 14 = 588), as one implicit GEMM over the NCHW images on v_mfma_f32_32x32x2_f32.
//
//   x[img][0][:]   = cls + pos[0]
//   x[img][1+p][:] = conv_b + patch_p . conv_w + pos[1+p]            (the contract of vithip_patch_embed_f32)
//
// The A_PATCHES loader of vit_gemm.hip takes 16 bytes along a patch row and K steps of 32: patch % 4, img % 4, K % 32.  Here:
//  * Loads are 8 bytes wide.  With patch and img even, a pair of consecutive k (k even) lies inside one patch row and starts
//    8-byte aligned in the image; K = C * P * P is a multiple of 4, so a thread's four consecutive k (two pairs, possibly in two
//    pixel rows: 14 % 4 == 2) are inside K together or past it together, and conv_w [D][K] is read as it lies in pairs too.
//  * K tail: the last K step is filled with zeros when the tile is written to LDS.  Nothing past column K of a weight row or
//    past the last channel of an image is loaded (the thread loads k = 0 of its own row instead and the value is dropped), so no
//    out-of-range datum is ever multiplied by zero.  Rows past M = n * patches and weight rows past D are clamped to the last
//    row on the load side and never stored.
//  * k runs ASCENDING from a zero accumulator: MFMA number j of a K step multiplies k = 2j (lanes 0-31) and k = 2j + 1 (lanes
//    32-63), and the instruction adds its two products one after the other (tools/probes/mfma_order_probe.hip).  An LDS row holds
//    the even k of a step in floats 0..15 and the odd k in floats 16..31, so a lane still fetches its operands 16 bytes at a time.
//    The epilogue adds the bias, then pos.  An output row is therefore the same fmaf chain wherever its tile sits: its bits do
//    not depend on the batch or on the image's place in it.
//  * Workgroup = 256 threads = 4 waves, tile 128 x 64, K step 32, a wave owns 64 x 32 as two 32 x 32 accumulators.  Register-staged
//    double buffering: the loads of step t + 1 are issued before the matrix instructions of step t and written to the other LDS
//    buffer behind them; one barrier per step.  LDS rows are padded to 36 floats (conflict-free ds_read_b128, as vit_gemm.hip).
//  * Workgroup ids that share an XCD walk consecutive tiles, N fastest: the pixels of a tile row are fetched into that XCD's L2
//    once for all its N tiles.
#include "vit_gemm_common.hpp"

namespace {

using namespace vitgemm;

constexpr int GBM = 128, GBN = 64, GBK = 32, GLD = GBK + 4;
constexpr int A_PASSES = GBM / 32, B_PASSES = GBN / 32;  // a staging pass covers 32 tile rows: 8 threads x 4 k per row

struct EmbedParams {
    const float *images, *conv_w, *conv_b, *pos;
    float *x;
    int M, N, K;           // n * patches, embed_dim, chans * patch * patch
    int patches, grid, patch, img, chans;
    int prefix;            // rows in front of an image's patch rows in x: 1 + the register tokens
    int tiles_m, tiles_n;
};

__global__ __launch_bounds__(256, 2) void patch_embed_general_kernel(const EmbedParams p) {
    __shared__ __attribute__((aligned(16))) float lds[2 * (GBM + GBN) * GLD];
    float *const As0 = lds;
    float *const Bs0 = lds + 2 * GBM * GLD;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;

    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    const int tm = tile / p.tiles_n, tn = tile - tm * p.tiles_n;
    const int m0 = tm * GBM, n0 = tn * GBN;

    // ---- staging: thread = (row ld_row of a 32-row pass, k quad ld_kq): k = k0 + 4 ld_kq .. + 3 as two 8-byte pairs ----
    const int ld_row = tid >> 3, ld_kq = tid & 7;
    const float *a_src[A_PASSES], *b_src[B_PASSES];
#pragma unroll
    for (int i = 0; i < A_PASSES; ++i) {
        int m = m0 + ld_row + i * 32;
        m = m < p.M ? m : p.M - 1;
        const int im = m / p.patches, pp = m - im * p.patches;
        const int oh = pp / p.grid, ow = pp - oh * p.grid;
        a_src[i] = p.images + ((size_t)im * p.chans * p.img + (size_t)oh * p.patch) * p.img + ow * p.patch;
    }
#pragma unroll
    for (int i = 0; i < B_PASSES; ++i) {
        int n = n0 + ld_row + i * 32;
        n = n < p.N ? n : p.N - 1;
        b_src[i] = p.conv_w + (size_t)n * p.K;
    }

    f32x2 a_stage[A_PASSES][2], b_stage[B_PASSES][2];
    bool stage_valid = false;  // the staged k quad lies inside K (a quad is inside or outside as a whole: K % 4 == 0)

    const int pp2 = p.patch * p.patch;
    auto load_global = [&](int k0) {
        const int k = k0 + 4 * ld_kq;
        stage_valid = k < p.K;
        const int kk = stage_valid ? k : 0;  // past K: the row's own first elements, loaded and dropped
        // k = (ic, kh, kw); the second pair is two pixels on, or at the start of the next patch row / channel
        const int ic = kk / pp2, rem = kk - ic * pp2;
        const int kh = rem / p.patch, kw = rem - kh * p.patch;
        int ic1 = ic, kh1 = kh, kw1 = kw + 2;
        if (kw1 >= p.patch) { kw1 = 0; ++kh1; }
        if (kh1 >= p.patch) { kh1 = 0; ++ic1; }
        const int off0 = (ic * p.img + kh) * p.img + kw;
        const int off1 = (ic1 * p.img + kh1) * p.img + kw1;
#pragma unroll
        for (int i = 0; i < A_PASSES; ++i) {
            a_stage[i][0] = *reinterpret_cast<const f32x2 *>(a_src[i] + off0);
            a_stage[i][1] = *reinterpret_cast<const f32x2 *>(a_src[i] + off1);
        }
#pragma unroll
        for (int i = 0; i < B_PASSES; ++i) {
            b_stage[i][0] = *reinterpret_cast<const f32x2 *>(b_src[i] + kk);
            b_stage[i][1] = *reinterpret_cast<const f32x2 *>(b_src[i] + kk + 2);
        }
    };
    // LDS row: [even k of the step: 16 floats][odd k: 16 floats][4 floats of padding]; k = 4 q + e sits at (e & 1) * 16 + 2 q + (e >> 1)
    auto store_lds = [&](int buf) {
        float *As = As0 + buf * GBM * GLD, *Bs = Bs0 + buf * GBN * GLD;
        const f32x2 zero = f32x2{0.0f, 0.0f};
#pragma unroll
        for (int i = 0; i < A_PASSES; ++i) {
            float *row = As + (ld_row + i * 32) * GLD + 2 * ld_kq;
            const f32x2 v0 = a_stage[i][0], v1 = a_stage[i][1];
            *reinterpret_cast<f32x2 *>(row) = stage_valid ? f32x2{v0.x, v1.x} : zero;
            *reinterpret_cast<f32x2 *>(row + 16) = stage_valid ? f32x2{v0.y, v1.y} : zero;
        }
#pragma unroll
        for (int i = 0; i < B_PASSES; ++i) {
            float *row = Bs + (ld_row + i * 32) * GLD + 2 * ld_kq;
            const f32x2 v0 = b_stage[i][0], v1 = b_stage[i][1];
            *reinterpret_cast<f32x2 *>(row) = stage_valid ? f32x2{v0.x, v1.x} : zero;
            *reinterpret_cast<f32x2 *>(row + 16) = stage_valid ? f32x2{v0.y, v1.y} : zero;
        }
    };

    f32x16 acc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[i][v] = 0.0f;

    const int n_lane = n0 + wn * 32 + r;
    const float bias_r = n_lane < p.N ? p.conv_b[n_lane] : 0.0f;

    const int nk = (p.K + GBK - 1) / GBK;
    const int a_frag_off = (wm * 64 + r) * GLD + h * 16;
    const int b_frag_off = (wn * 32 + r) * GLD + h * 16;

    load_global(0);
    store_lds(0);
    __syncthreads();
    int cur = 0;
    for (int kt = 0; kt < nk; ++kt) {
        const bool more = kt + 1 < nk;  // workgroup-uniform
        if (more) load_global((kt + 1) * GBK);
        const float *As = As0 + cur * GBM * GLD + a_frag_off;
        const float *Bs = Bs0 + cur * GBN * GLD + b_frag_off;
#pragma unroll
        for (int q = 0; q < 4; ++q) {  // k = 8 q + 2 s + h
            const f32x4 a0 = *reinterpret_cast<const f32x4 *>(As + 4 * q);
            const f32x4 a1 = *reinterpret_cast<const f32x4 *>(As + 32 * GLD + 4 * q);
            const f32x4 b = *reinterpret_cast<const f32x4 *>(Bs + 4 * q);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], b[s], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], b[s], acc[1], 0, 0, 0);
            }
        }
        if (more) store_lds(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }

    // ---- epilogue: + bias, + pos, token-row remap (patch row m of image im is token row m + (im + 1) * prefix) ----
    if (n_lane >= p.N) return;
    // the 16 pos values of an accumulator are fetched (rows past M clamped) before its first store: a load waited for between
    // stores would serialise them on the write latency (vit_gemm_common.hpp, epilogue_store)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        float add[16];
        size_t orow[16];
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int m = m0 + wm * 64 + i * 32 + 4 * h + (v & 3) + 8 * (v >> 2);
            const int mc = m < p.M ? m : p.M - 1;
            const int im = mc / p.patches, pp = mc - im * p.patches;
            add[v] = p.pos[(size_t)(pp + 1) * p.N + n_lane];
            orow[v] = (size_t)(mc + (im + 1) * p.prefix);
        }
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int m = m0 + wm * 64 + i * 32 + 4 * h + (v & 3) + 8 * (v >> 2);
            if (m < p.M) p.x[orow[v] * p.N + n_lane] = acc[i][v] + bias_r + add[v];
        }
    }
}

bool aligned8(const void *ptr) { return (reinterpret_cast<size_t>(ptr) & 7) == 0; }

}  // namespace

extern "C" {

int vithip_patch_embed_f32_general_reg(vithip_stream_t stream, const float *images, const float *conv_w, const float *conv_b,
                                       const float *prefix, const float *pos, float *x, int n_images, int img_size, int patch_size,
                                       int in_chans, int embed_dim, int num_registers) {
    if (!images || !conv_w || !conv_b || !prefix || !pos || !x || n_images <= 0) return static_cast<int>(hipErrorInvalidValue);
    if (patch_size < 2 || patch_size % 2 || img_size < patch_size || img_size % 2 || img_size % patch_size)
        return static_cast<int>(hipErrorInvalidValue);
    if (in_chans < 1 || embed_dim < 4 || embed_dim % 4) return static_cast<int>(hipErrorInvalidValue);
    // one image is addressed with 32-bit element offsets
    if ((unsigned long long)in_chans * img_size * img_size > 0x3fffffffull) return static_cast<int>(hipErrorInvalidValue);
    const int G = img_size / patch_size;
    if ((unsigned long long)n_images * G * G > (1ull << 24)) return static_cast<int>(hipErrorInvalidValue);
    if (!embed_rows_ok(n_images, G * G, num_registers)) return static_cast<int>(hipErrorInvalidValue);
    if ((unsigned long long)in_chans * patch_size * patch_size > 0x3fffffffull) return static_cast<int>(hipErrorInvalidValue);
    if (!aligned8(images) || !aligned8(conv_w)) return static_cast<int>(hipErrorInvalidValue);
    EmbedParams p{};
    p.images = images; p.conv_w = conv_w; p.conv_b = conv_b; p.pos = pos; p.x = x;
    p.M = n_images * G * G; p.N = embed_dim; p.K = in_chans * patch_size * patch_size;
    p.patches = G * G; p.grid = G; p.patch = patch_size; p.img = img_size; p.chans = in_chans; p.prefix = 1 + num_registers;
    const dim3 grid(set_tile_grid(p, GBM, GBN));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (const int e = launch_prefix_rows(s, prefix, pos, x, n_images, G * G + 1 + num_registers, num_registers, embed_dim)) return e;
    hipLaunchKernelGGL(patch_embed_general_kernel, grid, dim3(256), 0, s, p);
    return static_cast<int>(hipGetLastError());
}

int vithip_patch_embed_f32_general(vithip_stream_t stream, const float *images, const float *conv_w, const float *conv_b,
                                   const float *cls, const float *pos, float *x, int n_images, int img_size, int patch_size,
                                   int in_chans, int embed_dim) {
    return vithip_patch_embed_f32_general_reg(stream, images, conv_w, conv_b, cls, pos, x, n_images, img_size, patch_size, in_chans,
                                              embed_dim, 0);
}

}  // extern "C"
