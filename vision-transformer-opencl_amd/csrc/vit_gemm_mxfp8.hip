// csrc/vit_gemm_mxfp8.hip -- the encoder GEMMs in MXFP8 on gfx950's scaled fp8 matrix instruction:
//   vithip_mxfp8_weights   W fp32 [N][ldw] -> the weight image the GEMM reads (once per install)
//   vithip_gemm_mxfp8      C = epilogue(q(A) . q(W)^T + bias), A bf16 in memory, quantised on chip; fp32 accumulate
// The format (include/vit_hip_kernels.h, "MXFP8"): blocks of 32 consecutive k of one row, one e8m0 exponent X + 127 per block with
// X = floor(log2(amax)) - 8 clamped to [-127, 127], elements x * 2^-X clamped to +-448 and rounded to nearest even to OCP e4m3.
//
// v_mfma_scale_f32_32x32x64_f8f6f4 (measured, profiles/r38/mxfp8.md): lane r + 32 h supplies row r, in registers 0..3 k 16 h .. 16 h + 15
// and in registers 4..7 k 32 + 16 h .. 32 + 16 h + 15 of the 64-deep step -- two 32-deep halves side by side, NOT 32 consecutive k --
// and its scale byte is applied to k 32 h .. 32 h + 31 of that row: an MX block's bytes sit in the two lanes of a row, its scale in one.
// Operand roles are swapped as in the bf16 kernels (matrix A = W rows, matrix B = activation rows):
// a lane owns ONE output row and 4 consecutive columns per register group.
//
// Design.  Workgroup = 4 waves, tile 128 x 128, K step 64; a wave owns 64 x 64: 2 x 2 accumulators, 4 matrix instructions a step.
//  * W never enters LDS.  The image is cut into blocks of (32 rows, 64 k): 64 lanes x 32 bytes, each lane's eight registers as the
//    matrix operand wants them, the 64 scale bytes behind them.  A wave's fragment is one contiguous 2 KB run, a lane's share two 16-byte loads and
//    one byte, fetched a K step ahead into registers.
//  * A is quantised on chip.  The tile's 128 rows x 2 blocks of a step are one block per thread: four 16-byte loads of bf16 a step
//    ahead, amax over the lane's own registers (integer maximum of the magnitudes: no cross-lane step), X from amax's exponent
//    field, v_cvt_scalef32_pk_fp8_bf16, then 32 bytes + the scale byte into the other LDS stage, in the layout the fragments are read
//    back in.  That work is issued behind the step's matrix instructions and runs under them.
//  * The clamp to +-448 is done in code in front of the convert (v_pk_min_u16 on the magnitudes: the limit 1.75 * 2^(X + 8) has
//    amax's exponent field and mantissa 0x60): the kernel then does not depend on how the instruction treats values past 448.
//    Blocks with X = -127 (amax < 2^-118, zero blocks included) take a plain C++ path: the scale 2^-127 is no fp32 normal, and what
//    the instruction makes of such an operand is not documented.
//  * LDS per stage: [k block 0: bytes 0..15 of 128 rows | bytes 16..31][64 B pad][k block 1: the same][scale bytes 2 x 128].
//    A fragment read is two ds_read_b128 of 32 consecutive rows (contiguous: conflict-free); 8 consecutive threads write 4 rows x
//    2 k blocks, which the pad puts on disjoint banks.  Two stages, one barrier per step.
#include "vit_device.hpp"
#include "vit_gemm_common.hpp"

namespace {

using vitgemm::f32x16;
using vitgemm::f32x2;
using vitgemm::f32x4;
using vitgemm::gelu_bf16_lockstep;
using vitgemm::quick_gelu;
using vitgemm::tile_coords;
using vitgemm::u32x4;
using vitgemm::xcd_remap;

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef short i16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

constexpr int BM = 128, BN = 128, BK = 64, THREADS = 256;
// the image: blocks of IMG_ROWS rows x BK k, rows padded to the tile
constexpr int IMG_ROWS = 32, IMG_ELEM_BYTES = 64 * 32, IMG_BLOCK_BYTES = IMG_ELEM_BYTES + 64;
static_assert(IMG_BLOCK_BYTES == VITHIP_MXFP8_BLOCK_BYTES && IMG_BLOCK_BYTES % 16 == 0, "the header states the block");
// an LDS stage of A
constexpr int LDS_HALF = BM * 16, LDS_KB = 2 * LDS_HALF + 64, LDS_SCALES = 2 * LDS_KB, LDS_STAGE = LDS_SCALES + 2 * BM;

struct Mx8Params {
    const unsigned short *A;
    const unsigned char *W;
    const float *bias;
    const float *R;
    void *C;
    int lda, ldr, ldc;
    int M, N, K;
    int tiles_m, tiles_n, group_m;
};

// |v| <= 448, finite -> OCP e4m3, round to nearest even; a zero keeps its sign
__device__ __forceinline__ unsigned e4m3_rne(float v) {
    unsigned b = __builtin_bit_cast(unsigned, v);
    const unsigned sign = (b >> 24) & 0x80u;
    b &= 0x7fffffffu;
    const float a = __builtin_bit_cast(float, b);
    if (a < 0.015625f) return sign | (unsigned)__builtin_rintf(a * 512.0f);  // subnormals: steps of 2^-9; 8 is the least normal
    b += 0x7ffffu + ((b >> 20) & 1u);
    return sign | ((b >> 20) - ((127u - 7u) << 3));
}
__device__ __forceinline__ unsigned e4m3_scaled(float x, float factor) {
    return e4m3_rne(fminf(fmaxf(x * factor, -448.0f), 448.0f));
}

// One MX block of A: 32 bf16 in 16 dwords -> 32 e4m3 bytes (lo: k 0..15, hi: k 16..31) and the e8m0 byte.
__device__ __forceinline__ void quantize_a_block(const u32x4 (&x)[4], u32x4 &lo, u32x4 &hi, unsigned &sb) {
    unsigned w[16], out[8];
#pragma unroll
    for (int i = 0; i < 16; ++i) w[i] = x[i >> 2][i & 3];
    unsigned amax = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const unsigned a = w[i] & 0x7fff7fffu;
        amax = max(amax, max(a & 0xffffu, a >> 16));
    }
    const unsigned e = amax >> 7;  // amax's exponent field: floor(log2(amax)) + 127 for a normal amax
    sb = e > 8 ? e - 8 : 0;        // X + 127, X = floor(log2(amax)) - 8 clamped at -127
    if (sb != 0) {
        const unsigned lim = ((e << 7) | 0x60u) * 0x10001u;  // 448 * 2^X, twice
        const float scale = __builtin_bit_cast(float, sb << 23);  // 2^X; the convert divides by it
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            unsigned v[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const u16x2 mag = __builtin_elementwise_min(__builtin_bit_cast(u16x2, w[2 * o + s] & 0x7fff7fffu), __builtin_bit_cast(u16x2, lim));
                v[s] = __builtin_bit_cast(unsigned, mag) | (w[2 * o + s] & 0x80008000u);
            }
            i16x2 d = {0, 0};
            d = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(d, __builtin_bit_cast(bf16x2, v[0]), scale, false);
            d = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(d, __builtin_bit_cast(bf16x2, v[1]), scale, true);
            out[o] = __builtin_bit_cast(unsigned, d);
        }
    } else {  // X = -127: |x| < 2^-118, times 2^127 exactly
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            out[o] = 0;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const unsigned u = w[2 * o + s];
                out[o] |= e4m3_scaled(__builtin_bit_cast(float, u << 16), 0x1p127f) << (16 * s);
                out[o] |= e4m3_scaled(__builtin_bit_cast(float, u & 0xffff0000u), 0x1p127f) << (16 * s + 8);
            }
        }
    }
    lo = u32x4{out[0], out[1], out[2], out[3]};
    hi = u32x4{out[4], out[5], out[6], out[7]};
}

template <int EPI>
__global__ __launch_bounds__(THREADS) void gemm_mxfp8_kernel(const Mx8Params p) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * LDS_STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5, wm = wave >> 1, wn = wave & 1;  // 2 x 2 waves of 64 x 64

    int tm, tn;
    tile_coords(xcd_remap(blockIdx.x, gridDim.x), p.tiles_m, p.tiles_n, p.group_m, tm, tn);
    const int m0 = tm * BM, n0 = tn * BN, nk = p.K / BK;

    // A: thread t stages k block t & 1 of tile row t >> 1 (a pair of lanes reads 128 contiguous bytes); rows past M are clamped
    const int srow = tid >> 1, skb = tid & 1;
    const int sm = m0 + srow < p.M ? m0 + srow : p.M - 1;
    const unsigned short *a_src = p.A + (size_t)sm * p.lda + skb * 32;
    const int st_off = skb * LDS_KB + srow * 16, st_scale = LDS_SCALES + skb * BM + srow;
    // fragments: registers 0..3 = bytes 16 h .. of k block 0, registers 4..7 = the same bytes of k block 1; the scale of k block h
    int fr_off[2], fr_scale[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = wm * 64 + i * 32 + r;
        fr_off[i] = h * LDS_HALF + row * 16;
        fr_scale[i] = LDS_SCALES + h * BM + row;
    }
    // W: the wave's two 32-row blocks of the image, K steps IMG_BLOCK_BYTES apart
    const unsigned char *w_blk[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) w_blk[j] = p.W + (size_t)((n0 + wn * 64) / IMG_ROWS + j) * nk * IMG_BLOCK_BYTES;

    u32x4 areg[4];
    auto load_a = [&](int kt) {
#pragma unroll
        for (int q = 0; q < 4; ++q) areg[q] = *reinterpret_cast<const u32x4 *>(a_src + kt * BK + q * 8);
    };
    auto load_w = [&](int kt, i32x8 (&f)[2], int (&sc)[2]) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const unsigned char *blk = w_blk[j] + (size_t)kt * IMG_BLOCK_BYTES;
            const u32x4 a = *reinterpret_cast<const u32x4 *>(blk + lane * 32), b = *reinterpret_cast<const u32x4 *>(blk + lane * 32 + 16);
            f[j] = i32x8{(int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)b[0], (int)b[1], (int)b[2], (int)b[3]};
            sc[j] = blk[IMG_ELEM_BYTES + lane];
        }
    };
    auto stage_a = [&](int buf) {
        u32x4 lo, hi;
        unsigned sb;
        quantize_a_block(areg, lo, hi, sb);
        unsigned char *base = lds + buf * LDS_STAGE;
        *reinterpret_cast<u32x4 *>(base + st_off) = lo;
        *reinterpret_cast<u32x4 *>(base + st_off + LDS_HALF) = hi;
        base[st_scale] = (unsigned char)sb;
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[j][i][v] = 0.0f;
    // bias of the lane's columns, fetched now
    f32x4 b4[2][4];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            int nb = n0 + wn * 64 + j * 32 + 8 * g + 4 * h;
            nb = nb + 4 <= p.N ? nb : p.N - 4;  // clamped address; such groups are never stored
            b4[j][g] = *reinterpret_cast<const f32x4 *>(p.bias + nb);
        }

    i32x8 wf[2], wnext[2];
    int wsc[2], wnsc[2];
    load_a(0);
    load_w(0, wf, wsc);
    stage_a(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        const bool more = kt + 1 < nk;  // workgroup-uniform
        if (more) {
            load_a(kt + 1);
            load_w(kt + 1, wnext, wnsc);
        }
        const unsigned char *base = lds + cur * LDS_STAGE;
        i32x8 af[2];
        int asc[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const u32x4 a = *reinterpret_cast<const u32x4 *>(base + fr_off[i]), b = *reinterpret_cast<const u32x4 *>(base + fr_off[i] + LDS_KB);
            af[i] = i32x8{(int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)b[0], (int)b[1], (int)b[2], (int)b[3]};
            asc[i] = base[fr_scale[i]];
        }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i)  // fp8 (e4m3) both operands; scale byte 0 of each lane's register
                acc[j][i] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(wf[j], af[i], acc[j][i], 0, 0, 0, wsc[j], 0, asc[i]);
        if (more) {
            stage_a(cur ^ 1);  // under the matrix instructions above
#pragma unroll
            for (int j = 0; j < 2; ++j) wf[j] = wnext[j], wsc[j] = wnsc[j];
        }
        __syncthreads();
    }

    // ---- epilogue: lane = row m, 4 consecutive columns per register group ------------------------------------------------------
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = m0 + wm * 64 + i * 32 + r;
        if (m >= p.M) continue;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = n0 + wn * 64 + j * 32 + 8 * g + 4 * h;
                if (n + 4 > p.N) continue;
                if constexpr (EPI == VITHIP_BF16_EPI_F32_RESIDUAL) {
                    const f32x4 res = *reinterpret_cast<const f32x4 *>(p.R + (size_t)m * p.ldr + n);
                    f32x4 y;
#pragma unroll
                    for (int q = 0; q < 4; ++q) y[q] = acc[j][i][4 * g + q] + b4[j][g][q] + res[q];
                    *reinterpret_cast<f32x4 *>(static_cast<float *>(p.C) + (size_t)m * p.ldc + n) = y;
                } else {
                    bf16x4 y;
                    if constexpr (EPI == VITHIP_BF16_EPI_BF16_GELU) {  // the bf16 kernels' GELU, operation for operation
                        f32x2 v[2];
#pragma unroll
                        for (int q = 0; q < 2; ++q)
                            v[q] = f32x2{acc[j][i][4 * g + 2 * q] + b4[j][g][2 * q], acc[j][i][4 * g + 2 * q + 1] + b4[j][g][2 * q + 1]};
                        gelu_bf16_lockstep<2>(v);
                        y = bf16x4{(__bf16)v[0].x, (__bf16)v[0].y, (__bf16)v[1].x, (__bf16)v[1].y};
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            float t = acc[j][i][4 * g + q] + b4[j][g][q];
                            if constexpr (EPI == VITHIP_BF16_EPI_BF16_QGELU) t = quick_gelu(t);
                            y[q] = (__bf16)t;
                        }
                    }
                    *reinterpret_cast<bf16x4 *>(static_cast<unsigned short *>(p.C) + (size_t)m * p.ldc + n) = y;
                }
            }
    }
}

// One thread makes one MX block of the image: row n = 32 * block + lane % 32, k = 64 * step + 32 * (lane / 32) .. + 31.  Its first 16
// bytes are registers 4 h .. 4 h + 3 of the row's lane r, its last 16 those of lane r + 32; its scale byte is lane r + 32 h's.
__global__ __launch_bounds__(64) void mxfp8_weights_kernel(const float *__restrict__ W, int ldw, int N, int nk, unsigned char *__restrict__ out) {
    const size_t blk = blockIdx.x;  // 32-row block * nk + K step
    const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
    const int nb = (int)(blk / nk), step = (int)(blk - (size_t)nb * nk), n = nb * IMG_ROWS + r;
    f32x4 x[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) x[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (n < N) {
        const float *src = W + (size_t)n * ldw + step * BK + h * 32;
#pragma unroll
        for (int q = 0; q < 8; ++q) x[q] = *reinterpret_cast<const f32x4 *>(src + 4 * q);
    }
    unsigned amax = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float v = x[q][c];  // (a bit cast of the vector's element itself reads element 0)
            amax = max(amax, __builtin_bit_cast(unsigned, v) & 0x7fffffffu);
        }
    const unsigned e = amax >> 23, sb = e > 8 ? e - 8 : 0;
    const float factor = __builtin_bit_cast(float, (254u - sb) << 23);  // 2^-X
    unsigned o[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        o[q] = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) o[q] |= e4m3_scaled(x[q][c], factor) << (8 * c);
    }
    unsigned char *dst = out + blk * IMG_BLOCK_BYTES;
    *reinterpret_cast<u32x4 *>(dst + r * 32 + h * 16) = u32x4{o[0], o[1], o[2], o[3]};
    *reinterpret_cast<u32x4 *>(dst + (32 + r) * 32 + h * 16) = u32x4{o[4], o[5], o[6], o[7]};
    dst[IMG_ELEM_BYTES + lane] = (unsigned char)sb;
}

inline bool aligned16(const void *ptr) { return (reinterpret_cast<size_t>(ptr) & 15) == 0; }

}  // namespace

extern "C" {

size_t vithip_mxfp8_image_bytes(int N, int K) {
    if (N <= 0 || K <= 0 || K % BK) return 0;
    return (size_t)((N + BN - 1) / BN) * (BN / IMG_ROWS) * (size_t)(K / BK) * IMG_BLOCK_BYTES;
}

size_t vithip_mxfp8_image_row_offset(int n, int K) {
    if (n < 0 || n % IMG_ROWS || K <= 0 || K % BK) return 0;
    return (size_t)(n / IMG_ROWS) * (size_t)(K / BK) * IMG_BLOCK_BYTES;
}

int vithip_mxfp8_weights(vithip_stream_t stream, const float *W, int ldw, int N, int K, void *image) {
    if (!W || !image || N <= 0 || K <= 0 || K % BK || ldw < K || ldw % 4) return static_cast<int>(hipErrorInvalidValue);
    if (!aligned16(W) || !aligned16(image)) return static_cast<int>(hipErrorInvalidValue);
    const size_t blocks = vithip_mxfp8_image_bytes(N, K) / IMG_BLOCK_BYTES;
    if (blocks >= 0x7fffffffull) return static_cast<int>(hipErrorInvalidValue);
    hipLaunchKernelGGL(mxfp8_weights_kernel, dim3((unsigned)blocks), dim3(64), 0, static_cast<hipStream_t>(stream), W, ldw, N, K / BK,
                       static_cast<unsigned char *>(image));
    return static_cast<int>(hipGetLastError());
}

int vithip_gemm_mxfp8(vithip_stream_t stream, const vithip_gemm_mxfp8_args *a) {
    if (!a || !a->A || !a->W || !a->bias || !a->C) return static_cast<int>(hipErrorInvalidValue);
    if (a->M <= 0 || a->N <= 0 || a->K <= 0 || a->K % BK || a->N % 8) return static_cast<int>(hipErrorInvalidValue);
    if (a->lda % 8 || a->lda < a->K || a->ldc < a->N || a->ldc % 4) return static_cast<int>(hipErrorInvalidValue);
    if (!aligned16(a->A) || !aligned16(a->W) || !aligned16(a->bias) || !aligned16(a->C)) return static_cast<int>(hipErrorInvalidValue);
    if (a->epilogue == VITHIP_BF16_EPI_F32_RESIDUAL && (!a->residual || a->ldr < a->N || a->ldr % 4 || !aligned16(a->residual)))
        return static_cast<int>(hipErrorInvalidValue);
    Mx8Params p{};
    p.A = a->A; p.W = static_cast<const unsigned char *>(a->W); p.bias = a->bias; p.R = a->residual; p.C = a->C;
    p.lda = a->lda; p.ldr = a->ldr; p.ldc = a->ldc;
    p.M = a->M; p.N = a->N; p.K = a->K;
    const int total = vitgemm::set_tile_grid(p, BM, BN);
    p.group_m = 8;
    return vitgemm::with_epilogue(vitgemm::Bf16Epilogues{}, a->epilogue, [&](auto epi) {
        hipLaunchKernelGGL(gemm_mxfp8_kernel<decltype(epi)::value>, dim3(total), dim3(THREADS), 0, static_cast<hipStream_t>(stream), p);
        return static_cast<int>(hipGetLastError());
    });
}

}  // extern "C"
