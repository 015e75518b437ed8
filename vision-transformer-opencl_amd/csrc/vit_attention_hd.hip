// csrc/vit_attention_hd.hip -- attention for head dims other than 64: every multiple of 8 from 72 to 128 (ViT-H/14: 80, OpenCLIP
// ViT-g-14 / EVA-g: 88, SigLIP2 giant: 96, OpenCLIP ViT-bigG-14: 104).  head_dim 64 is not computed here: each entry hands it to the
// entry it generalises (vit_attention.hip, vit_cls_attention.hip), whose kernels are untouched.
//
// Reference semantics: ViT_seq.c:156-215 with 64 replaced by head_dim (scores / sqrtf(head_dim), row softmax with max subtraction,
// P.V).  qkv [n*T][3*heads*hd], columns [Q | K | V], head h = columns hd*h.. of each; out [n*T][heads*hd].
//
// One kernel for every sequence length.  K and V of a head do not fit the LDS at head_dim 128 in fp32, so there is
// no resident variant: a workgroup of 4 waves takes (image, head, block of 128 query rows), a wave owns 32 query rows with their
// online-softmax state (running maximum, running sum, O^T accumulators) and their Q fragments in registers, and K / V stream
// through the LDS in chunks of 64 (bf16) or 32 (fp32) keys, single-buffered between two barriers; three or four workgroups per CU
// cover each other's staging.  The MFMA orientation is the one of attention_bf16_kernel: S^T = K . Q^T puts a query on a lane and its 32
// keys into the 16 registers of the two half-waves, so O^T += V^T . P^T takes P from the accumulator as its B operand with no lane
// movement; V is transposed while it is staged ([d][key] in LDS), so its A fragments are contiguous reads.
//
//   bf16: v_mfma_f32_32x32x16_bf16 for both products, fp32 scores and softmax, the output rounded to bf16 once.  P multiplies V in
//         two bf16 pieces, bf16(p) and bf16(p - bf16(p)) (accurate to 2^-17): with one piece the rounding of P alone passes the 1e-3
//         of the bf16 bar on short sequences (tests/test_gpu_attention_hd.py::test_bf16_matches_the_oracle).  The contraction over d runs in steps of 16: for head_dim 72, 88, 104, 120 the last step's upper 8 columns are ZEROS on both
//         sides -- the K image's columns [hd, hd16) are written as zeros by the staging pass and a lane's Q fragment of that piece is
//         a zero register, never a load: nothing reads behind column hd of a head's slice.
//   fp32: v_mfma_f32_32x32x2_f32.  A k-step takes d = 8g + i from the lower half-wave and d = 8g + 4 + i from the upper one
//         (i = 0..3 of one 16-byte read): a permutation of the sum over d that both operands share; hd % 8 == 0 needs no padding.
//
// Keys past the last token are zeros in both LDS images and their scores are set to -inf: they weigh exactly 0.  Rows of the V^T
// image from hd up to the next multiple of 32 are never written and never stored: an A-operand row reaches its own output row only.
// A workgroup reads one image's rows only (query rows past q_rows are clamped to the image's row q_rows - 1 and dropped at the store),
// so a non-finite value stays in its image and an image's bits depend on neither the batch nor its place in it.  No atomics.
#include <hip/hip_runtime.h>

#include <math.h>

#include <type_traits>

#include "vit_hip_kernels.h"
#include "vit_row.hpp"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short bf16_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// A workgroup is 4 waves of 32 query rows.  What counts is how many workgroups a CU holds to cover each other's staging and
// barriers (measured at 257 tokens, batch 256, against the head_dim 64 kernels at equal MACs: profiles/r20/head_dim.md): with 8 waves
// and whatever registers the allocator liked, a workgroup was alone on its CU from head_dim 104 (bf16) and for every fp32 kernel,
// and took 1.2 - 2.0 x the 64 launch; 4 waves with the allocation capped for four (bf16 up to head_dim 96: three O^T tiles, 128
// VGPRs) or three workgroups per CU (168 VGPRs) take 0.85 - 1.35 x.
constexpr int HD_WAVES = 4, HD_THREADS = HD_WAVES * 64;
constexpr int HD_QROWS = HD_WAVES * 32;  // query rows per workgroup

template <int HD, bool BF16>
struct Geo {
    typedef typename std::conditional<BF16, bf16_t, float>::type elem;
    static constexpr int VEC = BF16 ? 8 : 4;              // elements of a 16-byte piece
    static constexpr int KC = BF16 ? 64 : 32;             // keys per chunk
    static constexpr int KT = KC / 32;                    // 32-key tiles per chunk
    static constexpr int DT = (HD + 31) / 32;             // 32-row tiles of O^T
    static constexpr int HDK = BF16 ? (HD + 15) / 16 * 16 : HD;  // contraction length of the scores, padded to the instruction's K
    static constexpr int KROW = HDK + (BF16 ? 8 : 4);     // K image: elements per key row (an odd number of 16-byte slots)
    static constexpr int VROW = KC + 4;                   // V^T image: elements per d row (bf16: 34 dwords, fp32: 9 slots)
    static constexpr int K_ELEMS = KC * KROW, V_ELEMS = DT * 32 * VROW;
    static constexpr int MIN_WAVES = BF16 && HD <= 96 ? 4 : 3;  // waves per SIMD the register allocation must leave room for
};

template <int HD, bool BF16, bool QS>
__global__ __launch_bounds__(HD_THREADS, (Geo<HD, BF16>::MIN_WAVES)) void attention_hd_kernel(
    const typename Geo<HD, BF16>::elem *__restrict__ qkv, typename Geo<HD, BF16>::elem *__restrict__ out, int tokens, int heads, int q_rows,
    int qblocks, float scale) {
    typedef Geo<HD, BF16> G;
    typedef typename G::elem elem;
    constexpr int VEC = G::VEC, KC = G::KC, KT = G::KT, DT = G::DT, KROW = G::KROW, VROW = G::VROW;
    __shared__ __attribute__((aligned(16))) elem Ks[G::K_ELEMS];
    __shared__ __attribute__((aligned(16))) elem Vt[G::V_ELEMS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int image = blockIdx.x / qblocks, qblock = blockIdx.x - image * qblocks, head = blockIdx.y;
    const size_t D = (size_t)heads * HD, ld = 3 * D;
    const elem *rows = qkv + (size_t)image * tokens * ld + (size_t)head * HD;  // the image's token rows, this head's Q columns
    const elem *krows = rows + D, *vrows = rows + 2 * D;
    const int qrow0 = qblock * HD_QROWS + wave * 32;
    const bool active = qrow0 < q_rows;  // wave-uniform: this wave owns query rows

    // ---- Q fragments of this wave's 32 rows, for all of the sequence
    constexpr int NQ = BF16 ? G::HDK / 16 : HD / 8;
    typename std::conditional<BF16, bf16x8, f32x4>::type qf[NQ];
    {
        int qrow = qrow0 + r;
        qrow = qrow < q_rows ? qrow : q_rows - 1;  // a row of this image; dropped at the store
        const elem *qp = rows + (size_t)qrow * ld;
#pragma unroll
        for (int ks = 0; ks < NQ; ++ks) {
            if constexpr (BF16) {
                const int d0 = 16 * ks + 8 * h;
                u32x4 w = {0u, 0u, 0u, 0u};          // the padded tail of the contraction: zeros, not a load
                if (d0 < HD && active) w = *reinterpret_cast<const u32x4 *>(qp + d0);
                qf[ks] = __builtin_bit_cast(bf16x8, w);
            } else {
                f32x4 w = {0.0f, 0.0f, 0.0f, 0.0f};
                if (active) w = *reinterpret_cast<const f32x4 *>(qp + 8 * ks + 4 * h);
                qf[ks] = w;
            }
        }
    }

    f32x16 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int v = 0; v < 16; ++v) o[dt][v] = 0.0f;
    float m_run = -INFINITY, l_run = 0.0f;  // per query (lane & 31); l_run: this half-wave's keys

    for (int key0 = 0; key0 < tokens; key0 += KC) {
        // ---- stage the chunk: K as it lies (zeros behind hd and behind the last token), V transposed (zeros behind the last token)
        constexpr int KP = G::HDK / VEC;  // 16-byte pieces of a K image row
        for (int i = tid; i < KC * KP; i += HD_THREADS) {
            const int row = i / KP, c = i - row * KP, key = key0 + row;
            u32x4 w = {0u, 0u, 0u, 0u};
            if (key < tokens && c * VEC < HD) w = *reinterpret_cast<const u32x4 *>(krows + (size_t)key * ld + c * VEC);
            *reinterpret_cast<u32x4 *>(Ks + row * KROW + c * VEC) = w;
        }
        constexpr int VP = HD / VEC;      // 16-byte pieces of a V row
        if constexpr (BF16) {  // the same 8 d of two adjacent keys per thread: 8 dword writes, adjacent lanes on adjacent banks
            for (int i = tid; i < (KC / 2) * VP; i += HD_THREADS) {
                const int c = i / (KC / 2), row = 2 * (i - c * (KC / 2)), key = key0 + row;
                u32x4 a = {0u, 0u, 0u, 0u}, b = {0u, 0u, 0u, 0u};
                if (key < tokens) a = *reinterpret_cast<const u32x4 *>(vrows + (size_t)key * ld + c * VEC);
                if (key + 1 < tokens) b = *reinterpret_cast<const u32x4 *>(vrows + (size_t)(key + 1) * ld + c * VEC);
#pragma unroll
                for (int j = 0; j < 4; ++j) {  // elements 2j, 2j + 1 of the piece: key `row` in the low half, key row + 1 in the high half
                    *reinterpret_cast<unsigned *>(Vt + (c * 8 + 2 * j) * VROW + row) = (a[j] & 0xffffu) | (b[j] << 16);
                    *reinterpret_cast<unsigned *>(Vt + (c * 8 + 2 * j + 1) * VROW + row) = (a[j] >> 16) | (b[j] & 0xffff0000u);
                }
            }
        } else {
            for (int i = tid; i < KC * VP; i += HD_THREADS) {
                const int c = i / KC, row = i - c * KC, key = key0 + row;
                u32x4 w = {0u, 0u, 0u, 0u};
                if (key < tokens) w = *reinterpret_cast<const u32x4 *>(vrows + (size_t)key * ld + c * VEC);
#pragma unroll
                for (int j = 0; j < 4; ++j) Vt[(c * 4 + j) * VROW + row] = __uint_as_float(w[j]);
            }
        }
        __syncthreads();

        if (active) {
#pragma unroll
            for (int t = 0; t < KT; ++t) {
                const int tile0 = key0 + 32 * t;
                if (tile0 >= tokens) break;  // wave-uniform: a tile of zeros
                // ---- S^T = K . Q^T: key = (v & 3) + 8 (v >> 2) + 4 h of the tile in register v, query r on the lane
                f32x16 s;
#pragma unroll
                for (int v = 0; v < 16; ++v) s[v] = 0.0f;
                const elem *kp = Ks + (32 * t + r) * KROW;
#pragma unroll
                for (int ks = 0; ks < NQ; ++ks) {
                    if constexpr (BF16) {
                        const bf16x8 kf = *reinterpret_cast<const bf16x8 *>(kp + 16 * ks + 8 * h);
                        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[ks], s, 0, 0, 0);
                    } else {
                        const f32x4 kf = *reinterpret_cast<const f32x4 *>(kp + 8 * ks + 4 * h);
#pragma unroll
                        for (int i = 0; i < 4; ++i) s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[i], qf[ks][i], s, 0, 0, 0);
                    }
                }
                if (tile0 + 32 > tokens) {  // wave-uniform: the sequence's last tile
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        const int key = tile0 + (v & 3) + 8 * (v >> 2) + 4 * h;
                        s[v] = key < tokens ? s[v] : -INFINITY;
                    }
                }
                // ---- online softmax: p = 2^(scale s - scale m), m the running maximum of the raw scores
                float cmax = s[0];
#pragma unroll
                for (int v = 1; v < 16; ++v) cmax = fmaxf(cmax, s[v]);
                cmax = fmaxf(cmax, __shfl_xor(cmax, 32));
                // The running maximum is a reference, not a bound (as in vit_attention_stream.hip): it moves only when a row's scores
                // outgrow it by more than kDefer in the exponent.  P then reaches 2^kDefer instead of 1 -- the same relative precision
                // in bf16 and in the fp32 sums -- and the rescale of O below runs a few times per sequence, not in every tile.
                constexpr float kDefer = 8.0f;
                const float m_old = m_run;
                const float m_new = (cmax - m_old) * scale > kDefer ? cmax : m_old;  // first tile: m_old = -inf -> cmax
                const float mneg = -m_new * scale;
                m_run = m_new;
                float sum = 0.0f;
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    s[v] = __builtin_amdgcn_exp2f(QS ? s[v] + mneg : fmaf(s[v], scale, mneg));  // exp2(-inf) = 0: masked keys
                    sum += s[v];
                }
                if (__any(m_new != m_old)) {  // wave-uniform
                    const float alpha = __builtin_amdgcn_exp2f((m_old - m_new) * scale);  // first tile: exp2(-inf) = 0; unmoved rows: 1
                    l_run *= alpha;
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                        for (int v = 0; v < 16; ++v) o[dt][v] *= alpha;
                }
                l_run += sum;
                // ---- O^T += V^T . P^T: d = 32 dt + r on the A operand's lane, the keys of register v as above
                if constexpr (BF16) {
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2) {
                        // P goes to the matrix pipe as bf16(p) and, in a second product, as bf16(p - bf16(p)): the rounding of P
                        // (relative 2^-9 per weight) does not average out over the few keys of a short sequence -- at 33 and 65
                        // keys it alone can pass 1e-3 of an output -- and with the remainder it is 2^-17.
                        bf16x8 pf, pl;
#pragma unroll
                        for (int j = 0; j < 8; ++j) {
                            pf[j] = (__bf16)s[8 * s2 + j];
                            pl[j] = (__bf16)(s[8 * s2 + j] - (float)pf[j]);
                        }
#pragma unroll
                        for (int dt = 0; dt < DT; ++dt) {
                            const bf16_t *vp = Vt + (32 * dt + r) * VROW + 32 * t + 16 * s2 + 4 * h;
                            const u32x2 lo = *reinterpret_cast<const u32x2 *>(vp), hi = *reinterpret_cast<const u32x2 *>(vp + 8);
                            const u32x4 both = {lo[0], lo[1], hi[0], hi[1]};
                            o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, both), pl, o[dt], 0, 0, 0);
                            o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, both), pf, o[dt], 0, 0, 0);
                        }
                    }
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
#pragma unroll
                        for (int dt = 0; dt < DT; ++dt) {
                            const f32x4 vf = *reinterpret_cast<const f32x4 *>(Vt + (32 * dt + r) * VROW + 32 * t + 8 * q + 4 * h);
#pragma unroll
                            for (int i = 0; i < 4; ++i) o[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vf[i], s[4 * q + i], o[dt], 0, 0, 0);
                        }
                }
            }
        }
        __syncthreads();  // everybody is done with the chunk
    }

    // ---- normalise and store: a lane holds d = 32 dt + 8 q + 4 h + (0..3) of its query row in registers 4 q .. 4 q + 3
    const int qrow = qrow0 + r;
    if (active && qrow < q_rows) {
        const float inv = 1.0f / (l_run + __shfl_xor(l_run, 32));
        elem *dst = out + ((size_t)image * tokens + qrow) * D + (size_t)head * HD;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int d0 = 32 * dt + 8 * q + 4 * h;
                if (d0 < HD) {
                    if constexpr (BF16) {
                        bf16x4 w;
#pragma unroll
                        for (int i = 0; i < 4; ++i) w[i] = (__bf16)(o[dt][4 * q + i] * inv);
                        *reinterpret_cast<u32x2 *>(dst + d0) = __builtin_bit_cast(u32x2, w);
                    } else {
                        const f32x4 w = {o[dt][4 * q] * inv, o[dt][4 * q + 1] * inv, o[dt][4 * q + 2] * inv, o[dt][4 * q + 3] * inv};
                        *reinterpret_cast<f32x4 *>(dst + d0) = w;
                    }
                }
            }
    }
}

bool hd_accepted(int head_dim) { return head_dim == 64 || (head_dim >= 72 && head_dim <= 128 && head_dim % 8 == 0); }

template <int HD, bool BF16, bool QS>
int launch_hd(hipStream_t s, const typename Geo<HD, BF16>::elem *qkv, typename Geo<HD, BF16>::elem *out, int n_images, int tokens,
              int heads, int q_rows, float scale) {
    const int qblocks = (q_rows + HD_QROWS - 1) / HD_QROWS;
    hipLaunchKernelGGL((attention_hd_kernel<HD, BF16, QS>), dim3((unsigned)(n_images * qblocks), (unsigned)heads), dim3(HD_THREADS), 0, s,
                       qkv, out, tokens, heads, q_rows, qblocks, scale);
    return static_cast<int>(hipGetLastError());
}

template <bool BF16, bool QS>
int dispatch_hd(hipStream_t s, const typename Geo<128, BF16>::elem *qkv, typename Geo<128, BF16>::elem *out, int n_images, int tokens,
                int heads, int head_dim, int q_rows) {
    if (!qkv || !out || n_images <= 0 || tokens <= 0 || heads <= 0 || heads > 65535 || q_rows <= 0 || q_rows > tokens)
        return static_cast<int>(hipErrorInvalidValue);
    if ((reinterpret_cast<size_t>(qkv) & 15) || (reinterpret_cast<size_t>(out) & 15)) return static_cast<int>(hipErrorInvalidValue);
    const long long blocks = (long long)n_images * ((q_rows + HD_QROWS - 1) / HD_QROWS);
    if (blocks > 0x7fffffffLL) return static_cast<int>(hipErrorInvalidValue);
    const float scale = QS ? 1.0f : vithip_qscale(head_dim);
    switch (head_dim) {
#define HD_CASE(N) case N: return launch_hd<N, BF16, QS>(s, qkv, out, n_images, tokens, heads, q_rows, scale);
        HD_CASE(72) HD_CASE(80) HD_CASE(88) HD_CASE(96) HD_CASE(104) HD_CASE(112) HD_CASE(120) HD_CASE(128)
#undef HD_CASE
        default: return static_cast<int>(hipErrorInvalidValue);
    }
}

// ---- the class token's attention row (the contract of vit_cls_attention.hip with 64 replaced by head_dim) -----------------------
//
// The same three passes: scores of all keys (a group of lanes per key), sum of the weights, the stored row.  A group is 16 lanes for
// both element types and a lane takes the 16-byte pieces sub, sub + 16 of a head's slice of a row (fp32: 18..32 pieces, two rounds;
// bf16: 9..16 pieces, one round); a piece past head_dim is not loaded and adds nothing.  Products in element order, pieces in
// order, then the butterfly: score() is one function of (image, head, key) and gives the same bits wherever it is called.
using vit_row::wave_max;
using vit_row::wave_sum;

constexpr int CA_THREADS = 256, CA_WAVES = CA_THREADS / 64, CA_CACHE = 4096, CA_GROUP = 16, CA_KEYS = CA_THREADS / CA_GROUP;
constexpr int CA_AHEAD = 2;  // keys a group loads ahead in pass 1

template <bool BF16> struct Piece;
template <> struct Piece<false> {
    static constexpr int VEC = 4, ROUNDS = 2;
    typedef float elem;
    static __device__ __forceinline__ void load(const float *p, float (&v)[4]) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(p);
        v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
    }
};
template <> struct Piece<true> {
    static constexpr int VEC = 8, ROUNDS = 1;
    typedef unsigned short elem;
    static __device__ __forceinline__ void load(const unsigned short *p, float (&v)[8]) {
        const u32x4 a = *reinterpret_cast<const u32x4 *>(p);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[2 * j] = __uint_as_float(a[j] << 16);
            v[2 * j + 1] = __uint_as_float(a[j] & 0xffff0000u);
        }
    }
};

template <bool MAX>
__device__ __forceinline__ float block_reduce(float v, float *red) {
    v = MAX ? wave_max(v) : wave_sum(v);
    __syncthreads();  // red may still be read from the reduction before
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int w = 1; w < CA_WAVES; ++w) r = MAX ? fmaxf(r, red[w]) : r + red[w];
    return r;
}

template <bool BF16>
__global__ __launch_bounds__(CA_THREADS) void cls_attention_hd_kernel(const typename Piece<BF16>::elem *__restrict__ qkv, size_t row_stride,
                                                                       float *__restrict__ out, size_t ld_out, int tokens, int heads,
                                                                       int head_dim, int head_mean, int q_scaled, float scale) {
    typedef Piece<BF16> E;
    constexpr int VEC = E::VEC, ROUNDS = E::ROUNDS;
    __shared__ float cache[CA_CACHE];
    __shared__ float red[CA_WAVES];

    const int tid = threadIdx.x, sub = tid % CA_GROUP, grp = tid / CA_GROUP;
    const int image = head_mean ? blockIdx.x : blockIdx.x / heads;
    const int h_lo = head_mean ? 0 : blockIdx.x - image * heads, h_hi = head_mean ? heads : h_lo + 1;
    const size_t D = (size_t)heads * head_dim;
    const typename E::elem *rows = qkv + (size_t)image * tokens * row_stride;  // the image's token rows: [Q | K | V]
    const int cached = tokens < CA_CACHE ? tokens : CA_CACHE;
    bool mine[ROUNDS];  // this lane has a piece in round i
#pragma unroll
    for (int i = 0; i < ROUNDS; ++i) mine[i] = (sub + CA_GROUP * i) * VEC < head_dim;

    for (int h = h_lo; h < h_hi; ++h) {
        float q[ROUNDS][VEC];
#pragma unroll
        for (int i = 0; i < ROUNDS; ++i) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) q[i][j] = 0.0f;
            if (mine[i]) E::load(rows + (size_t)h * head_dim + (sub + CA_GROUP * i) * VEC, q[i]);
        }
        const typename E::elem *kh = rows + D + (size_t)h * head_dim + sub * VEC;  // this lane's first 16 bytes of key 0

        auto load_key = [&](int t, float (&k)[ROUNDS][VEC]) {
#pragma unroll
            for (int i = 0; i < ROUNDS; ++i) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) k[i][j] = 0.0f;
                if (mine[i]) E::load(kh + (size_t)t * row_stride + CA_GROUP * i * VEC, k[i]);
            }
        };
        // the score of a key whose pieces are in k, in every lane of the group
        auto dot = [&](const float (&k)[ROUNDS][VEC]) -> float {
            float a = q[0][0] * k[0][0];
#pragma unroll
            for (int i = 0; i < ROUNDS; ++i)
#pragma unroll
                for (int j = (i == 0 ? 1 : 0); j < VEC; ++j) a = fmaf(q[i][j], k[i][j], a);
#pragma unroll
            for (int off = CA_GROUP / 2; off > 0; off >>= 1) a += __shfl_xor(a, off);
            return a * scale;
        };
        auto score = [&](int t) -> float {
            float k[ROUNDS][VEC];
            load_key(t, k);
            return dot(k);
        };
        auto weight = [&](float s, float m) -> float { return q_scaled ? exp2f(s - m) : expf(s - m); };

        __syncthreads();  // the cache of the head before has been read
        float m = -INFINITY;
        for (int t0 = grp; t0 < tokens; t0 += CA_AHEAD * CA_KEYS) {
            float k[CA_AHEAD][ROUNDS][VEC];
#pragma unroll
            for (int u = 0; u < CA_AHEAD; ++u) {
                const int t = t0 + u * CA_KEYS;
                load_key(t < tokens ? t : tokens - 1, k[u]);  // clamped: always a row of this image
            }
#pragma unroll
            for (int u = 0; u < CA_AHEAD; ++u) {
                const int t = t0 + u * CA_KEYS;
                const float s = dot(k[u]);
                if (t < tokens) {
                    if (sub == 0 && t < CA_CACHE) cache[t] = s;
                    m = fmaxf(m, s);
                }
            }
        }
        m = block_reduce<true>(m, red);  // its barriers also publish the cache

        float l = 0.0f;
        for (int t = tid; t < cached; t += CA_THREADS) l += weight(cache[t], m);
        for (int t = CA_CACHE + grp; t < tokens; t += CA_KEYS) {  // past the cache: the group recomputes, its first lane counts
            const float w = weight(score(t), m);
            if (sub == 0) l += w;
        }
        l = block_reduce<false>(l, red);

        float *dst = out + (size_t)image * ld_out + (head_mean ? 0 : (size_t)h * tokens);
        const int first = h == 0, last = h == heads - 1;
        auto emit = [&](int t, float p) {  // the owner of dst[t] is the same thread for every head
            if (head_mean) {
                if (!first) p = dst[t] + p;
                if (last) p = p / (float)heads;
            }
            dst[t] = p;
        };
        for (int t = tid; t < cached; t += CA_THREADS) emit(t, weight(cache[t], m) / l);
        for (int t = CA_CACHE + grp; t < tokens; t += CA_KEYS) {
            const float p = weight(score(t), m) / l;
            if (sub == 0) emit(t, p);
        }
    }
}

template <bool BF16>
int launch_cls_hd(vithip_stream_t stream, const typename Piece<BF16>::elem *qkv, size_t q_row_stride, float *out, size_t ld_out,
                  int n_images, int tokens, int heads, int head_dim, int head_mean, int q_scaled) {
    if (!qkv || !out || n_images <= 0 || tokens <= 0 || heads <= 0 || (head_mean != 0 && head_mean != 1) || (q_scaled != 0 && q_scaled != 1))
        return static_cast<int>(hipErrorInvalidValue);
    const size_t width = 3 * (size_t)heads * head_dim, row = head_mean ? (size_t)tokens : (size_t)heads * tokens;
    if (q_row_stride < width || q_row_stride % Piece<BF16>::VEC || ld_out < row) return static_cast<int>(hipErrorInvalidValue);
    if ((reinterpret_cast<size_t>(qkv) & 15) || (reinterpret_cast<size_t>(out) & 3)) return static_cast<int>(hipErrorInvalidValue);
    const size_t blocks = (size_t)n_images * (head_mean ? 1 : (size_t)heads);
    if (blocks > (size_t)0x7fffffff) return static_cast<int>(hipErrorInvalidValue);
    const float scale = q_scaled ? 1.0f : 1.0f / sqrtf((float)head_dim);
    hipLaunchKernelGGL(cls_attention_hd_kernel<BF16>, dim3((unsigned)blocks), dim3(CA_THREADS), 0, static_cast<hipStream_t>(stream), qkv,
                       q_row_stride, out, ld_out, tokens, heads, head_dim, head_mean, q_scaled, scale);
    return static_cast<int>(hipGetLastError());
}

}  // namespace

extern "C" {

float vithip_qscale(int head_dim) {
    if (!hd_accepted(head_dim)) return 0.0f;
    return (float)((1.0 / sqrt((double)head_dim)) * 1.4426950408889634074);  // log2(e)
}

int vithip_attention_f32_hd(vithip_stream_t stream, const float *qkv, float *out, int n_images, int tokens, int heads, int head_dim,
                            int q_rows) {
    if (!hd_accepted(head_dim)) return static_cast<int>(hipErrorInvalidValue);
    if (head_dim == 64) {
        if (q_rows == tokens) return vithip_attention_f32(stream, qkv, out, n_images, tokens, heads);
        return vithip_attention_f32_rows(stream, qkv, out, n_images, tokens, heads, q_rows);
    }
    return dispatch_hd<false, false>(static_cast<hipStream_t>(stream), qkv, out, n_images, tokens, heads, head_dim, q_rows);
}

int vithip_attention_bf16io_hd(vithip_stream_t stream, const unsigned short *qkv, unsigned short *out, int n_images, int tokens,
                               int heads, int head_dim, int q_rows, int q_scaled) {
    if (!hd_accepted(head_dim) || (q_scaled != 0 && q_scaled != 1)) return static_cast<int>(hipErrorInvalidValue);
    if (head_dim == 64) {
        if (q_scaled) return vithip_attention_bf16io_qscaled(stream, qkv, out, n_images, tokens, heads, q_rows);
        if (q_rows == tokens) return vithip_attention_bf16io(stream, qkv, out, n_images, tokens, heads);
        return vithip_attention_bf16io_rows(stream, qkv, out, n_images, tokens, heads, q_rows);
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    return q_scaled ? dispatch_hd<true, true>(s, qkv, out, n_images, tokens, heads, head_dim, q_rows)
                    : dispatch_hd<true, false>(s, qkv, out, n_images, tokens, heads, head_dim, q_rows);
}

int vithip_cls_attention_f32_hd(vithip_stream_t stream, const float *qkv, size_t q_row_stride, float *out, size_t ld_out, int n_images,
                                int tokens, int heads, int head_dim, int head_mean) {
    if (!hd_accepted(head_dim)) return static_cast<int>(hipErrorInvalidValue);
    if (head_dim == 64) return vithip_cls_attention_f32(stream, qkv, q_row_stride, out, ld_out, n_images, tokens, heads, head_mean);
    return launch_cls_hd<false>(stream, qkv, q_row_stride, out, ld_out, n_images, tokens, heads, head_dim, head_mean, 0);
}

int vithip_cls_attention_bf16_hd(vithip_stream_t stream, const unsigned short *qkv, size_t q_row_stride, float *out, size_t ld_out,
                                 int n_images, int tokens, int heads, int head_dim, int head_mean, int q_scaled) {
    if (!hd_accepted(head_dim)) return static_cast<int>(hipErrorInvalidValue);
    if (head_dim == 64)
        return vithip_cls_attention_bf16(stream, qkv, q_row_stride, out, ld_out, n_images, tokens, heads, head_mean, q_scaled);
    return launch_cls_hd<true>(stream, qkv, q_row_stride, out, ld_out, n_images, tokens, heads, head_dim, head_mean, q_scaled);
}

}  // extern "C"
