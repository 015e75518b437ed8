// csrc/vit_attention_hd.hip -- attention for head dims other than 64: every multiple of 8 from 72 to 128 (ViT-H/14: 80, OpenCLIP
// ViT-g-14 / EVA-g: 88, SigLIP2 giant: 96, OpenCLIP ViT-bigG-14: 104).  Of head_dim 64 only the split mode is computed here (fp32 on
// the bf16 matrix pipe: attention_split_kernel, below the streaming kernel whose skeleton it shares).  The entries and what sends them
// here are in vit_attention.hip (routes 7 and 8 of the table at its head).  The class token's row at these head dims: vit_cls_attention.hip.
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

#include "vit_attention.hpp"
#include "vit_hip_kernels.h"
#include "vit_split3.hpp"

namespace {

using namespace vitattn;
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

// ---- fp32 in and out at head_dim 64 on the bf16 matrix pipe: the three-piece split (route 8 of vit_attention.hip) -------
// The skeleton of the bf16 mode above -- the same chunks of 64 keys, the same K rows and V^T rows (Geo<64, true>), the same online
// softmax -- with every fp32 operand in three bf16 pieces (vit_split3.hpp: hi, mid, lo, each rounded to nearest even) and both
// products as the six piece products of rank <= 2, small terms first in the GEMM's order, on one accumulator:
//   K, V  split while a chunk is staged: three LDS planes of each (3 x 9 KB + 3 x 8.5 KB);
//   Q     split once, into registers (3 x 4 bf16x8 per lane);
//   P     split per 16 keys after the v_exp_f32: 0 <= p <= 2^kDefer, so hi + mid + lo == p exactly.
// The contraction over d runs in four steps of 16 and a step adds its six terms before the next one starts, as a K step of the split
// GEMM does; O^T takes the six terms of 16 keys at a time.  A group of 16 keys past the last token is skipped (its P is 0).
// Keys past the last token are zeros in all planes and their scores are -inf; a workgroup reads one image's rows only; no atomics:
// a row's bits depend on neither the batch, nor the image's place in it, nor q_rows.
// Measured at batch 256, 197 tokens (profiles/r23): 4 waves with three workgroups per CU 0.28 ms per launch; 8 waves (one staging pass
// per head, -DATT_SPLIT_WAVES=8) 0.31 ms, alone on their CU at 165 VGPRs, and they spill when capped at 128 for two workgroups.
#ifndef ATT_SPLIT_WAVES
#define ATT_SPLIT_WAVES 4  // waves (32 query rows each) per workgroup
#endif
#ifndef ATT_SPLIT_MINW
#define ATT_SPLIT_MINW 3   // waves per SIMD the register allocation leaves room for: 3 workgroups of 4 waves per CU (3 x 52.5 KB of LDS)
#endif
constexpr int SP_WAVES = ATT_SPLIT_WAVES, SP_THREADS = SP_WAVES * 64, SP_QROWS = SP_WAVES * 32;

__global__ __launch_bounds__(SP_THREADS, ATT_SPLIT_MINW) void attention_split_kernel(const float *__restrict__ qkv, float *__restrict__ out,
                                                                                    int tokens, int heads, int q_rows, int qblocks) {
    using vitsplit::SPLIT_TERM_A;
    using vitsplit::SPLIT_TERM_W;
    using vitsplit::split3_piece8;
    typedef Geo<64, true> G;
    constexpr int HD = 64, KC = G::KC, KT = G::KT, DT = G::DT, KROW = G::KROW, VROW = G::VROW, NQ = HD / 16;
    __shared__ __attribute__((aligned(16))) bf16_t Ks[3 * G::K_ELEMS];  // plane pl (0 = hi, 1 = mid, 2 = lo) at pl * K_ELEMS
    __shared__ __attribute__((aligned(16))) bf16_t Vt[3 * G::V_ELEMS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int image = blockIdx.x / qblocks, qblock = blockIdx.x - image * qblocks, head = blockIdx.y;
    const size_t D = (size_t)heads * HD, ld = 3 * D;
    const float *rows = qkv + (size_t)image * tokens * ld + (size_t)head * HD;  // the image's token rows, this head's Q columns
    const float *krows = rows + D, *vrows = rows + 2 * D;
    const int qrow0 = qblock * SP_QROWS + wave * 32;
    const bool active = qrow0 < q_rows;  // wave-uniform: this wave owns query rows
    const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};

    // ---- the pieces of this wave's 32 query rows, for all of the sequence: d = 16 ks + 8 h + (0..7) of row r on the lane
    bf16x8 qf[3][NQ];
    {
        int qrow = qrow0 + r;
        qrow = qrow < q_rows ? qrow : q_rows - 1;  // a row of this image; dropped at the store
        const float *qp = rows + (size_t)qrow * ld + 8 * h;
#pragma unroll
        for (int ks = 0; ks < NQ; ++ks) {
            f32x4 x0 = zero4, x1 = zero4;
            if (active) {
                x0 = *reinterpret_cast<const f32x4 *>(qp + 16 * ks);
                x1 = *reinterpret_cast<const f32x4 *>(qp + 16 * ks + 4);
            }
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) qf[pl][ks] = __builtin_bit_cast(bf16x8, split3_piece8(x0, x1, pl));
        }
    }

    f32x16 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int v = 0; v < 16; ++v) o[dt][v] = 0.0f;
    float m_run = -INFINITY, l_run = 0.0f;  // per query (lane & 31); l_run: this half-wave's keys

    // ---- a chunk of K and V on its way to the LDS: fetch() takes this thread's share into registers (zeros behind the last token),
    // store() splits it and writes the three planes.  K: eight d of a key per item, one 16-byte piece of each plane.  V transposed:
    // the same 8 d of two adjacent keys per item, 8 dword writes per plane, adjacent lanes on adjacent banks.
    constexpr int K_ITEMS = KC * (HD / 8), V_ITEMS = (KC / 2) * (HD / 8);
    constexpr int KI = (K_ITEMS + SP_THREADS - 1) / SP_THREADS;
    constexpr int V_TID0 = SP_THREADS > V_ITEMS ? SP_THREADS - V_ITEMS : 0;  // V goes to the last waves: with 8, the one without rows at 197 tokens
    static_assert(V_ITEMS <= SP_THREADS, "one V item per thread at most");
    const int vi = tid - V_TID0;
    f32x4 kx[KI][2], vx[4];
    auto fetch = [&](int key0) {
#pragma unroll
        for (int it = 0; it < KI; ++it) {
            const int i = tid + it * SP_THREADS, row = i / (HD / 8), c = i - row * (HD / 8), key = key0 + row;
            kx[it][0] = kx[it][1] = zero4;
            if (i < K_ITEMS && key < tokens) {
                const float *p = krows + (size_t)key * ld + 8 * c;
                kx[it][0] = *reinterpret_cast<const f32x4 *>(p);
                kx[it][1] = *reinterpret_cast<const f32x4 *>(p + 4);
            }
        }
        if (vi >= 0) {
            const int c = vi / (KC / 2), key = key0 + 2 * (vi - c * (KC / 2));
#pragma unroll
            for (int j = 0; j < 4; ++j) vx[j] = zero4;
            if (key < tokens) {
                const float *p = vrows + (size_t)key * ld + 8 * c;
                vx[0] = *reinterpret_cast<const f32x4 *>(p);
                vx[1] = *reinterpret_cast<const f32x4 *>(p + 4);
            }
            if (key + 1 < tokens) {
                const float *p = vrows + (size_t)(key + 1) * ld + 8 * c;
                vx[2] = *reinterpret_cast<const f32x4 *>(p);
                vx[3] = *reinterpret_cast<const f32x4 *>(p + 4);
            }
        }
    };
    auto store = [&](bf16_t *Kd, bf16_t *Vd) {
#pragma unroll
        for (int it = 0; it < KI; ++it) {
            const int i = tid + it * SP_THREADS, row = i / (HD / 8), c = i - row * (HD / 8);
            if (i < K_ITEMS) {
#pragma unroll
                for (int pl = 0; pl < 3; ++pl)
                    *reinterpret_cast<u32x4 *>(Kd + pl * G::K_ELEMS + row * KROW + 8 * c) = split3_piece8(kx[it][0], kx[it][1], pl);
            }
        }
        if (vi >= 0) {
            const int c = vi / (KC / 2), row = 2 * (vi - c * (KC / 2));
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                const u32x4 a = split3_piece8(vx[0], vx[1], pl), b = split3_piece8(vx[2], vx[3], pl);
                bf16_t *vd = Vd + pl * G::V_ELEMS + (c * 8) * VROW + row;
#pragma unroll
                for (int j = 0; j < 4; ++j) {  // elements 2j, 2j + 1 of the piece: key `row` in the low half, key row + 1 in the high half
                    *reinterpret_cast<unsigned *>(vd + (2 * j) * VROW) = (a[j] & 0xffffu) | (b[j] << 16);
                    *reinterpret_cast<unsigned *>(vd + (2 * j + 1) * VROW) = (a[j] >> 16) | (b[j] & 0xffff0000u);
                }
            }
        }
    };

    for (int key0 = 0; key0 < tokens; key0 += KC) {
        fetch(key0);
        store(Ks, Vt);
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
                const bf16_t *kp = Ks + (32 * t + r) * KROW + 8 * h;
#pragma unroll
                for (int ks = 0; ks < NQ; ++ks) {
                    bf16x8 kf[3];
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) kf[pl] = *reinterpret_cast<const bf16x8 *>(kp + pl * G::K_ELEMS + 16 * ks);
#pragma unroll
                    for (int term = 0; term < 6; ++term)
                        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[SPLIT_TERM_A[term]], qf[SPLIT_TERM_W[term]][ks], s, 0, 0, 0);
                }
                if (tile0 + 32 > tokens) {  // wave-uniform: the sequence's last tile
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        const int key = tile0 + (v & 3) + 8 * (v >> 2) + 4 * h;
                        s[v] = key < tokens ? s[v] : -INFINITY;
                    }
                }
                // ---- online softmax, as in attention_hd_kernel: p = 2^(scale s - scale m), m the deferred running maximum
                float cmax = s[0];
#pragma unroll
                for (int v = 1; v < 16; ++v) cmax = fmaxf(cmax, s[v]);
                cmax = fmaxf(cmax, __shfl_xor(cmax, 32));
                constexpr float kDefer = 8.0f, scale = kScale64;
                const float m_old = m_run;
                const float m_new = (cmax - m_old) * scale > kDefer ? cmax : m_old;  // first tile: m_old = -inf -> cmax
                const float mneg = -m_new * scale;
                m_run = m_new;
                float sum = 0.0f;
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    s[v] = __builtin_amdgcn_exp2f(fmaf(s[v], scale, mneg));  // exp2(-inf) = 0: masked keys
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
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    if (tile0 + 16 * s2 >= tokens) break;  // wave-uniform: sixteen masked keys
                    f32x4 x0 = {s[8 * s2], s[8 * s2 + 1], s[8 * s2 + 2], s[8 * s2 + 3]};
                    f32x4 x1 = {s[8 * s2 + 4], s[8 * s2 + 5], s[8 * s2 + 6], s[8 * s2 + 7]};
                    bf16x8 pf[3], vf[DT][3];
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) pf[pl] = __builtin_bit_cast(bf16x8, split3_piece8(x0, x1, pl));
#pragma unroll
                    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
                        for (int pl = 0; pl < 3; ++pl) {
                            const bf16_t *vp = Vt + pl * G::V_ELEMS + (32 * dt + r) * VROW + 32 * t + 16 * s2 + 4 * h;
                            const u32x2 lo = *reinterpret_cast<const u32x2 *>(vp), hi = *reinterpret_cast<const u32x2 *>(vp + 8);
                            const u32x4 both = {lo[0], lo[1], hi[0], hi[1]};
                            vf[dt][pl] = __builtin_bit_cast(bf16x8, both);
                        }
#pragma unroll
                    for (int term = 0; term < 6; ++term)
#pragma unroll
                        for (int dt = 0; dt < DT; ++dt)
                            o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[dt][SPLIT_TERM_A[term]], pf[SPLIT_TERM_W[term]], o[dt], 0, 0, 0);
                }
            }
        }
        __syncthreads();  // everybody is done with the chunk
    }

    // ---- normalise and store: a lane holds d = 32 dt + 8 q + 4 h + (0..3) of its query row in registers 4 q .. 4 q + 3
    const int qrow = qrow0 + r;
    if (active && qrow < q_rows) {
        const float inv = 1.0f / (l_run + __shfl_xor(l_run, 32));
        float *dst = out + ((size_t)image * tokens + qrow) * D + (size_t)head * HD + 4 * h;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 w = {o[dt][4 * q] * inv, o[dt][4 * q + 1] * inv, o[dt][4 * q + 2] * inv, o[dt][4 * q + 3] * inv};
                *reinterpret_cast<f32x4 *>(dst + 32 * dt + 8 * q) = w;
            }
    }
}

template <bool BF16, bool QS>
int launch_hd(hipStream_t s, const typename Geo<128, BF16>::elem *qkv, typename Geo<128, BF16>::elem *out, int n_images, int tokens,
              int heads, int head_dim, int q_rows) {
    const int qblocks = (q_rows + HD_QROWS - 1) / HD_QROWS;
    if (heads > 65535 || (long long)n_images * qblocks > 0x7fffffffLL) return static_cast<int>(hipErrorInvalidValue);  // the grid
    const float scale = QS ? 1.0f : vithip_qscale(head_dim);
    return dispatch_int<72, 8, 8>(head_dim, [&](auto hd) {
        hipLaunchKernelGGL((attention_hd_kernel<decltype(hd)::value, BF16, QS>), dim3((unsigned)(n_images * qblocks), (unsigned)heads),
                           dim3(HD_THREADS), 0, s, qkv, out, tokens, heads, q_rows, qblocks, scale);
        return static_cast<int>(hipGetLastError());
    });
}

}  // namespace

// The callers (route() in vit_attention.hip) have checked the arguments every P.V entry shares (vitattn::qkv_args_ok).
int vitattn::attention_hd_f32(hipStream_t s, const float *qkv, float *out, int n_images, int tokens, int heads, int head_dim, int q_rows) {
    return launch_hd<false, false>(s, qkv, out, n_images, tokens, heads, head_dim, q_rows);
}

int vitattn::attention_hd_bf16(hipStream_t s, const unsigned short *qkv, unsigned short *out, int n_images, int tokens, int heads,
                               int head_dim, int q_rows, bool q_scaled) {
    return q_scaled ? launch_hd<true, true>(s, qkv, out, n_images, tokens, heads, head_dim, q_rows)
                    : launch_hd<true, false>(s, qkv, out, n_images, tokens, heads, head_dim, q_rows);
}

int vitattn::attention_split_f32(hipStream_t s, const float *qkv, float *out, int n_images, int tokens, int heads, int q_rows) {
    const int qblocks = (q_rows + SP_QROWS - 1) / SP_QROWS;
    if (heads > 65535 || (long long)n_images * qblocks > 0x7fffffffLL) return static_cast<int>(hipErrorInvalidValue);  // the grid
    hipLaunchKernelGGL(attention_split_kernel, dim3((unsigned)(n_images * qblocks), (unsigned)heads), dim3(SP_THREADS), 0, s, qkv, out,
                       tokens, heads, q_rows, qblocks);
    return static_cast<int>(hipGetLastError());
}

extern "C" float vithip_qscale(int head_dim) {
    if (!vitattn::hd_accepted(head_dim)) return 0.0f;
    return (float)((1.0 / sqrt((double)head_dim)) * 1.4426950408889634074);  // log2(e)
}
