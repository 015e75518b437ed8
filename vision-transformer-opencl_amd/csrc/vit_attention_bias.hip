// csrc/vit_attention_bias.hip -- attention with an additive bias on the scores: softmax(q.k / sqrtf(head_dim) + b[head][query][key]) . V,
// for every accepted head_dim (64, and the multiples of 8 from 72 to 128), fp32 and bf16.  BEiT's relative position bias (BEiT, BEiT v2,
// data2vec-vision, DPT-BEiT, timm's vit_relpos_*), and with -inf entries a key mask.  The entries: vithip_attention_f32_bias /
// _bf16io_bias (vit_hip_kernels.h); the engine calls them for the layers that vit_engine_set_attention_bias has given a bias.
//
// qkv [n*T][3*heads*hd], columns [Q | K | V], head h = columns hd*h.. of each; out [n*T][heads*hd]; bias fp32 [heads][T][ld_bias] in
// natural-log units, one array for every image.
//
// The skeleton is the one of vit_attention_hd.hip: a workgroup of 4 waves takes (image, head, block of 128 query rows); a wave owns 32
// query rows with their online-softmax state and their Q fragments in registers; K and V stream through the LDS in chunks of 64 (bf16)
// or 32 (fp32) keys, single-buffered between two barriers, V transposed while it is staged; S^T = K . Q^T puts a query on a lane, so
// O^T += V^T . P^T takes P from the accumulator as its B operand.  bf16: v_mfma_f32_32x32x16_bf16, P in two bf16 pieces; fp32:
// v_mfma_f32_32x32x2_f32.  The padding of the contraction (head_dim 72, 88, 104, 120 in bf16) and of the last chunk is that file's too.
//
// What is new is the bias and a softmax that lives with -inf:
//
//   The path.  In the S^T orientation register v of a tile's accumulator is key (v & 3) + 8 (v >> 2) + 4 h of the tile for the query
//   on the lane: registers 4q .. 4q+3 are the four consecutive keys 8q + 4h .. of ONE bias row, a 16-byte piece.  A tile is four such
//   loads per lane, and the two half-waves of a query read adjacent pieces: per tile a query's 32 floats are one 128-byte run.  Every
//   bias element is read once, by one lane of one workgroup of an image -- nothing is reused within a workgroup, so the LDS has
//   nothing to offer but a round trip (and 16 - 32 KB that would cost a workgroup per CU): the bias goes from L2 straight to registers.
//   Across images the array is shared, [heads][T][ld_bias] x 4 bytes (1.9 MB at 12 x 197 x 200), and stays in L2.
//
//   Where the loads are issued.  At the head of the chunk loop, all of the chunk's tiles (KT x 4 loads per lane), IN FRONT of the
//   chunk's K and V loads.  Vector memory returns in order: the wait that the staging pass needs for its own K / V data before it
//   writes the LDS retires the bias loads in front of them as well, so their latency lies under the staging's own; behind the barrier
//   the score MFMAs find the bias in registers and the softmax waits for nothing.  The conversion to the exponent's unit (times log2(e))
//   is done on arrival, in the same registers.
//
//   Registers.  16 per tile: 32 (bf16, two tiles) or 16 (fp32) more than attention_hd_kernel holds through the staging pass.  That
//   kernel's bf16 form up to head_dim 96 is capped at 128 VGPRs for four workgroups per CU; with the bias it would spill there.  Here
//   head dims up to 80 (three O^T tiles at most) leave room for three waves per SIMD (168 VGPRs, three workgroups of 4 waves per CU:
//   146 - 168 allocated, none spilled), and from head_dim 88 on, where that cap spills 2 to 61 registers, for two (256) -- MIN_WAVES below.
//   No instance spills or uses scratch.
//
//   Bounds.  A piece starts at a key that is a multiple of 4 and ld_bias % 4 == 0, so a piece whose first key is below ld_bias lies
//   inside its row; a piece at or behind ld_bias is not loaded (the ragged last chunk: its registers are -inf).  Columns [T, ld_bias) may
//   thus be read; keys >= T are SELECTED to -inf afterwards, never added, so their bits (NaN patterns included) reach nothing.  Query
//   rows past q_rows are clamped to row q_rows - 1 for Q and for the bias alike (the 129th row of a second block, or all but one lane
//   at q_rows = 1) and dropped at the store: every address is inside [heads][T][ld_bias] and inside the image's rows.
//
//   The softmax.  x = scale s + log2(e) b is formed with one fma per score (q_scaled: one add) and the online softmax runs on x: running
//   maximum m (moved only when outgrown by more than 2^8, as in the hd kernel), p = exp2(x - m).  A bias of -inf gives x = -inf and
//   p = exp2(-inf) = 0, exactly.  A tile -- or every tile so far -- may hold nothing but -inf for a row: then m stays -inf, and both
//   places where -inf - -inf would make a NaN are guarded: the subtrahend is 0 while m is -inf (p = exp2(-inf - 0) = 0), and the rescale
//   factor of a row whose maximum did not move is 1 by selection, not exp2(m - m).  A row whose only finite entry is key j with
//   p = exp2(x_j - x_j) = 1 therefore returns V's row j bit for bit.  A row with no finite entry at all ends with l = 0: NaN, the caller's error.
//
// A workgroup reads one image's rows (and the shared bias) only; no atomics; an image's bits depend on neither the batch nor its place in it.
#include <hip/hip_runtime.h>

#include <math.h>

#include <type_traits>

#include "vit_attention.hpp"
#include "vit_hip_kernels.h"

namespace {

using namespace vitattn;
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

constexpr int AB_WAVES = 4, AB_THREADS = AB_WAVES * 64;
constexpr int AB_QROWS = AB_WAVES * 32;  // query rows per workgroup
constexpr float kLog2e = 1.4426950408889634f;

template <int HD, bool BF16>
struct Geo {  // the LDS images of vit_attention_hd.hip
    typedef typename std::conditional<BF16, bf16_t, float>::type elem;
    static constexpr int VEC = BF16 ? 8 : 4;              // elements of a 16-byte piece
    static constexpr int KC = BF16 ? 64 : 32;             // keys per chunk
    static constexpr int KT = KC / 32;                    // 32-key tiles per chunk
    static constexpr int DT = (HD + 31) / 32;             // 32-row tiles of O^T
    static constexpr int HDK = BF16 ? (HD + 15) / 16 * 16 : HD;  // contraction length of the scores, padded to the instruction's K
    static constexpr int KROW = HDK + (BF16 ? 8 : 4);     // K image: elements per key row (an odd number of 16-byte slots)
    static constexpr int VROW = KC + 4;                   // V^T image: elements per d row
    static constexpr int K_ELEMS = KC * KROW, V_ELEMS = DT * 32 * VROW;
    static constexpr int MIN_WAVES = HD <= 80 ? 3 : 2;    // waves per SIMD the register allocation leaves room for (the head of the file)
};

template <int HD, bool BF16, bool QS>
__global__ __launch_bounds__(AB_THREADS, (Geo<HD, BF16>::MIN_WAVES)) void attention_bias_kernel(
    const typename Geo<HD, BF16>::elem *__restrict__ qkv, typename Geo<HD, BF16>::elem *__restrict__ out, const float *__restrict__ bias,
    size_t ld_bias, int tokens, int heads, int q_rows, int qblocks, float scale) {
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
    const int qrow0 = qblock * AB_QROWS + wave * 32;
    const bool active = qrow0 < q_rows;  // wave-uniform: this wave owns query rows
    int qrow_in = qrow0 + r;
    qrow_in = qrow_in < q_rows ? qrow_in : q_rows - 1;  // a row of this image and of the bias; dropped at the store
    // this lane's bias row, at its half-wave's first piece: key k of a tile at tile0 is brow[tile0 + 8 q + (k & 3)], q = 0..3
    const float *brow = bias + ((size_t)head * tokens + qrow_in) * ld_bias + 4 * h;

    // ---- Q fragments of this wave's 32 rows, for all of the sequence
    constexpr int NQ = BF16 ? G::HDK / 16 : HD / 8;
    typename std::conditional<BF16, bf16x8, f32x4>::type qf[NQ];
    {
        const elem *qp = rows + (size_t)qrow_in * ld;
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
    float m_run = -INFINITY, l_run = 0.0f;  // per query (lane & 31), m_run in the exponent's unit; l_run: this half-wave's keys

    for (int key0 = 0; key0 < tokens; key0 += KC) {
        // ---- the chunk's bias pieces, in flight in front of the staging pass: b[t][q] = keys key0 + 32 t + 8 q + 4 h + (0..3) of this
        // lane's query row.  A piece at or behind ld_bias is not a load: -inf (its keys are behind the last token)
        f32x4 b[KT][4];
        if (active) {
#pragma unroll
            for (int t = 0; t < KT; ++t)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int col = key0 + 32 * t + 8 * q;  // + 4 h: in brow
                    f32x4 w = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                    if ((size_t)(col + 4 * h) < ld_bias) w = *reinterpret_cast<const f32x4 *>(brow + col);
                    b[t][q] = w;
                }
        }
        // ---- stage the chunk: K as it lies (zeros behind hd and behind the last token), V transposed (zeros behind the last token)
        constexpr int KP = G::HDK / VEC;  // 16-byte pieces of a K image row
        for (int i = tid; i < KC * KP; i += AB_THREADS) {
            const int row = i / KP, c = i - row * KP, key = key0 + row;
            u32x4 w = {0u, 0u, 0u, 0u};
            if (key < tokens && c * VEC < HD) w = *reinterpret_cast<const u32x4 *>(krows + (size_t)key * ld + c * VEC);
            *reinterpret_cast<u32x4 *>(Ks + row * KROW + c * VEC) = w;
        }
        constexpr int VP = HD / VEC;      // 16-byte pieces of a V row
        if constexpr (BF16) {  // the same 8 d of two adjacent keys per thread: 8 dword writes, adjacent lanes on adjacent banks
            for (int i = tid; i < (KC / 2) * VP; i += AB_THREADS) {
                const int c = i / (KC / 2), row = 2 * (i - c * (KC / 2)), key = key0 + row;
                u32x4 a = {0u, 0u, 0u, 0u}, bb = {0u, 0u, 0u, 0u};
                if (key < tokens) a = *reinterpret_cast<const u32x4 *>(vrows + (size_t)key * ld + c * VEC);
                if (key + 1 < tokens) bb = *reinterpret_cast<const u32x4 *>(vrows + (size_t)(key + 1) * ld + c * VEC);
#pragma unroll
                for (int j = 0; j < 4; ++j) {  // elements 2j, 2j + 1 of the piece: key `row` in the low half, key row + 1 in the high half
                    *reinterpret_cast<unsigned *>(Vt + (c * 8 + 2 * j) * VROW + row) = (a[j] & 0xffffu) | (bb[j] << 16);
                    *reinterpret_cast<unsigned *>(Vt + (c * 8 + 2 * j + 1) * VROW + row) = (a[j] >> 16) | (bb[j] & 0xffff0000u);
                }
            }
        } else {
            for (int i = tid; i < KC * VP; i += AB_THREADS) {
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
                // ---- the exponent x = scale s + log2(e) b; a key behind the last token: -inf by selection, whatever its piece held
                const bool last = tile0 + 32 > tokens;  // wave-uniform: the sequence's last tile
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const float bl = b[t][v >> 2][v & 3] * kLog2e;
                    const float x = QS ? s[v] + bl : fmaf(s[v], scale, bl);
                    const int key = tile0 + (v & 3) + 8 * (v >> 2) + 4 * h;
                    s[v] = last && key >= tokens ? -INFINITY : x;
                }
                // ---- online softmax on x: p = 2^(x - m), m the deferred running maximum (a reference, not a bound: it moves only when
                // a row outgrows it by more than kDefer, and P then reaches 2^kDefer instead of 1 -- vit_attention_hd.hip)
                float cmax = s[0];
#pragma unroll
                for (int v = 1; v < 16; ++v) cmax = fmaxf(cmax, s[v]);
                cmax = fmaxf(cmax, __shfl_xor(cmax, 32));
                constexpr float kDefer = 8.0f;
                const float m_old = m_run;
                // nothing finite so far (m_old = -inf) and a finite key: inf > kDefer -> cmax; a tile of -inf: NaN or -inf > kDefer is false -> m_old
                const float m_new = cmax - m_old > kDefer ? cmax : m_old;
                const float m_sub = m_new == -INFINITY ? 0.0f : m_new;  // no finite key yet: x - 0 = -inf, p = 0
                m_run = m_new;
                float sum = 0.0f;
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    s[v] = __builtin_amdgcn_exp2f(s[v] - m_sub);  // exp2(-inf) = 0: masked keys
                    sum += s[v];
                }
                if (__any(m_new != m_old)) {  // wave-uniform
                    // the first finite key of a row: exp2(-inf) = 0; a row that did not move: 1 by selection (-inf - -inf is NaN)
                    const float alpha = m_new == m_old ? 1.0f : __builtin_amdgcn_exp2f(m_old - m_new);
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
                        bf16x8 pf, pl;  // bf16(p) and bf16(p - bf16(p)): P accurate to 2^-17 (vit_attention_hd.hip)
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

// What both entries ask: qkv_args_ok, an accepted head_dim, the bias pointer and its leading dimension, and the grid's two limits.
bool bias_args_ok(const void *qkv, const void *out, const float *bias, size_t ld_bias, int n_images, int tokens, int heads, int head_dim,
                  int q_rows) {
    if (!qkv_args_ok(qkv, out, n_images, tokens, heads, q_rows) || !hd_accepted(head_dim)) return false;
    if (!bias || (reinterpret_cast<size_t>(bias) & 15) || ld_bias < (size_t)tokens || ld_bias % 4 != 0) return false;
    const int qblocks = (q_rows + AB_QROWS - 1) / AB_QROWS;
    return heads <= 65535 && (long long)n_images * qblocks <= 0x7fffffffLL;
}

template <bool BF16, bool QS>
int launch_bias(hipStream_t s, const typename Geo<128, BF16>::elem *qkv, typename Geo<128, BF16>::elem *out, const float *bias,
                size_t ld_bias, int n_images, int tokens, int heads, int head_dim, int q_rows) {
    const int qblocks = (q_rows + AB_QROWS - 1) / AB_QROWS;
    const float scale = QS ? 1.0f : vithip_qscale(head_dim);
    return dispatch_int<64, 9, 8>(head_dim, [&](auto hd) {
        hipLaunchKernelGGL((attention_bias_kernel<decltype(hd)::value, BF16, QS>), dim3((unsigned)(n_images * qblocks), (unsigned)heads),
                           dim3(AB_THREADS), 0, s, qkv, out, bias, ld_bias, tokens, heads, q_rows, qblocks, scale);
        return static_cast<int>(hipGetLastError());
    });
}

}  // namespace

extern "C" int vithip_attention_f32_bias(vithip_stream_t stream, const float *qkv, float *out, const float *bias, size_t ld_bias,
                                         int n_images, int tokens, int heads, int head_dim, int q_rows) {
    if (!bias_args_ok(qkv, out, bias, ld_bias, n_images, tokens, heads, head_dim, q_rows)) return static_cast<int>(hipErrorInvalidValue);
    return launch_bias<false, false>(static_cast<hipStream_t>(stream), qkv, out, bias, ld_bias, n_images, tokens, heads, head_dim, q_rows);
}

extern "C" int vithip_attention_bf16io_bias(vithip_stream_t stream, const unsigned short *qkv, unsigned short *out, const float *bias,
                                            size_t ld_bias, int n_images, int tokens, int heads, int head_dim, int q_rows, int q_scaled) {
    if (!bias_args_ok(qkv, out, bias, ld_bias, n_images, tokens, heads, head_dim, q_rows) || (q_scaled != 0 && q_scaled != 1))
        return static_cast<int>(hipErrorInvalidValue);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    return q_scaled ? launch_bias<true, true>(s, qkv, out, bias, ld_bias, n_images, tokens, heads, head_dim, q_rows)
                    : launch_bias<true, false>(s, qkv, out, bias, ld_bias, n_images, tokens, heads, head_dim, q_rows);
}
