// csrc/vit_topk.hip -- the k best classes of every logits row, as records: k labels, then the k scores' fp32 bit patterns.
//
// The score of class c is logits[c] (VITHIP_SCORE_LOGIT) or the probability softmax_top1_f32_kernel (csrc/vit_rowops.hip) stores
// for the same row, bit for bit (VITHIP_SCORE_PROB): both kernels take the row's maximum and its sum of e_c = expf(logits[c] - mx)
// from vit_row::softmax_row_stats (csrc/vit_row.hpp), and p_c = e_c / sum.
// Nothing but the records is written: the probabilities live in LDS while a row is selected from (TOPK_CACHE floats; thread t keeps
// its own classes t, t + 256, ... there and is their only reader, so the cache needs no barrier and lanes touch consecutive banks) or,
// for a longer row, are recomputed from the logits in every selection round.  Both give the same bits: e_c / sum is one expression.
//
// Selection: k rounds.  The candidates of a round are the classes behind the previous round's winner in the total order "higher score
// first; among equal scores (==) the lower label first"; a NaN score compares false with everything and is never one.  Every thread
// finds the best candidate among its own classes, the wave's 64 meet in an xor butterfly, the four waves' in LDS, where every thread
// reads them (two buffers, used in turn: one barrier per round).  Labels are unique, so the order is total and the winner does not
// depend on the order in which candidates meet.  "Best" starts as the empty slot (0x7fffffff, -1.0f or -INFINITY), which every
// candidate beats -- a -INFINITY logit by its smaller label -- so a round without candidates yields the empty slot, and so does every
// round behind it.  One workgroup per row, no atomics: a row's records depend on that row's logits alone.
#include <hip/hip_runtime.h>

#include "vit_hip_kernels.h"
#include "vit_row.hpp"

namespace {

constexpr int TOPK_THREADS = vit_row::THREADS;
constexpr int TOPK_WAVES = TOPK_THREADS / 64;
constexpr int TOPK_CACHE = 4096;  // floats of LDS for a row's scores; a longer row is recomputed per round
constexpr int TOPK_EMPTY = 0x7fffffff;

// (s, c) comes before (bs, bc) in the total order
__device__ __forceinline__ bool before(float s, int c, float bs, int bc) { return s > bs || (s == bs && c < bc); }

template <bool PROB, bool CACHED>
__global__ __launch_bounds__(TOPK_THREADS) void softmax_topk_f32_kernel(const float *__restrict__ logits, int ld_logits,
                                                                        int *__restrict__ out, int ld_out, int classes, int k) {
    __shared__ float red_f[2][TOPK_WAVES];
    __shared__ int red_i[2][TOPK_WAVES];
    __shared__ float cache[CACHED ? TOPK_CACHE : 1];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *src = logits + (size_t)row * ld_logits;
    int *dst = out + (size_t)row * ld_out;

    float mx = 0.0f, sum = 1.0f;
    if (PROB) {
        vit_row::softmax_row_stats(src, classes, red_f, mx, sum, [&](int c, float e) {
            if (CACHED) cache[c] = e;
        });
        // no barrier here: round 0 writes red_f[0], which everyone read in front of the function's second barrier, and round 1
        // writes red_f[1] behind round 0's barrier
        if (CACHED)
            for (int c = tid; c < classes; c += TOPK_THREADS) cache[c] = cache[c] / sum;
    } else if (CACHED) {
        for (int c = tid; c < classes; c += TOPK_THREADS) cache[c] = src[c];
    }

    const float empty = PROB ? -1.0f : -INFINITY;
    float ps = INFINITY;  // the previous winner: every non-NaN score is a candidate behind (+inf, -1)
    int pc = -1;
    for (int j = 0; j < k; ++j) {
        float bs = empty;
        int bc = TOPK_EMPTY;
        for (int c = tid; c < classes; c += TOPK_THREADS) {
            const float s = CACHED ? cache[c] : (PROB ? expf(src[c] - mx) / sum : src[c]);
            if (before(ps, pc, s, c) && before(s, c, bs, bc)) { bs = s; bc = c; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float os = __shfl_xor(bs, off);
            const int oc = __shfl_xor(bc, off);
            if (before(os, oc, bs, bc)) { bs = os; bc = oc; }
        }
        const int buf = j & 1;
        if (lane == 0) { red_f[buf][wave] = bs; red_i[buf][wave] = bc; }
        __syncthreads();
        bs = red_f[buf][0]; bc = red_i[buf][0];
#pragma unroll
        for (int w = 1; w < TOPK_WAVES; ++w)
            if (before(red_f[buf][w], red_i[buf][w], bs, bc)) { bs = red_f[buf][w]; bc = red_i[buf][w]; }
        if (tid == 0) { dst[j] = bc; dst[k + j] = __float_as_int(bs); }
        ps = bs; pc = bc;
    }
}

template <bool PROB>
int launch_topk(hipStream_t s, const float *logits, int ld_logits, int *out, int ld_out, int rows, int classes, int k) {
    if (classes <= TOPK_CACHE)
        hipLaunchKernelGGL((softmax_topk_f32_kernel<PROB, true>), dim3(rows), dim3(TOPK_THREADS), 0, s, logits, ld_logits, out, ld_out,
                           classes, k);
    else
        hipLaunchKernelGGL((softmax_topk_f32_kernel<PROB, false>), dim3(rows), dim3(TOPK_THREADS), 0, s, logits, ld_logits, out, ld_out,
                           classes, k);
    return static_cast<int>(hipGetLastError());
}

}  // namespace

extern "C" {

int vithip_softmax_topk_f32(vithip_stream_t stream, const float *logits, int ld_logits, int *out, int ld_out, int rows, int classes,
                            int k, int score) {
    if (!logits || !out || rows <= 0 || k < 1 || k > classes || k > VITHIP_MAX_TOPK || ld_logits < classes || ld_out < 2 * k ||
        (score != VITHIP_SCORE_PROB && score != VITHIP_SCORE_LOGIT))
        return static_cast<int>(hipErrorInvalidValue);
    hipStream_t s = static_cast<hipStream_t>(stream);
    return score == VITHIP_SCORE_PROB ? launch_topk<true>(s, logits, ld_logits, out, ld_out, rows, classes, k)
                                      : launch_topk<false>(s, logits, ld_logits, out, ld_out, rows, classes, k);
}

}  // extern "C"
