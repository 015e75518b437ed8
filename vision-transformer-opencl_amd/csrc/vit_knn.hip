// csrc/vit_knn.hip -- the k nearest rows of a feature bank for every query row, as records: a similarity GEMM whose epilogue is a
// selection.  score[i][g] = sum_d q[i][d] * bank[g][d]; no [n][G] array is written anywhere.  DESIGN 4.25.
//
// Work split: the grid is (tiles of QT = 32 queries) x (slices of the bank).  A workgroup of four waves walks its slice in tiles of
// BT = 128 bank rows; wave w owns rows 32 w .. 32 w + 31 of the tile and all 32 queries: one 32 x 32 accumulator of S^T = bank . Q^T,
// so lane l holds query l % 32 and sixteen bank rows of it.  The K loop streams both operands through LDS in chunks of KC = 32
// columns, the next chunk's global loads in flight under this chunk's MFMAs.  Columns behind D, bank rows behind the slice and
// queries behind n are zero-filled in LDS and never read from memory.
//   fp32 bank: v_mfma_f32_32x32x2_f32; lanes 0..31 take columns 0..15 of the chunk, lanes 32..63 columns 16..31.
//   bf16 bank: v_mfma_f32_32x32x16_bf16 with the fp32 query in the three bf16 pieces of vit_split3.hpp, lo, mid, hi in that order:
//              every product is exact in fp32.
// The contraction order of a (query, bank row) pair is fixed by D alone: its score has the same bits whatever the slices, the
// query's place in the batch and n.
//
// Selection: every query of the tile has, in LDS, a candidate list of `cap` = max(256, k + 128 rounded up to 64) entries (score,
// row inside the slice), its length, and a threshold (score, row): the k-th best entry at the list's last compaction, (-inf,
// INT_MAX) before the first.  A lane appends the accumulator entries that come before the threshold in the total order "higher
// score first, among equal scores (==) the lower row first" (LDS atomic on the length; NaN compares false and is never appended).
// A tile adds at most 128 entries to a list, and a list longer than cap - 128 is compacted before the next tile: the wave that owns
// the query finds the k-th best key by a radix select over the 64-bit keys (ordered score bits, then the inverted row; one ballot
// per entry and bit), keeps the k entries that are not behind it and raises the threshold.  The order inside a list depends on
// the atomics, its SET does not: what survives is decided by the total order alone.  At the end of the slice the list is compacted
// once more if it holds more than k, every entry's rank is counted and the records are written in order; slots without a
// candidate hold (0x7fffffff, -inf).  With one slice that is the caller's record row; otherwise the slice's list goes to the
// workspace [n][slices][2k] and one wave per query merges the sorted lists (knn_merge_kernel).  No global atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vit_hip_kernels.h"
#include "vit_split3.hpp"

namespace {

using namespace vitsplit;
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int KNN_QT = 32, KNN_BT = 128, KNN_KC = 32, KNN_THREADS = 256;
constexpr int KNN_PITCH_F = KNN_KC + 4;  // floats per staged fp32 row: 16-byte aligned, rows 4 banks apart
constexpr int KNN_PITCH_H = KNN_KC + 8;  // bf16 per staged bf16 row
constexpr int KNN_MAX_SLICES = 256;      // four lists per lane of the merging wave
constexpr int KNN_EMPTY = 0x7fffffff;
constexpr int KNN_SEL = 6;               // entries per lane in a compaction: cap <= 384
constexpr int KNN_OUT = VITHIP_MAX_NEIGHBOURS / 64;  // entries per lane when the records are written

constexpr int knn_capacity(int k) { return (k + KNN_BT + 63) / 64 * 64 < 256 ? 256 : (k + KNN_BT + 63) / 64 * 64; }
static_assert(knn_capacity(VITHIP_MAX_NEIGHBOURS) == 64 * KNN_SEL, "a compaction holds a whole list in registers");
constexpr size_t knn_stage_bytes(bool bf16) {
    return bf16 ? (size_t)(KNN_BT + 3 * KNN_QT) * KNN_PITCH_H * 2 : (size_t)(KNN_BT + KNN_QT) * KNN_PITCH_F * 4;
}
constexpr size_t knn_lds_bytes(bool bf16, int cap) { return knn_stage_bytes(bf16) + 3 * KNN_QT * 4 + (size_t)KNN_QT * cap * 8; }

// (s, c) comes before (bs, bc) in the total order
__device__ __forceinline__ bool before(float s, int c, float bs, int bc) { return s > bs || (s == bs && c < bc); }

// fp32 bits -> unsigned, ascending with the value; -0.0 and +0.0 (equal scores) give the same key.  No NaN comes here.
__device__ __forceinline__ uint32_t ordered(float s) {
    const uint32_t u = s == 0.0f ? 0u : __float_as_uint(s);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unordered(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }
// the key of an entry: larger = earlier in the total order; row < 2^bits.  Never 0 (ordered(-inf) = 0x007fffff).
__device__ __forceinline__ uint64_t make_key(float s, int row, int bits) {
    return ((uint64_t)ordered(s) << bits) | (uint64_t)(((1u << bits) - 1u) - (uint32_t)row);
}

// One wave compacts one list of m > k entries to its best k (any order) and returns their last as the new threshold.
__device__ void compact_list(float *cs, int *ci, int m, int k, int bits, int lane, float &thr_s, int &thr_i) {
    uint64_t key[KNN_SEL];
    float s[KNN_SEL];
    int row[KNN_SEL];
#pragma unroll
    for (int t = 0; t < KNN_SEL; ++t) {
        const int p = t * 64 + lane;
        key[t] = 0;
        if (p < m) { s[t] = cs[p]; row[t] = ci[p]; key[t] = make_key(s[t], row[t], bits); }
    }
    uint64_t kth = 0;  // the largest value with at least k keys at or above it, built from the top bit down
    for (int b = 31 + bits; b >= 0; --b) {
        const uint64_t trial = kth | (1ull << b);
        int c = 0;
#pragma unroll
        for (int t = 0; t < KNN_SEL; ++t) c += __popcll(__ballot(key[t] >= trial));
        if (c >= k) kth = trial;
    }
    int base = 0;  // every entry is in registers: the list is rewritten from its head
#pragma unroll
    for (int t = 0; t < KNN_SEL; ++t) {
        const bool keep = key[t] >= kth;
        const uint64_t mask = __ballot(keep);
        if (keep) {
            const int p = base + __popcll(mask & ((1ull << lane) - 1ull));
            cs[p] = s[t]; ci[p] = row[t];
        }
        base += __popcll(mask);
    }
    thr_s = unordered((uint32_t)(kth >> bits));
    thr_i = (int)(((1u << bits) - 1u) - (uint32_t)(kth & ((1ull << bits) - 1ull)));
}

// One wave writes a list of m <= k entries as records: entry of rank r (entries before it) to slot r, empty slots behind.
__device__ void write_records(float *cs, int *ci, int m, int k, int bits, int lane, long slice_base, int *dst) {
    uint64_t key[KNN_OUT];
    float s[KNN_OUT];
    int row[KNN_OUT], rank[KNN_OUT];
#pragma unroll
    for (int t = 0; t < KNN_OUT; ++t) {
        const int p = t * 64 + lane;
        key[t] = 0; rank[t] = 0; s[t] = 0.0f; row[t] = 0;
        if (p < m) { s[t] = cs[p]; row[t] = ci[p]; key[t] = make_key(s[t], row[t], bits); }
    }
    // the keys take the entries' place, as the bit patterns of a float and an int: every lane has its own entries in registers
#pragma unroll
    for (int t = 0; t < KNN_OUT; ++t) {
        const int p = t * 64 + lane;
        if (p < m) { cs[p] = __uint_as_float((uint32_t)(key[t] >> 32)); ci[p] = (int)(uint32_t)key[t]; }
    }
    for (int j = 0; j < m; ++j) {
        const uint64_t kj = ((uint64_t)__float_as_uint(cs[j]) << 32) | (uint32_t)ci[j];
#pragma unroll
        for (int t = 0; t < KNN_OUT; ++t) rank[t] += kj > key[t];
    }
#pragma unroll
    for (int t = 0; t < KNN_OUT; ++t)
        if (t * 64 + lane < m) { dst[rank[t]] = (int)(slice_base + row[t]); dst[k + rank[t]] = __float_as_int(s[t]); }
    for (int p = m + lane; p < k; p += 64) { dst[p] = KNN_EMPTY; dst[k + p] = __float_as_int(-INFINITY); }
}

template <bool BF16>
__global__ __launch_bounds__(KNN_THREADS) void knn_slice_kernel(const float *__restrict__ q, size_t ldq, int n, const void *__restrict__ bank_,
                                                                size_t ldb, long G, int D, int k, int cap, long rows_per_slice, int bits,
                                                                int *__restrict__ out, size_t ld_query, size_t ld_slice) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    float *sAf = reinterpret_cast<float *>(lds);                     // fp32: [BT][PITCH_F], then the queries [QT][PITCH_F]
    float *sQf = sAf + KNN_BT * KNN_PITCH_F;
    __bf16 *sAh = reinterpret_cast<__bf16 *>(lds);                   // bf16: [BT][PITCH_H], then the query pieces [3][QT][PITCH_H]
    __bf16 *sQh = sAh + KNN_BT * KNN_PITCH_H;
    float *thr_s = reinterpret_cast<float *>(lds + knn_stage_bytes(BF16));
    int *thr_i = reinterpret_cast<int *>(thr_s + KNN_QT);
    int *cnt = thr_i + KNN_QT;
    float *cs = reinterpret_cast<float *>(cnt + KNN_QT);             // [QT][cap]
    int *ci = reinterpret_cast<int *>(cs + (size_t)KNN_QT * cap);    // [QT][cap]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, qi = lane & 31;
    const int q0 = blockIdx.x * KNN_QT;
    const long slice_base = (long)blockIdx.y * rows_per_slice;
    const int slice_len = (int)(G - slice_base < rows_per_slice ? G - slice_base : rows_per_slice);
    const float *bankf = static_cast<const float *>(bank_) + (size_t)slice_base * ldb;       // the slice's 64-bit base
    const uint16_t *bankh = static_cast<const uint16_t *>(bank_) + (size_t)slice_base * ldb;

    if (tid < KNN_QT) { thr_s[tid] = -INFINITY; thr_i[tid] = 0x7fffffff; cnt[tid] = 0; }

    // staging slots of this thread: the query's float4 at (row tid / 8, column 4 (tid % 8)); fp32 bank: four float4 at rows
    // tid / 8 + 32 i; bf16 bank: two 16-byte runs of eight at (row tid / 4 + 64 i, column 8 (tid % 4))
    const int qrow = tid >> 3, qcol = (tid & 7) * 4;
    const bool qlive = q0 + qrow < n;
    const float *qsrc = q + (size_t)(qlive ? q0 + qrow : 0) * ldq + qcol;
    const int nchunks = (D + KNN_KC - 1) / KNN_KC;

    for (int tile = 0; tile < slice_len; tile += KNN_BT) {
        f32x4 rq, ra[4];
        u32x4 rh[2];
        auto fetch = [&](int d0) {
            rq = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (qlive && d0 + qcol < D) rq = *reinterpret_cast<const f32x4 *>(qsrc + d0);
            if constexpr (BF16) {
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int r = (tid >> 2) + 64 * i, c = (tid & 3) * 8;
                    rh[i] = u32x4{0u, 0u, 0u, 0u};
                    if (tile + r < slice_len && d0 + c < D) rh[i] = *reinterpret_cast<const u32x4 *>(bankh + (size_t)(tile + r) * ldb + d0 + c);
                }
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int r = qrow + 32 * i;
                    ra[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                    if (tile + r < slice_len && d0 + qcol < D) ra[i] = *reinterpret_cast<const f32x4 *>(bankf + (size_t)(tile + r) * ldb + d0 + qcol);
                }
            }
        };
        f32x16 acc;
#pragma unroll
        for (int j = 0; j < 16; ++j) acc[j] = 0.0f;
        fetch(0);
        for (int c = 0; c < nchunks; ++c) {
            __syncthreads();  // the chunk before has been read (first chunk: the lists of the tile before are settled)
            if constexpr (BF16) {
#pragma unroll
                for (int i = 0; i < 2; ++i) *reinterpret_cast<u32x4 *>(sAh + ((tid >> 2) + 64 * i) * KNN_PITCH_H + (tid & 3) * 8) = rh[i];
#pragma unroll
                for (int p = 0; p < 3; ++p)
                    *reinterpret_cast<u32x2 *>(sQh + (p * KNN_QT + qrow) * KNN_PITCH_H + qcol) = split3_piece(rq, p);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) *reinterpret_cast<f32x4 *>(sAf + (qrow + 32 * i) * KNN_PITCH_F + qcol) = ra[i];
                *reinterpret_cast<f32x4 *>(sQf + qrow * KNN_PITCH_F + qcol) = rq;
            }
            __syncthreads();
            if (c + 1 < nchunks) fetch((c + 1) * KNN_KC);
            if constexpr (BF16) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const int col = ks * 16 + half * 8;
                    const bf16x8 a = *reinterpret_cast<const bf16x8 *>(sAh + (wave * 32 + qi) * KNN_PITCH_H + col);
#pragma unroll
                    for (int p = 2; p >= 0; --p) {  // lo, mid, hi: small terms first
                        const bf16x8 b = *reinterpret_cast<const bf16x8 *>(sQh + (p * KNN_QT + qi) * KNN_PITCH_H + col);
                        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
                    }
                }
            } else {
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const f32x4 a = *reinterpret_cast<const f32x4 *>(sAf + (wave * 32 + qi) * KNN_PITCH_F + half * 16 + v * 4);
                    const f32x4 b = *reinterpret_cast<const f32x4 *>(sQf + qi * KNN_PITCH_F + half * 16 + v * 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[e], acc, 0, 0, 0);
                }
            }
        }

        // the selection: lane = query qi, accumulator entry j = bank row 32 wave + 8 (j / 4) + 4 half + j % 4 of the tile
        if (q0 + qi < n) {
            const float ts = thr_s[qi];
            const int ti = thr_i[qi];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int row = tile + wave * 32 + (j >> 2) * 8 + half * 4 + (j & 3);
                const float s = acc[j];
                if (row < slice_len && before(s, row, ts, ti)) {
                    const int p = atomicAdd(&cnt[qi], 1);  // LDS; at most cap - 128 before the tile, at most 128 rows in it
                    cs[(size_t)qi * cap + p] = s; ci[(size_t)qi * cap + p] = row;
                }
            }
        }
        __syncthreads();
        for (int u = 0; u < KNN_QT / 4; ++u) {  // wave w keeps queries 8 w .. 8 w + 7
            const int x = wave * (KNN_QT / 4) + u;
            const int m = __builtin_amdgcn_readfirstlane(cnt[x]);
            if (m > cap - KNN_BT) {
                float ns; int ni;
                compact_list(cs + (size_t)x * cap, ci + (size_t)x * cap, m, k, bits, lane, ns, ni);
                if (lane == 0) { thr_s[x] = ns; thr_i[x] = ni; cnt[x] = k; }
            }
        }
        // the next tile's first barrier stands between these lists and their next readers
    }

    __syncthreads();
    for (int u = 0; u < KNN_QT / 4; ++u) {
        const int x = wave * (KNN_QT / 4) + u;
        if (q0 + x >= n) continue;
        int m = __builtin_amdgcn_readfirstlane(cnt[x]);
        if (m > k) {
            float ns; int ni;
            compact_list(cs + (size_t)x * cap, ci + (size_t)x * cap, m, k, bits, lane, ns, ni);
            m = k;
        }
        write_records(cs + (size_t)x * cap, ci + (size_t)x * cap, m, k, bits, lane, slice_base,
                      out + (size_t)(q0 + x) * ld_query + (size_t)blockIdx.y * ld_slice);
    }
}

// One wave per query: the `slices` sorted lists of the workspace into the record row.  Lane l reads lists l, l + 64, ..; each of the
// k rounds takes the best head of all lists (xor butterfly; bank rows are unique, so every lane sees the same winner while a
// candidate is left, and behind that every head is the empty slot) and moves that list on.
__global__ __launch_bounds__(64) void knn_merge_kernel(const int *__restrict__ ws, int slices, int k, int *__restrict__ records, size_t ld_records) {
    constexpr int LISTS = KNN_MAX_SLICES / 64;
    const int lane = threadIdx.x;
    const int *src = ws + (size_t)blockIdx.x * slices * 2 * k;
    int *dst = records + (size_t)blockIdx.x * ld_records;
    int pos[LISTS], hi[LISTS];
    float hs[LISTS];
#pragma unroll
    for (int t = 0; t < LISTS; ++t) {
        const int l = lane + 64 * t;
        pos[t] = 0; hi[t] = KNN_EMPTY; hs[t] = -INFINITY;
        if (l < slices) { hi[t] = src[(size_t)l * 2 * k]; hs[t] = __int_as_float(src[(size_t)l * 2 * k + k]); }
    }
    for (int j = 0; j < k; ++j) {
        float bs = -INFINITY;
        int bi = KNN_EMPTY, bl = -1;
#pragma unroll
        for (int t = 0; t < LISTS; ++t)
            if (before(hs[t], hi[t], bs, bi)) { bs = hs[t]; bi = hi[t]; bl = lane + 64 * t; }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float os = __shfl_xor(bs, off);
            const int oi = __shfl_xor(bi, off), ol = __shfl_xor(bl, off);
            if (before(os, oi, bs, bi)) { bs = os; bi = oi; bl = ol; }
        }
        if (lane == 0) { dst[j] = bi; dst[k + j] = __float_as_int(bs); }
#pragma unroll
        for (int t = 0; t < LISTS; ++t)
            if (bl == lane + 64 * t) {
                hi[t] = KNN_EMPTY; hs[t] = -INFINITY;
                if (++pos[t] < k) { hi[t] = src[(size_t)bl * 2 * k + pos[t]]; hs[t] = __int_as_float(src[(size_t)bl * 2 * k + k + pos[t]]); }
            }
    }
}

// The slices of a launch and the bank rows of each.  slices = 0, the launcher's rule (profiles/r39/knn.md): about 512 workgroups
// (two per compute unit of a 256-CU device), no slice shorter than four tiles, whole tiles per slice.
int resolve_slices(int n, long G, int slices, long *rows_per_slice) {
    long rps;
    if (slices <= 0) {
        const long qt = (n + KNN_QT - 1) / KNN_QT, tiles = (G + KNN_BT - 1) / KNN_BT;
        long want = 512 / qt, longest = tiles / 4;
        if (want > longest) want = longest;
        if (want > KNN_MAX_SLICES) want = KNN_MAX_SLICES;
        if (want < 1) want = 1;
        rps = (tiles + want - 1) / want * KNN_BT;
    } else {
        const long s = slices < G ? slices : G;
        rps = (G + s - 1) / s;
    }
    *rows_per_slice = rps;
    return (int)((G + rps - 1) / rps);
}

bool knn_args_ok(int n, long G, int D, int k, int slices) {
    return n >= 1 && G >= 1 && G < 0x7fffffffL && D >= 8 && D <= 4096 && D % 8 == 0 && k >= 1 && k <= VITHIP_MAX_NEIGHBOURS &&
           slices >= 0 && slices <= KNN_MAX_SLICES;
}

template <bool BF16>
int launch_knn(hipStream_t s, const float *q, long ldq, int n, const void *bank, long ldb, long G, int D, int k, int *records,
               long ld_records, void *workspace, int slices) {
    const int align = BF16 ? 8 : 4;
    if (!q || !bank || !records || !knn_args_ok(n, G, D, k, slices) || ldq < D || ldq % 4 || ldb < D || ldb % align || ld_records < 2L * k ||
        ((uintptr_t)q & 15) || ((uintptr_t)bank & 15))
        return static_cast<int>(hipErrorInvalidValue);
    long rps;
    const int S = resolve_slices(n, G, slices, &rps);
    if (S > 1 && !workspace) return static_cast<int>(hipErrorInvalidValue);
    int bits = 1;
    while ((1L << bits) < rps) ++bits;
    const int cap = knn_capacity(k);
    const size_t lds = knn_lds_bytes(BF16, cap);
    static bool raised = false;  // per instantiation
    if (!raised) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(knn_slice_kernel<BF16>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e != hipSuccess) return static_cast<int>(e);
        raised = true;
    }
    int *out = S > 1 ? static_cast<int *>(workspace) : records;
    const size_t ld_query = S > 1 ? (size_t)S * 2 * k : (size_t)ld_records, ld_slice = 2 * (size_t)k;
    hipLaunchKernelGGL((knn_slice_kernel<BF16>), dim3((n + KNN_QT - 1) / KNN_QT, S), dim3(KNN_THREADS), lds, s, q, (size_t)ldq, n, bank, (size_t)ldb,
                       G, D, k, cap, rps, bits, out, ld_query, ld_slice);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || S == 1) return static_cast<int>(e);
    hipLaunchKernelGGL(knn_merge_kernel, dim3(n), dim3(64), 0, s, static_cast<const int *>(workspace), S, k, records, (size_t)ld_records);
    return static_cast<int>(hipGetLastError());
}

}  // namespace

extern "C" {

size_t vithip_knn_workspace_bytes(int n, long G, int k, int slices) {
    if (!knn_args_ok(n, G, 8, k, slices)) return 0;
    long rps;
    const int S = resolve_slices(n, G, slices, &rps);
    return (size_t)n * S * 2 * k * sizeof(int);
}

int vithip_knn_slices(int n, long G, int slices) {
    long rps;
    return knn_args_ok(n, G, 8, 1, slices) ? resolve_slices(n, G, slices, &rps) : 0;
}

int vithip_knn_topk_f32(vithip_stream_t stream, const float *q, long ldq, int n, const float *bank, long ldb, long G, int D, int k, int *records,
                        long ld_records, void *workspace, int slices) {
    return launch_knn<false>(static_cast<hipStream_t>(stream), q, ldq, n, bank, ldb, G, D, k, records, ld_records, workspace, slices);
}

int vithip_knn_topk_bf16bank(vithip_stream_t stream, const float *q, long ldq, int n, const unsigned short *bank, long ldb, long G, int D, int k,
                             int *records, long ld_records, void *workspace, int slices) {
    return launch_knn<true>(static_cast<hipStream_t>(stream), q, ldq, n, bank, ldb, G, D, k, records, ld_records, workspace, slices);
}

}  // extern "C"
