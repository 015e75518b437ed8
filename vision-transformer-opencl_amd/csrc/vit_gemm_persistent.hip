// csrc/vit_gemm_persistent.hip -- persistent, cross-tile pipelined variant of the fp32 NT GEMM.
//
// Same math, tile (BM x BN, K step 32) and fragment scheme as vit_gemm.hip.  What changes is the
// schedule: the grid is 2 workgroups per CU and each workgroup walks a strided list of tiles, treating
// (tile, k-step) as ONE flat sequence.  The staging pipeline (global -> registers -> LDS, two steps
// ahead) therefore runs straight through tile boundaries: while the last K steps of tile i multiply,
// the first K steps of tile i+1 are already being fetched, and the only non-matrix work left at a
// boundary is the store of the finished accumulators.  Measured per 128x128 tile of fc1 in the
// one-tile-per-workgroup kernel: 12.9k cycles of prologue (load latency, LDS fill) + ~10k of epilogue
// + ~5 % of workgroup launch gaps around 187k cycles of K loop; this kernel removes the prologue and
// the launch gaps.
//
// fp32 VALU instructions and v_mfma_f32_32x32x2_f32 share the SIMD's fp32 lanes (tools/valu_probe.py:
// 1 M partner-wave v_fma add 2.4 M cycles to an MFMA-bound loop), so every VALU instruction in the
// loop or the epilogue is paid for in matrix throughput; the bookkeeping below is scalar (SALU)
// wherever it is wave-uniform.
//
// Tile quantisation and the helper pieces (round 2).  fc2 / out_proj at batch 256 are 394 x 6 = 2,364 tiles on 512 workgroups:
// 4.62 rounds paid as 5 -- 316 workgroups own five tiles, 196 four, and for the length of one tile 38 % of the chip idles
// (7.7 % of the kernel; the stage model 0.923 x 0.95 matched the measured 0.877 of the clock-limited peak).  The owners of a
// fifth tile now hand the FIRST x K-steps of it to a four-tile workgroup: the helper runs that piece before its own tiles,
// parks the 64 KB of accumulators in a workspace slot and raises the slot's flag; the owner, at the very end of its walk, loads
// them as its INITIAL accumulators and continues with K-steps x..nk.  Every output still sums its k in the sequential order with
// the same instruction -- the hand-over moves an accumulation chain between workgroups, it does not split it -- so the result is
// bit-identical to the one-workgroup tile (tests/test_gpu_ops.py::test_gemm_tile_shapes_are_bit_identical), which plain
// split-K / stream-K fix-ups are not.  With c = ceil(owners / helpers) pieces per helper and x = floor(nk / (c + 1)) every workgroup
// ends within full x nk + c x steps: fc2 448 instead of 480 (ideal 443.25), out_proj 112 / 120, fc1 444 / 456.
// Dependencies: NOBODY WAITS (round 3).  A helper runs its pieces first thing and waits for nobody.  An owner looks at its
// slot's flag ONCE, three K-steps before its load cursor enters the extra tile (about 380 steps after the helper finished in the
// resident case): piece there -> its walk ends with [x, nk) from the parked accumulators; piece not there (helper not resident
// yet: another lane's or process's kernels hold its CU, ...) -> the owner withdraws the request (flag 0 -> 2) and runs the
// whole tile [0, nk) itself, the helper finds the 2 when it parks and clears it.  Either way every output sums its k in the
// same order: no code path stores a tile whose accumulators it did not wait for, nothing spins, nothing can time out, and
// the hand-over needs no co-residency of the grid (lanes > 1, shared devices).  The two outcomes are counted in the
// workspace (vithip_gemm_f32_workspace_stats): a recomputed piece costs x K-steps of one workgroup, never a wrong bit.
#include "vit_device.hpp"
#include "vit_gemm_common.hpp"

namespace vitgemm {

constexpr int PBK = 32;           // K step
constexpr int PLD = PBK + 4;      // padded LDS row (floats)
// workspace: [SK_HEADER_BYTES of ints: flag per owner | two counters] [slots of 128 x 128 x 4 bytes]
constexpr int SK_HEADER_BYTES = 4096, SK_MAX_OWNERS = 1000, SK_STAT_TAKEN = 1016, SK_STAT_RECOMPUTED = 1017;

// SK: helper pieces compiled in (launches without them use the SK = false instantiation: no segment bookkeeping in its registers)
// DBG: timing-only switch-off instantiations for tools/gemm_f32_switchoff.py, results wrong by construction; instantiated in the
// probe build only (libvit_mi355x_probe.so, tile codes 131-136), the product library holds DBG = 0 alone: 1 no epilogue stores,
// 2 no staging loads inside the K loop, 3 no K-loop barrier, 4 no fragment reads, 5 no staging ds_writes, 6 = 2 + 5.
// (What such builds measure is mostly the POWER of frozen operand data, not the removed instructions: DESIGN 4.1 item 11.)
// ARITH = ARITH_SPLIT3: the three-piece split on the bf16 matrix pipe (vit_gemm_common.hpp): the same walk, hand-over and
// epilogues, K step SPLIT_BK, LDS rows of SPLIT_LD floats (56 KB at 128 x 128).
// WIMG (split only): W's pieces come ready-made from the weight image p.w_split and A is split in registers -- no vector
// instruction and no LDS instruction touches W in the loop.  A wave loads its W fragments of the next K step straight from the
// image, in matrix operand order, under this step's matrix instructions (TN x 3 16-byte buffer loads per lane and step: mid and
// lo in place behind their last use, hi into a spare set; split3_step_pf).
// LDS holds A only: per thread and K step 8 consecutive k of one row of A (two 16-byte loads, split into three 16-byte plane
// chunks) written with ds_write_b128 into swizzled rows of SPLIT_LD_SW floats (two buffers, 32 KB), conflict-free (see
// split_swizzle).  The same pieces in the same places of the product: the same bits as WIMG = false.  A's split is dealt out in
// quarters of a plane over the first 14 gaps between the step's matrix instructions (restage_fine) and, except under the residual
// epilogues, A's fragments of the next step are read under this step's matrix instructions (PIPE).
// (Measured against the step that copied W's chunks through LDS -- 3 ds_write_b128 and 6 ds_read_b128 more per wave and step,
// 64 KB: +2.3 % images/s at the metric configuration; per launch in the forward the residual walks -4.9 %, QKV -1.8 %,
// fc1 -1.4 %: profiles/r30.)
// The image walk in 64 x 256 tiles (BM = 64, BN = 256; launch_persistent picks it where N % 256 == 0, walk_tile()): the four waves
// sit 1 x 4, each on the 64 x 64 wave tile and the 48 matrix instructions per 32 of k it has in the 128 x 128 walk, and share ONE
// split of A: the workgroup stages 64 rows x 32 k per K step (KSUB = 2 sub-steps of 16; a thread's work per step is unchanged, so per
// matrix instruction the split, the ds_write_b128, the loads of A and the barriers are halved) into two 16-deep sub-buffers of the
// same swizzled rows, runs split3_step_pf's body once per sub-buffer and meets at one barrier per 32 of k.  A wave column reads
// panel 2 tn + wn / 2 of the image, rows (wn % 2) * 64 + ...; every wave's W is now its own (no duplicate request for L1 to
// absorb).  K steps, the load cursor's lead, the hand-over's pieces and the fold's counted wait are in 32-deep steps here; the
// accumulators, the epilogues, the 64 KB parking slots and the bits are the 128 x 128 walk's.  (Measured per launch at batch 256
// against the 128 x 128 image walk: QKV -8 %, fc1 -8.5 %, fc2 -5 %, out_proj -4 %: profiles/r32.)
template <int BM, int BN, int WM, int WN, int EPI, bool STAMP = false, bool SK = false, int DBG = 0, int ARITH = ARITH_F32,
          bool WIMG = false>
__global__ __launch_bounds__(256, 2) void gemm_f32_nt_persistent_kernel(const GemmParams p) {
    constexpr bool SPLIT = ARITH == ARITH_SPLIT3;
    static_assert(!SPLIT || DBG == 0, "switch-off builds are fp32 only");
    // KSUB: 16-deep sub-steps per K step of the image walk.  128 x 128 (waves 2 x 2): one.  64 x 256 (waves 1 x 4): two -- the
    // workgroup splits 64 rows x 32 k per step, the same 8 consecutive k per thread, for twice the matrix instructions.
    constexpr int KSUB = (WIMG && BM * 2 == WIMG_ROWS) ? 2 : 1;
    static_assert(!WIMG || (SPLIT && BM * KSUB == WIMG_ROWS && BM * BN == WIMG_ROWS * WIMG_ROWS && WN == 64),
                  "the weight image feeds the split walks of 128 x 128 and 64 x 256: whole panels of the image, 64 KB of accumulators");
    // The pipelined step pays under the fold consumers' walks (QKV, fc1) and not under the residual ones (out_proj, fc2), which are
    // faster with the finer slots alone: measured per launch at batch 256, profiles/r21, and again with W fed from the image
    // (fc2 +1.5 % per launch and -0.6 % images/s with the residual walks pipelined too, profiles/r30).
    constexpr bool PIPE = WIMG && EPI != VITHIP_EPI_BIAS_RESIDUAL && EPI != EPI_RESIDUAL_STATS;
    constexpr int PBK = SPLIT ? SPLIT_BK * KSUB : vitgemm::PBK;  // K step
    constexpr int PLD = WIMG ? SPLIT_LD_SW : SPLIT ? SPLIT_LD : vitgemm::PLD;  // LDS row (floats)
    constexpr int ROWS_PER_PASS = 256 / (PBK / 4);
    constexpr int WGN = BN / WN;
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int A_CHUNKS = BM * (PBK / 4) / 256;
    constexpr int B_CHUNKS = BN * (PBK / 4) / 256;
    constexpr int NC = PBK / 8;              // 8-deep chunks per K step (fp32)
    constexpr int NS = A_CHUNKS + B_CHUNKS;  // staged float4 per thread per K step
    constexpr int W_FRAGS = 3 * TN * KSUB;   // WIMG: image chunks per lane per K step (one per plane, 32-row block of the wave and sub-step)
    constexpr int NL = WIMG ? A_CHUNKS + W_FRAGS : NS;  // global loads per thread per (prefetching) K step
    static_assert(!WIMG || (A_CHUNKS == 2 && BM * 2 * KSUB == 256), "WIMG: one 8-deep half row of A (of one sub-step) per thread");
    constexpr int A_SUB = BM * PLD;          // floats of one 16-deep (sub-)buffer of A
    constexpr int A_BUF = KSUB * A_SUB;      // ... of one K step's buffer
    constexpr int NM = 4 * TM * TN;          // MFMAs per chunk
    static_assert((BM / WM) * WGN == 4, "4 waves per workgroup");

    __shared__ __attribute__((aligned(16))) float lds[2 * (WIMG ? BM * KSUB : BM + BN) * PLD];  // WIMG: A only
    __shared__ int sk_decision;  // owner: 1 = the helper's piece is there (written by thread 0, read by all after a barrier)
    // LayerNorm fold, consumer epilogues: (rstd, mean) of the tile's BM rows = 1 KB, copied here when the tile BEGINS by one
    // global -> LDS instruction of wave 0 (16 bytes per lane), written as inline assembly so that it stays off the compiler's
    // vmcnt book-keeping: a value fetched at the tile's start and consumed at its end -- in registers or through the
    // buffer-load-to-LDS builtin alike -- makes the compiler wait for EVERYTHING in flight at the point of use (it cannot count
    // the restage loads of a run-time number of K-steps in between): a drained staging pipeline once per tile, measured +0.8 us
    // per tile (fc1 +2 %).  vmcnt retires in order, so "at most 16 outstanding" at the top of the tile's LAST K-step means the
    // copy, at least three K-steps and 24 loads old by then, has landed; the barrier inside that step publishes it.  Two buffers,
    // alternating: wave 0 issues the next tile's copy as soon as ITS epilogue is done, while the other waves may still be reading
    // the finished tile's pairs; a buffer's next writer is two tiles (many barriers) later.  (An unknown younger operation in the
    // queue only makes the compiler's own counted waits wait for one load more than they need.)
    constexpr bool FOLD = epi_is_fold(EPI);
    // (A 64-row tile has 512 bytes of pairs.  The copy stays one instruction of all 64 lanes and each buffer stays FOLD_ROWS pairs:
    // the descriptor ends behind the tile's rows, so lanes 32 .. 63 fetch nothing and what they write -- zeros -- lands in the
    // upper half of the tile's OWN buffer, which nobody reads.)
    constexpr int FOLD_ROWS = 128;
    __shared__ __attribute__((aligned(16))) f32x2 fold_rows_lds[FOLD ? 2 * FOLD_ROWS : 2];
    static_assert(!FOLD || (BM <= FOLD_ROWS && FOLD_ROWS * 8 == 64 * 16), "one 16-byte lane copy of 64 lanes = 128 rows");
    float *const As0 = lds;
    float *const Bs0 = WIMG ? lds : lds + 2 * BM * PLD;  // (WIMG: unused)

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int wm = wave / WGN, wn = wave % WGN;

    unsigned long long st0 = 0, st_rt0 = 0, st_loop0 = 0, st_epi = 0;
    // WIMG stamps: the sum over the K steps of the cycles from the step's top (the plain step: leaving its barrier; a segment's
    // first step: in front of its cold W request) to the point in front of its first matrix instruction where A's fragments (LDS)
    // and the W fragments that instruction needs have landed: everything but the youngest four loads, A's two and W-mid's two
    [[maybe_unused]] unsigned long long st_frag = 0, st_top = 0, st_landed = 0;
    auto stamp_top = [&]() __attribute__((always_inline)) {
        if constexpr (STAMP && WIMG) st_top = __builtin_amdgcn_s_memtime();
    };
    auto stamp_landed = [&]() __attribute__((always_inline)) {
        if constexpr (STAMP && WIMG) {
            __builtin_amdgcn_s_waitcnt(0x0074);  // lgkmcnt(0) and vmcnt(4)
            st_landed = __builtin_amdgcn_s_memtime();
        }
    };
    auto stamp_step = [&]() __attribute__((always_inline)) {
        if constexpr (STAMP && WIMG) st_frag += st_landed - st_top;
    };
    if constexpr (STAMP) {
        st0 = __builtin_amdgcn_s_memtime();
        st_rt0 = __builtin_amdgcn_s_memrealtime();
    }

    const int total = p.tiles_m * p.tiles_n;
    const int nwg = gridDim.x;
    const int first = xcd_remap(blockIdx.x, nwg);  // XCD-mates take neighbouring tiles of every round
    if (first >= total) return;                    // workgroup-uniform
    const int nk = p.K / PBK;

    // ---- this workgroup's walk: segments (tile, k0, k1, partial in, partial out), all wave-uniform ----------------------
    //   helper (first >= R, pieces on):  its pieces [0, x) of the owners' extra tiles, then `full` whole tiles
    //   owner  (first <  R):             `full` whole tiles, then its extra tile: [x, nk) from the parked partial, or [0, nk)
    const int full = total / nwg, R = total - full * nwg;
    const int x = SK ? p.sk_x : 0;               // K-steps of an extra tile that its helper runs (0: no pieces)
    const int H = nwg - R;
    const bool owner = first < R;
    const int npre = (x > 0 && !owner && R > 0) ? (R - (first - R) + H - 1) / H : 0;  // owners first-R, first-R+H, ...
    // p.sk_late (tests): a helper runs its pieces AFTER its own tiles, i.e. too late for the owners' look at the flag
    const int pstart = (SK && p.sk_late) ? full : 0, fstart = (SK && p.sk_late) ? 0 : npre;
    const int nseg = npre + full + (owner ? 1 : 0);
    bool took = false;                           // owner: the parked piece is the start of its extra tile (set by decide())
    struct Seg { int tile, k0, k1, in, out; };
    auto get_seg = [&](int i) -> Seg {
        Seg g;
        if (i >= pstart && i < pstart + npre) {
            const int o = (first - R) + (i - pstart) * H;
            g.tile = full * nwg + o; g.k0 = 0; g.k1 = x; g.in = -1; g.out = o;
        } else if (i < npre + full) {
            g.tile = first + (i - fstart) * nwg; g.k0 = 0; g.k1 = nk; g.in = -1; g.out = -1;
        } else {
            g.tile = first + full * nwg; g.k0 = took ? x : 0; g.k1 = nk; g.in = took ? first : -1; g.out = -1;
        }
        return g;
    };

    const int ld_row = tid / (PBK / 4);
    const int ld_kc = (tid % (PBK / 4)) * 4;
    // WIMG: thread t stages row t / 2, k 8 (t % 2) .. 8 (t % 2) + 7 of A; wr_off[plane] = its chunk's place in a tile.
    // 64 x 256: row (t / 2) % 64 of sub-step t / 128, i.e. k 16 (t / 128) + 8 (t % 2) ...: the sub-step is wave-uniform (waves 0, 1
    // and 2, 3) and goes into a_src and wr_off once.  Eight consecutive threads are still one aligned quad of rows x both halves of
    // ONE sub-buffer, so the ds_write_b128 pattern is the conflict-free one of split_swizzle.  (The two sub-steps of a row on
    // neighbouring lanes would put two lanes of a group on the same slot, A_SUB = 8 KB apart: the same banks.)
    const int sw_row = KSUB == 1 ? tid >> 1 : (tid >> 1) & (BM - 1), sw_half = tid & 1;
    const int sw_sub = KSUB == 1 ? 0 : __builtin_amdgcn_readfirstlane(tid / (2 * BM));
    int wr_off[3];
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) wr_off[pl] = WIMG ? sw_sub * A_SUB + split_sw_offset(sw_row, 2 * pl + sw_half) : 0;
    // Staging loads are buffer loads: SGPR descriptor + per-thread 32-bit byte offset + SGPR K offset, so
    // stepping through K costs no vector instruction (a 64-bit v_lshl_add per load otherwise -- and fp32
    // VALU time comes out of the matrix pipe's).  Offsets fit 32 bits: the largest operand (fc2's A at
    // batch 256) is 620 MB; the launcher refuses operands >= 2 GB for this kernel.
    const __amdgpu_buffer_rsrc_t a_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.A), 0, 0x7fffffff, 0x00020000);
    const __amdgpu_buffer_rsrc_t w_rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(WIMG ? p.w_split : static_cast<const void *>(p.W)), 0, 0x7fffffff, 0x00020000);
    int a_src[A_CHUNKS];  // byte offsets
    int b_src[B_CHUNKS];
    f32x4 a_stage[A_CHUNKS], b_stage[B_CHUNKS];
    // WIMG: the lane's chunk (row (wn % 2) * WN + r of the wave's panel, half h) of plane 0 and block j = 0 inside an image block,
    // and the wave's panel of the COMPUTE cursor's tile (scalar; set by begin_segment): W's fragments follow the matrix instructions,
    // not the staging of A.  A tile is BN / 128 panels wide and two waves share a panel: wave column wn reads panel wn / 2 of them.
    constexpr int W_WAVES = WIMG_ROWS / WN;  // wave columns per panel
    const int w_lane = WIMG ? (((wn % W_WAVES) * WN + r) * 2 + h) * 16 : 0;
    const int w_wave_panel = (WIMG && BN > WIMG_ROWS) ? __builtin_amdgcn_readfirstlane(wn / W_WAVES) : 0;
    [[maybe_unused]] int w_panel = 0;

    auto set_sources = [&](int tile) {
        int tm, tn;
        tile_coords(tile, p.tiles_m, p.tiles_n, p.group_m, tm, tn);
        if constexpr (WIMG) {
            int m = tm * BM + sw_row;
            m = m < p.M ? m : p.M - 1;
#pragma unroll
            for (int i = 0; i < A_CHUNKS; ++i) a_src[i] = (m * p.lda + SPLIT_BK * sw_sub + 8 * sw_half + 4 * i) * 4;
            return;
        }
#pragma unroll
        for (int i = 0; i < A_CHUNKS; ++i) {
            int m = tm * BM + ld_row + i * ROWS_PER_PASS;
            m = m < p.M ? m : p.M - 1;
            a_src[i] = (m * p.lda + ld_kc) * 4;
        }
#pragma unroll
        for (int i = 0; i < B_CHUNKS; ++i) {
            int n = tn * BN + ld_row + i * ROWS_PER_PASS;
            n = n < p.N ? n : p.N - 1;
            b_src[i] = (n * p.ldw + ld_kc) * 4;
        }
    };
    auto load_bias = [&](int n0, float (&dst)[TN]) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int n = n0 + wn * WN + j * 32 + r;
            dst[j] = n < p.N ? p.bias[n] : 0.0f;
        }
    };

    // ---- the owner's one look at its slot (workgroup-uniform: thread 0 decides, a barrier and an LDS word tell the rest) -----
    // flag o: (generation << 2) | state, state 1 = piece parked, 2 = request withdrawn; p.sk_gen numbers the launches that use
    // the workspace, so ONLY a word written by THIS launch means anything: whatever an aborted earlier launch left behind (a
    // stale "parked" included) reads as empty.  Relaxed agent-scope atomics on an uncached word; what orders the DATA against the
    // flag is on the helper's side (park()).  A 1 of this generation is only ever written behind this launch's data.
    int *const sk_flags = reinterpret_cast<int *>(p.sk_ws);
    const int SK_PARKED = (p.sk_gen << 2) | 1, SK_WITHDRAWN = (p.sk_gen << 2) | 2;
    int steps = 0;                               // K-steps of the whole walk (loop trip count; decide() may shorten it)
    auto decide = [&]() {
        if (tid == 0) {
            int *const f = sk_flags + first;
            int v = __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            while (v != SK_PARKED) {  // not there: withdraw (whatever stale word is in the way); the helper may park in between
                int expected = v;
                if (__hip_atomic_compare_exchange_strong(f, &expected, SK_WITHDRAWN, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) {
                    v = SK_WITHDRAWN;
                    break;
                }
                v = expected;
            }
            // taken: the slot is free again as soon as this KERNEL ends (its next writer is a later launch on this stream)
            if (v == SK_PARKED) __hip_atomic_store(f, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(sk_flags + (v == SK_PARKED ? SK_STAT_TAKEN : SK_STAT_RECOMPUTED), 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            sk_decision = v == SK_PARKED;
        }
        __syncthreads();
        took = __builtin_amdgcn_readfirstlane(sk_decision) != 0;
        if (took) steps -= x;
    };

    // ---- load cursor: the (segment, k-step) the NEXT staging load will fetch ----------------------
    int seg_l = 0, k_l, kend_l;
    {
        const Seg g = get_seg(0);
        set_sources(g.tile);
        k_l = g.k0;
        kend_l = g.k1;
    }
    auto advance_load_cursor = [&]() {
        if (++k_l == kend_l) {
            // past the last segment the old sources stay: harmless re-reads into a buffer nobody uses
            if (++seg_l < nseg) {
                // the load cursor runs three K-steps ahead of the MFMAs: entering the owner's extra tile is where its first
                // K-step -- x or 0 -- has to be known
                if (SK && owner && x > 0 && seg_l == nseg - 1) decide();
                const Seg g = get_seg(seg_l);
                set_sources(g.tile);
                k_l = g.k0;
                kend_l = g.k1;
            } else {
                k_l = kend_l - 1;
            }
        }
    };
    auto load_step = [&]() {
        const int k0 = k_l * PBK;
#pragma unroll
        for (int i = 0; i < A_CHUNKS; ++i) a_stage[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, a_src[i], k0 * 4, 0));
        if constexpr (WIMG) return;
#pragma unroll
        for (int i = 0; i < B_CHUNKS; ++i) b_stage[i] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(w_rsrc, b_src[i], k0 * 4, 0));
    };
    // a staged float4 -> its LDS row: as it is, or as its three pieces (split)
    auto stage_write = [&](float *row, f32x4 v) __attribute__((always_inline)) {
        if constexpr (SPLIT) split3_store(row, ld_kc, v);
        else *reinterpret_cast<f32x4 *>(row + ld_kc) = v;
    };
    // WIMG: the A chunk of plane `pl` (split off what the earlier planes left of a_stage)
    auto write_a_plane = [&](float *As, int pl) __attribute__((always_inline)) {
        *reinterpret_cast<u32x4 *>(As + wr_off[pl]) = split3_piece8(a_stage[0], a_stage[1], pl);
    };
    auto store_step = [&](int buf) {
        float *As = As0 + buf * A_BUF, *Bs = Bs0 + buf * BN * PLD;
        if constexpr (WIMG) {
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) write_a_plane(As, pl);
            return;
        }
#pragma unroll
        for (int i = 0; i < A_CHUNKS; ++i) stage_write(As + (ld_row + i * ROWS_PER_PASS) * PLD, a_stage[i]);
#pragma unroll
        for (int i = 0; i < B_CHUNKS; ++i) stage_write(Bs + (ld_row + i * ROWS_PER_PASS) * PLD, b_stage[i]);
    };
    // one staging slot (fp32 and the on-the-fly split): write the float4 fetched a step ago, then refetch it for two steps ahead
    auto restage_slot = [&](int q, int buf, int k0) {
        if (q < A_CHUNKS) {
            float *As = As0 + buf * A_BUF;
            if (DBG != 5 && DBG != 6) stage_write(As + (ld_row + q * ROWS_PER_PASS) * PLD, a_stage[q]);
            if (DBG != 2 && DBG != 6) a_stage[q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, a_src[q], k0 * 4, 0));
        } else {
            const int qb = q - A_CHUNKS;
            float *Bs = Bs0 + buf * BN * PLD;
            if (DBG != 5 && DBG != 6) stage_write(Bs + (ld_row + qb * ROWS_PER_PASS) * PLD, b_stage[qb]);
            if (DBG != 2 && DBG != 6) b_stage[qb] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(w_rsrc, b_src[qb], k0 * 4, 0));
        }
    };

    // WIMG: the same in Split3SlotsFine's finer slots
    u32x4 a_plane;  // the plane chunk of A being put together
    auto restage_fine = [&](int q, int buf, int k0) {
        if (q <= 12) {
            const int pl = q / 5, sub = q % 5;  // hi and mid: four quarters and the write; lo: two halves and the write
            // (the empty asm statements pin a quarter's results to its slot: without them the vectoriser and the sinking passes,
            // which scheduling fences do not hold, gather the quarters again in front of the plane's write)
            auto quarter = [&](int s4) __attribute__((always_inline)) {  // values 2 s4, 2 s4 + 1 of the thread's eight
                f32x4 &x = a_stage[s4 >> 1];
                const int o = 2 * (s4 & 1);
                f32x2 xx = {x[o], x[o + 1]};
                unsigned pc = split3_piece2(xx, pl);
                asm volatile("" : "+v"(pc), "+v"(xx));
                x[o] = xx[0];
                x[o + 1] = xx[1];
                a_plane[s4] = pc;
            };
            if (pl < 2 && sub < 4) quarter(sub);
            else if (pl == 2 && sub < 2) {
                quarter(2 * sub);
                quarter(2 * sub + 1);
            } else *reinterpret_cast<u32x4 *>(As0 + buf * A_BUF + wr_off[pl]) = a_plane;
        } else {
            a_stage[q - 13] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, a_src[q - 13], k0 * 4, 0));
        }
    };
    // WIMG: the lane's W fragment (piece `pl`, 32-row block j of the wave's columns) of sub-step `sub` of K step k of the compute
    // cursor's tile, from the image.  The plane goes into the scalar offset and the block is a constant added to the lane's offset
    // (hipcc keeps the sum in a second register): no vector arithmetic in the loop.
    auto load_w_frag = [&](int pl, int j, int k, int sub = 0) __attribute__((always_inline)) {
        return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(w_rsrc, w_lane + j * (32 * 2 * 16),
                                                                                 w_panel + (k * KSUB + sub) * WIMG_BLOCK_BYTES + pl * (WIMG_ROWS * 2 * 16), 0));
    };
    // The pipelined step's restage hook: restage_fine and nothing else.  (It stays a closure of its own: without it hipcc orders two
    // moves in the preamble of the probe build's stamped residual walks differently, profiles/r28.)
    auto restage_any = [&](int q, int buf, int k0) __attribute__((always_inline)) {
        restage_fine(q, buf, k0);
    };

    const int a_frag_off = WIMG ? (wm * WM + r) * PLD : (wm * WM + r) * PLD + h * 4;
    const int b_frag_off = (wn * WN + r) * PLD + h * 4;  // (the image walk reads no W from LDS)
    int frag_poff[3];  // WIMG: the lane's chunk (2 piece + h) inside its rows (the swizzle repeats every 16 rows)
#pragma unroll
    for (int pc = 0; pc < 3; ++pc) frag_poff[pc] = WIMG ? split_sw_offset(r, 2 * pc + h) - r * PLD : 0;
    f32x4 af[2][TM], bf[2][TN];  // fp32 only (the split reads its pieces inside split3_step)
    auto read_frags = [&](int buf, int c, int set) {
        if constexpr (SPLIT) return;
        const float *As = As0 + buf * A_BUF + a_frag_off + c * 8;
        const float *Bs = Bs0 + buf * BN * PLD + b_frag_off + c * 8;
#pragma unroll
        for (int i = 0; i < TM; ++i) af[set][i] = *reinterpret_cast<const f32x4 *>(As + i * 32 * PLD);
#pragma unroll
        for (int j = 0; j < TN; ++j) bf[set][j] = *reinterpret_cast<const f32x4 *>(Bs + j * 32 * PLD);
    };

    // ---- parked accumulators: slot o = 64 KB, float4 q of thread t at ((q * 256 + t) * 16) bytes --------------------------
    // Every access to a slot is a SYSTEM-scope (sc0 sc1) buffer access to UNCACHED device memory: the store is written
    // through to memory and acknowledged (vmcnt) once it is there, the load is served from memory, whichever XCD either side
    // runs on.  A release fence at agent scope would add buffer_wbl2 -- a write-back of the XCD's whole L2, there for ORDINARY
    // stores, of which the hand-over has none (measured with such fences: out_proj +22 %, the A / W panels of the XCD's 63
    // other workgroups went out with it).  What a release needs of these stores is that they have COMPLETED before the flag
    // goes up: every thread waits for its own (s_waitcnt vmcnt(0), written out: a workgroup-scope fence only emits
    // lgkmcnt(0) on gfx950), then the workgroup barrier, then thread 0's flag.
    f32x16 acc[TM][TN];
    constexpr int SC_SYS = 0x11;  // cache policy of the raw buffer builtins on gfx94x/95x: bit 0 = sc0, bit 4 = sc1
    auto slot_rsrc = [&](int o) {
        return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<char *>(p.sk_ws) + SK_HEADER_BYTES + (size_t)o * (BM * BN * 4), 0, BM * BN * 4, 0x00020000);
    };
    auto park = [&](int o) {  // helper: accumulators -> slot o, then the flag
        const __amdgpu_buffer_rsrc_t rs = slot_rsrc(o);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    f32x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = acc[i][j][4 * q4 + e];
                    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs, tid * 16,
                                                           ((i * TN + j) * 4 + q4) * 4096, SC_SYS);
                }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
            // anything but this launch's "withdrawn" -> parked.  Found the owner's withdrawal (it computes the tile itself): clear it
            int cur = __hip_atomic_load(sk_flags + o, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (;;) {
                if (cur == SK_WITHDRAWN) {
                    __hip_atomic_store(sk_flags + o, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    break;
                }
                int expected = cur;
                if (__hip_atomic_compare_exchange_strong(sk_flags + o, &expected, SK_PARKED, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
                cur = expected;  // only the owner writes besides us, and only once
            }
        }
    };
    auto unpark = [&](int o) {  // owner, after decide() saw the flag: the piece is its initial accumulators
        const __amdgpu_buffer_rsrc_t rs = slot_rsrc(o);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int q4 = 0; q4 < 4; ++q4) {
                    const f32x4 v = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, tid * 16, ((i * TN + j) * 4 + q4) * 4096, SC_SYS));
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[i][j][4 * q4 + e] = v[e];
                }
        // The piece has LANDED before the K loop goes on -- said with the builtin, which the compiler's wait-count pass reads
        // (inline assembly it does not): accumulators "possibly still in flight" at the loop header made it put vmcnt(12) / (8) /
        // (5) / (1) in front of the first four MFMAs of EVERY K-step of the helper-piece instantiations, i.e. it drained the staging
        // queue at the top of each step where the plain walk only has its eight counted vmcnt(7).  Once per owner workgroup.
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), nothing else
    };

    // ---- compute cursor --------------------------------------------------------------------------
    int seg_c = 0, k_c, kend_c, m0, n0, out_c;
    [[maybe_unused]] int seg_k0 = 0;  // first K-step of the compute cursor's segment
    float bias_r[TN];
    FoldOperands<TN, TM> fold{};
    [[maybe_unused]] int fold_buf = 0;  // which half of fold_rows_lds the compute cursor's tile uses
    auto begin_segment = [&](int i) {
        const Seg g = get_seg(i);
        int tm, tn;
        tile_coords(g.tile, p.tiles_m, p.tiles_n, p.group_m, tm, tn);
        m0 = tm * BM;
        n0 = tn * BN;
        // the wave's panel of the image: its blocks follow each other in K
        if constexpr (WIMG) w_panel = (tn * (BN / WIMG_ROWS) + w_wave_panel) * (nk * KSUB) * WIMG_BLOCK_BYTES;
        k_c = g.k0;
        seg_k0 = g.k0;
        kend_c = g.k1;
        out_c = g.out;
        if (g.out < 0) load_bias(n0, bias_r);  // consumed at the segment's end
        if constexpr (FOLD) {
            if (g.out < 0) {
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int n = n0 + wn * WN + j * 32 + r;
                    fold.colsum[j] = (p.ln_colsum && n < p.N) ? p.ln_colsum[n] : 0.0f;  // NULL: centred weights
                }
                if (wave == 0) {  // the rows' pairs -> LDS (see fold_rows_lds); rows past M read as zero, never stored
                    const int left = p.M - m0 < BM ? p.M - m0 : BM;
                    const __amdgpu_buffer_rsrc_t rr = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.ln_rows) + (size_t)m0 * 2, 0, left * 8, 0x00020000);
                    const unsigned dst = (unsigned)(size_t)(fold_rows_lds + fold_buf * FOLD_ROWS);
                    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" ::"s"(dst), "v"(lane * 16), "s"(rr) : "memory", "m0");
                }
                fold.rows = fold_rows_lds + fold_buf * FOLD_ROWS;
                fold_buf ^= 1;
            }
        }
        if (SK && g.in >= 0) {
            unpark(g.in);
        } else {
#pragma unroll
            for (int ii = 0; ii < TM; ++ii)
#pragma unroll
                for (int jj = 0; jj < TN; ++jj)
#pragma unroll
                    for (int v = 0; v < 16; ++v) acc[ii][jj][v] = 0.0f;
        }
    };
    begin_segment(0);

    for (int i = 0; i < nseg; ++i) {  // (an owner's extra tile counts in full until decide() says otherwise)
        const Seg g = get_seg(i);
        steps += g.k1 - g.k0;
    }
    // ---- prologue (once per workgroup, not per tile): steps 0 and 1 -----------------------------
    load_step();
    advance_load_cursor();
    store_step(0);
    load_step();
    advance_load_cursor();
    __syncthreads();
    read_frags(0, 0, 0);
    if (DBG == 4) read_frags(0, 1, 1);
    (void)af; (void)bf;

    auto end_segment = [&]() {  // segment finished: store the tile (or park the piece), start the next one
        unsigned long long e0 = 0;
        if constexpr (STAMP) e0 = __builtin_amdgcn_s_memtime();
        if (SK && out_c >= 0) park(out_c);
        else if (DBG != 1 || p.M < 0) {  // (M < 0: never; keeps the MFMAs alive)
            if constexpr (EPI == EPI_RESIDUAL_STATS) epilogue_store_residual_stats<BM, BN, WM, WN>(p, acc, bias_r, m0, n0, wm, wn, r, h);
            else epilogue_store<BM, BN, WM, WN, EPI, A_DENSE>(p, acc, bias_r, m0, n0, wm, wn, r, h, fold);
        }
        if constexpr (STAMP) st_epi += __builtin_amdgcn_s_memtime() - e0;
        if (++seg_c < nseg) begin_segment(seg_c);
    };
    // top of a tile's last step (fold consumers): the copy of its rows' pairs has landed (see fold_rows_lds)
    auto fold_rows_landed = [&]() {
        if constexpr (FOLD) {
            if (out_c < 0) {
                // vmcnt retires in order: once at most FOLD_WAIT = 2 * NS operations are outstanding, everything older than the
                // restage loads of the last two K-steps is done.  The copy was issued before this tile's first restage load, and a
                // tile of FOLD_MIN_STEPS steps has issued (FOLD_MIN_STEPS - 1) * NS >= FOLD_WAIT + NS of them by now.
                // (NL: the global loads a K-step issues -- 4 float4 on the fly; 2 of A + 6 image chunks with WIMG, 2 + 12 per 32-deep
                // step of the 64 x 256 walk: 28 left in flight, and the copy at least 6 + 3 x 14 loads old)
                constexpr int FOLD_WAIT = 2 * NL, FOLD_MIN_STEPS = 4;
                static_assert(FOLD_WAIT <= 63, "vmcnt is a 6-bit count on gfx950");
                static_assert((FOLD_MIN_STEPS - 1) * NL >= FOLD_WAIT + NL, "the copy must be older than the loads the wait leaves in flight");
                if (kend_c - seg_k0 >= FOLD_MIN_STEPS) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(FOLD_WAIT) : "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
        }
    };

    if constexpr (STAMP) st_loop0 = __builtin_amdgcn_s_memtime();
    int cur = 0;
    if constexpr (WIMG) {
        // The image walk (split3_step_pf): segment by segment, so that the fragments are dead at every epilogue by construction --
        // a segment's first step requests W's fragments from the image and reads A's at its top (one exposed load latency per
        // segment), its last step prefetches none.  The load cursor of A, the restage slots, the hand-over and the fold's counted
        // wait are the flat loop's: a prefetching step issues its NL global loads, and the copy is still waited for at the top of
        // the tile's last step.
        // PIPE: A's fragments of the next step are read under this step's matrix instructions, behind the barrier inside the step.
        // The residual walks: A's fragments at the step's top, the barrier at the step's end, the finer slots and W's feed alone.
        Split3Frags<TM, TN> frags;
        auto tile_a = [&](int buf, int sub = 0) { return As0 + buf * A_BUF + sub * A_SUB + a_frag_off; };
        auto step = [&](auto prefetch) __attribute__((always_inline)) {
            constexpr bool PF = decltype(prefetch)::value;
            const int k_ahead = k_l * PBK;  // offset of the step the restage loads of A fetch (two steps ahead)
            if constexpr (!PIPE) split3_read_cold<TM, TN>(frags, tile_a(cur), frag_poff);
            if constexpr (KSUB == 2) {
                // The 32-deep step: two passes, the restage slots of Split3SlotsFine2 over both, one barrier.  Pass 0 (sub-step 0)
                // always prefetches: W of sub-step 1 from the image, and (PIPE) A's fragments of sub-step 1 from the SAME buffer,
                // complete since the barrier of the step before -- no barrier in this pass.  Pass 1 is the 16-deep step of the
                // 128 x 128 walk: the barrier behind instruction SPLIT_PF_BARRIER, every restage write into the other buffer in
                // front of it, the reads of that buffer's sub-step 0 behind it.  Every read of a buffer is issued in front of the
                // barrier of the step that reads it and has landed there (instructions 8 .. 11 of pass 1 use the last of them),
                // and the first write into it comes behind that barrier.  Residual form: cold reads at each pass's top, the
                // barrier at the step's end.
                auto restage = [&](int q) __attribute__((always_inline)) { restage_any(q, cur ^ 1, k_ahead); };
                split3_step_pf<TM, TN, PIPE, true, Split3SlotsFine2, 0, false>(acc, frags, tile_a(cur, 1), frag_poff, restage,
                    [&](int pl, int j) __attribute__((always_inline)) { return load_w_frag(pl, j, k_c, 1); }, [] {}, stamp_landed);
                if constexpr (!PIPE) split3_read_cold<TM, TN>(frags, tile_a(cur, 1), frag_poff);
                split3_step_pf<TM, TN, PF && PIPE, PF, Split3SlotsFine2, 1, true>(acc, frags, tile_a(cur ^ 1), frag_poff, restage,
                    [&](int pl, int j) __attribute__((always_inline)) { return load_w_frag(pl, j, k_c + 1); },
                    [] { if constexpr (PIPE) __syncthreads(); });
            } else
            split3_step_pf<TM, TN, PF && PIPE, PF>(acc, frags, tile_a(cur ^ 1), frag_poff,
                [&](int q) __attribute__((always_inline)) { restage_any(q, cur ^ 1, k_ahead); },
                [&](int pl, int j) __attribute__((always_inline)) { return load_w_frag(pl, j, k_c + 1); },
                [] { if constexpr (PIPE) __syncthreads(); }, stamp_landed);
            stamp_step();
            if constexpr (PIPE) stamp_top();
            advance_load_cursor();
            if constexpr (!PIPE) {
                __syncthreads();
                stamp_top();  // the residual walks' step begins on leaving its barrier
            }
            cur ^= 1;
            ++k_c;
        };
        for (;;) {
            stamp_top();
#pragma unroll
            for (int e = 0; e < 6; ++e)
                split3_w_dst(frags, SPLIT_W_LOADS[e].piece, SPLIT_W_LOADS[e].j) = load_w_frag(SPLIT_W_LOADS[e].piece, SPLIT_W_LOADS[e].j, k_c);
            if constexpr (PIPE) split3_read_cold<TM, TN>(frags, tile_a(cur), frag_poff);
            // The cold fragments have LANDED before the steps begin -- said with the builtin, which the compiler's wait-count pass
            // reads: fragments "possibly still in flight" at the loop header would make it wait for everything in flight at the top
            // of EVERY step (it merges the two ways into the loop), where the warm step leaves the youngest loads in flight.
            __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), nothing else
            while (k_c + 1 < kend_c) step(std::true_type{});
            fold_rows_landed();
            step(std::false_type{});
            end_segment();
            if (seg_c >= nseg) break;
        }
    } else
    for (int g = 0; g < steps; ++g) {
        const int k_ahead = k_l * PBK;  // offset of the step the restage loads fetch (step g + 2)
        if (k_c + 1 == kend_c) fold_rows_landed();
        if constexpr (SPLIT) {
            // one 16-deep step of the split: pieces from buffer `cur`, the staged step g + 1 split into cur^1 and the loads of step
            // g + 2 in the first half of the matrix instructions, then the one barrier (the fp32 loop's swap point)
            split3_step<TM, TN, NS>(acc, As0 + cur * A_BUF + a_frag_off, Bs0 + cur * BN * PLD + b_frag_off,
                                    [&](int q) __attribute__((always_inline)) { restage_slot(q, cur ^ 1, k_ahead); });
            advance_load_cursor();
            __syncthreads();
        } else
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            if (c + 1 < NC && DBG != 4) read_frags(cur, c + 1, (c + 1) & 1);
            if (c == NC - 1) {
                // every wave has read buffer `cur` and written buffer `cur^1` (chunk 0): swap point.
                if (DBG != 3) __syncthreads();
                if (DBG != 4) read_frags(cur ^ 1, 0, NC & 1);  // first fragments of step g + 1 (maybe the next tile)
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int idx = 0; idx < NM; ++idx) {
                const int s2 = idx / (TM * TN), i = (idx / TN) % TM, j = idx % TN;
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[c & 1][i][s2], bf[c & 1][j][s2], acc[i][j], 0, 0, 0);
                if (c == 0) {
                    // the NS restage slots spread evenly between the MFMAs of chunk 0
                    const int slot_before = (idx * NS) / NM, slot_after = ((idx + 1) * NS) / NM;
                    if (slot_after > slot_before) {
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int q = slot_before; q < slot_after; ++q) restage_slot(q, cur ^ 1, k_ahead);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
            if (c == 0) advance_load_cursor();  // scalar; re-bases the sources once per segment
        }
        cur ^= 1;

        if (++k_c == kend_c) end_segment();
    }
    if constexpr (STAMP) {
        const unsigned long long c3 = __builtin_amdgcn_s_memtime(), r3 = __builtin_amdgcn_s_memrealtime();
        if (tid == 0) {
            unsigned long long *d = p.dbg + (size_t)blockIdx.x * 8;
            d[0] = st0; d[1] = st_loop0; d[2] = st_epi; d[3] = c3; d[4] = WIMG ? st_frag : st_rt0; d[5] = r3;
            d[6] = (unsigned long long)nseg; d[7] = (unsigned long long)steps;
        }
    }
}

// 2 workgroups per CU of the CURRENT device (engines of several devices share the process: nothing is cached process-wide)
static int persistent_wgs() { return 2 * vitdev::current_cus(); }

// K-steps of a last-round tile that a helper workgroup runs (0: the hand-over does not pay) for the persistent walk of bm x bn
// tiles (128 x 128, or the image walk's 64 x 256: 64 KB of accumulators either way) on a grid of `wgs` workgroups (0: ask the
// current device) with `slots` parking slots
// (returned in K-steps of `kstep` deep: PBK for fp32, SPLIT_BK for the split.  The choice and the piece's depth in k are made in
// 32-deep steps for both, so that the split hands over exactly where the fp32 arithmetic does -- QKV at batch 256 included, which
// stays without pieces)
int persistent_piece_steps(int M, int N, int K, int slots, int wgs, int kstep, int bm, int bn) {
    if (wgs <= 0) wgs = persistent_wgs();
    if (wgs <= 0) return 0;
    const int total = ((M + bm - 1) / bm) * ((N + bn - 1) / bn);
    const int nwg = total < wgs ? total : wgs;
    const int full = total / nwg, R = total - full * nwg, nk = K / PBK;
    if (full < 1 || R <= 0 || R >= nwg || R > slots || R > SK_MAX_OWNERS) return 0;
    const int c = (R + (nwg - R) - 1) / (nwg - R);
    const int x = nk / (c + 1);
    // a hand-over costs about 3 K-steps (64 KB out, 64 KB in through uncached memory, the flag): worth it when the walk gets
    // at least 8 steps shorter (measured at batch 256: fc2 -5 %, out_proj -5 % (nk = 24, 8 of 120 saved), fc1 -1.7 %;
    // QKV would save 6 of 336 with six 3-step pieces per helper: off)
    return (x >= 4 && nk - c * x >= 8) ? x * (PBK / kstep) : 0;
}

template <int BM, int BN, int WM, int WN, int ARITH = ARITH_F32, bool WIMG = false>
int launch_persistent_tile(hipStream_t stream, GemmParams &p, int epilogue, int group_m) {
    const int wgs = persistent_wgs();
    if (wgs <= 0) return static_cast<int>(hipErrorInvalidDevice);
    const dim3 grid(set_tile_grid(p, BM, BN, wgs)), block(256);
    p.group_m = group_m;
    // helper pieces (see the head of this file): on when the caller lent a workspace, a partial last round exists and the
    // piece is long enough to be worth a 64 KB hand-over (>= 4 K-steps)
    constexpr int KSTEP = ARITH != ARITH_SPLIT3 ? PBK : (WIMG && BM * 2 == WIMG_ROWS) ? 2 * SPLIT_BK : SPLIT_BK;  // the kernel's K step
    p.sk_x = (p.sk_ws && BM * BN == 128 * 128) ? persistent_piece_steps(p.M, p.N, p.K, p.sk_slots, wgs, KSTEP, BM, BN) : 0;
    return with_epilogue(WalkEpilogues{}, epilogue, [&](auto epi) {
        auto launch = [&](auto sk) {
            hipLaunchKernelGGL((gemm_f32_nt_persistent_kernel<BM, BN, WM, WN, decltype(epi)::value, false, decltype(sk)::value, 0, ARITH, WIMG>), grid, block, 0, stream, p);
            return static_cast<int>(hipGetLastError());
        };
        return p.sk_x > 0 ? launch(std::true_type{}) : launch(std::false_type{});
    });
}

#ifdef VIT_PROBES
// The 128 x 128 walk of the probe instantiations below: no helper pieces
template <int EPI, bool STAMP, int DBG = 0, int ARITH = ARITH_F32, bool WIMG = false>
static int launch_walk_probe(hipStream_t stream, GemmParams &p, int group_m) {
    const int wgs = persistent_wgs();
    if (wgs <= 0) return static_cast<int>(hipErrorInvalidDevice);
    const dim3 grid(set_tile_grid(p, 128, 128, wgs));
    p.group_m = group_m;
    p.sk_x = 0;
    hipLaunchKernelGGL((gemm_f32_nt_persistent_kernel<128, 128, 64, 64, EPI, STAMP, false, DBG, ARITH, WIMG>), grid, dim3(256), 0, stream, p);
    return static_cast<int>(hipGetLastError());
}

// Stamped probe build (tools/gemm_probe.py --stamp-tile 129): p.dbg receives 8 x u64 per workgroup.
// arith = ARITH_SPLIT3 with a weight image (tools/gemm_f32_split_stamps.py): the image walk, word 4 of a record = the summed
// fragment waits of its K steps
int launch_persistent_stamped(hipStream_t stream, GemmParams &p, int epilogue, int group_m, int arith) {
    if (arith == ARITH_SPLIT3) {
        if (!p.w_split) return static_cast<int>(hipErrorInvalidValue);
        return with_epilogue<EPI_BIAS_GELU_LN, EPI_BIAS_LN, VITHIP_EPI_BIAS_RESIDUAL>(epilogue, [&](auto epi) {
            return launch_walk_probe<decltype(epi)::value, true, 0, ARITH_SPLIT3, true>(stream, p, group_m);
        });
    }
    // GELU, the LayerNorm fold's consumer epilogues (tools/gemm_f32_fold_stamps.py); every other code is stamped as the plain bias
    const bool listed = epilogue == VITHIP_EPI_BIAS_GELU || epilogue == EPI_BIAS_GELU_LN || epilogue == EPI_BIAS_LN;
    return with_epilogue<VITHIP_EPI_BIAS, VITHIP_EPI_BIAS_GELU, EPI_BIAS_GELU_LN, EPI_BIAS_LN>(listed ? epilogue : VITHIP_EPI_BIAS, [&](auto epi) {
        return launch_walk_probe<decltype(epi)::value, true>(stream, p, group_m);
    });
}

// Switch-off builds (tools/gemm_f32_switchoff.py; tile codes 131-136 of the probe library): the persistent walk without helper
// pieces and with one part of the kernel removed.  Timing only.
int launch_persistent_switchoff(hipStream_t stream, GemmParams &p, int epilogue, int group_m, int dbg) {
    return with_epilogue<1, 2, 3, 4, 5, 6>(dbg, [&](auto dbg_c) {
        return with_epilogue<VITHIP_EPI_BIAS, VITHIP_EPI_BIAS_GELU, VITHIP_EPI_BIAS_RESIDUAL>(epilogue, [&](auto epi) {
            return launch_walk_probe<decltype(epi)::value, false, decltype(dbg_c)::value>(stream, p, group_m);
        });
    });
}
#endif

// Entry used by vit_gemm.hip's dispatcher.  Needs at least 4 K steps per tile (K >= 128).
// group_m 0: the default grouping of the geometry the walk takes.  128 x 128: see dispatch() in vit_gemm.hip.  64 x 256: the groups
// that cover the same rows and columns of C -- plain N-fastest order up to 4 tile columns (N = 768: the 64 tiles an XCD holds at a
// time are ~21 whole tile rows, the ~11 rows of 128 of before), groups of 8 tile rows of 64 beyond (the 512 rows of 4 x 128).
// geometry (probe build: the override codes 137 / 138): 0 = walk_tile()'s choice, 1 = 128 x 128, 2 = 64 x 256 where it can run.
int launch_persistent(hipStream_t stream, GemmParams &p, int epilogue, int group_m, int arith, int geometry) {
    // residual GEMM whose caller also wants the row statistics of what it stores: in the epilogue when the columns are whole tiles
    if (epilogue == VITHIP_EPI_BIAS_RESIDUAL && p.row_partials && p.N % 128 == 0) {
        epilogue = EPI_RESIDUAL_STATS;
        p.stats_in_epilogue = 1;
    }
    const WalkTile t = walk_tile(p.N, epilogue, arith == ARITH_SPLIT3 && p.w_split != nullptr, geometry);
    if (group_m <= 0) group_m = t.bm == 64 ? (p.N / t.bn <= 4 ? 1 : 8) : ((p.N + 127) / 128 <= 8 ? 1 : 4);
    if (arith == ARITH_SPLIT3) {
        // W's pieces from the caller's pre-split image, or split on the fly: the same bits
        if (p.w_split && t.bm == 64) return launch_persistent_tile<64, 256, 64, 64, ARITH_SPLIT3, true>(stream, p, epilogue, group_m);
        if (p.w_split) return launch_persistent_tile<128, 128, 64, 64, ARITH_SPLIT3, true>(stream, p, epilogue, group_m);
        return launch_persistent_tile<128, 128, 64, 64, ARITH_SPLIT3>(stream, p, epilogue, group_m);
    }
    return launch_persistent_tile<128, 128, 64, 64>(stream, p, epilogue, group_m);
}

}  // namespace vitgemm
