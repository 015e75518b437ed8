// csrc/vit_attention.hpp -- what the attention files share (vit_attention.hip, _resident, _stream, _hd, vit_cls_attention.hip):
// the vector types, the transposing V read, the head_dim 64 exponent factor, the entries' argument checks, the integer-to-template
// dispatch and the functions one file exports to another.  Which kernel runs for which arguments: the head of vit_attention.hip.
//
// Not here, because one file alone uses them: load4 / store4 (vit_attention.hip), the 16-byte piece loader Piece (vit_cls_attention.hip,
// the one class-row kernel), max_halves (vit_attention_stream.hip), Geo (vit_attention_hd.hip).
#ifndef VIT_ATTENTION_HPP
#define VIT_ATTENTION_HPP

#include <hip/hip_runtime.h>

#include <type_traits>

#include "vit_hip_kernels.h"

namespace vitattn {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned short bf16_t;  // raw bf16 bits: qkv and the output of the bf16 variant (scores, softmax and accumulation stay fp32)
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef short short4v __attribute__((ext_vector_type(4)));
typedef short short8v __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) short4v lds_short4v;
typedef __attribute__((address_space(3))) void lds_void;

// (1 / sqrtf(64)) * log2(e): softmax(q.k / 8) = exp2(kScale64 * s - kScale64 * max) / sum.  The factor the engine folds into Q.
constexpr float kScale64 = 0.125f * 1.4426950408889634f;
static_assert(kScale64 == VITHIP_QSCALE, "the kernels' factor and the one the engine folds into the Q rows are the same bits");

// A fragment of O^T = V^T . P^T for d-tile dt and the 16 keys starting at key16 (a multiple of 16), in the key order of the P
// fragment: element j of lane half h is key key16 + 8(j>>2) + 4h + (j&3).  Vs: [keys][LD] bf16, the 16-byte chunk c of row k at
// c ^ 4*((k>>1)&1).  Per 16-lane group gfx950's transposing read takes a block of 4 keys x 16 d: lane 4q+p of the group supplies the
// address of key row q, d columns 4p..4p+3, lane i receives column i.  EXEC must be all ones (wave-uniform callers).
template <int LD>
__device__ __forceinline__ bf16x8 v_fragment_tr(const bf16_t *Vs, int key16, int dt, int lane) {
    const int h = lane >> 5, g2 = (lane >> 4) & 1, q = (lane & 15) >> 2, pq = lane & 3;
    const int row = key16 + 4 * h + q;                     // (row >> 1) & 1 == (q >> 1) & 1: key16 + 4h is a multiple of 4
    const int chunk = (dt * 4 + 2 * g2 + (pq >> 1)) ^ (4 * ((q >> 1) & 1));
    const bf16_t *ptr = Vs + row * LD + chunk * 8 + 4 * (pq & 1);
    const short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4v *)ptr);
    const short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4v *)(ptr + 8 * LD));
    const short8v both = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(bf16x8, both);
}

// ---- host side ----

// What every P.V entry asks of its arguments, whichever kernel then runs: both pointers there and 16-byte aligned, sizes positive.
static inline bool qkv_args_ok(const void *qkv, const void *out, int n_images, int tokens, int heads, int q_rows) {
    const size_t low_bits = (reinterpret_cast<size_t>(qkv) | reinterpret_cast<size_t>(out)) & 15;
    return qkv && out && !low_bits && n_images > 0 && tokens > 0 && heads > 0 && q_rows > 0 && q_rows <= tokens;
}

// The head dims the attention entries take: 64, and every multiple of 8 from 72 to 128.
static inline bool hd_accepted(int head_dim) { return head_dim == 64 || (head_dim >= 72 && head_dim <= 128 && head_dim % 8 == 0); }

// f(std::integral_constant<int, N>) for the N among FIRST, FIRST + STEP, ... (COUNT of them) that equals n; hipErrorInvalidValue for
// an n that is none of them.  Every N is instantiated.
template <int FIRST, int COUNT, int STEP = 1, typename F>
static inline int dispatch_int(int n, F &&f) {
    if constexpr (COUNT == 0) {
        return static_cast<int>(hipErrorInvalidValue);
    } else {
        if (n == FIRST) return f(std::integral_constant<int, FIRST>{});
        return dispatch_int<FIRST + STEP, COUNT - 1, STEP>(n, f);
    }
}

// ---- what one attention file exports to another; every one returns a hipError_t value ----

// vit_attention_resident.hip: fp32, head_dim 64, tokens <= 224, q_rows <= tokens
int attention_f32_resident(hipStream_t s, const float *qkv, float *out, int n_images, int tokens, int heads, int q_rows);
// vit_attention_stream.hip: bf16, head_dim 64, 128 < tokens <= 704, every query row
int attention_bf16_stream(hipStream_t s, const unsigned short *qkv, unsigned short *out, int n_images, int tokens, int heads, bool q_scaled);
// vit_attention_hd.hip: head_dim 72..128 in steps of 8, any tokens; heads <= 65535 and the grid fits (this route's own limits).
// Hidden: the library's exported names stay the ones it had.
__attribute__((visibility("hidden"))) int attention_hd_f32(hipStream_t s, const float *qkv, float *out, int n_images, int tokens,
                                                           int heads, int head_dim, int q_rows);
__attribute__((visibility("hidden"))) int attention_hd_bf16(hipStream_t s, const unsigned short *qkv, unsigned short *out, int n_images,
                                                            int tokens, int heads, int head_dim, int q_rows, bool q_scaled);
// vit_attention_hd.hip: fp32, head_dim 64, any tokens, on the bf16 matrix pipe (three-piece split); the same two limits
__attribute__((visibility("hidden"))) int attention_split_f32(hipStream_t s, const float *qkv, float *out, int n_images, int tokens,
                                                              int heads, int q_rows);

#ifdef VIT_PROBES  // the probe build's globals, set by vithip_attention_set_debug_buffer / _set_probe_mode (vit_attention.hip)
extern unsigned long long *g_res_dbg;     // vit_attention_resident.hip
extern int g_res_mode;                    // vit_attention_resident.hip
extern unsigned long long *g_stream_dbg;  // vit_attention_stream.hip
#endif

}  // namespace vitattn

#endif  // VIT_ATTENTION_HPP
