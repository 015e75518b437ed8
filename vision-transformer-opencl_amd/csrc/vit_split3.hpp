// csrc/vit_split3.hpp -- the three-piece split of an fp32 value into bf16 pieces: the one definition of the pieces and of the order
// their products are added in.  Used by the split GEMMs (vit_gemm_common.hpp, vit_split_weights.hip) and by the split attention
// kernel (vit_attention_hd.hip).  DESIGN 4.1.1.
//
//     hi = bf16(x),  mid = bf16(x - hi),  lo = bf16(x - hi - mid),   x == hi + mid + lo exactly
// Each piece is rounded to nearest even; both differences are exact in fp32 and the last remainder has at most 8 significant bits.
// +-Inf and NaN stay in hi.
#pragma once
#include <hip/hip_runtime.h>

namespace vitsplit {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

// piece pairs (A piece, W piece) in accumulation order, small terms first; 0 = hi, 1 = mid, 2 = lo
constexpr int SPLIT_TERM_A[6] = {0, 2, 1, 0, 1, 0};
constexpr int SPLIT_TERM_W[6] = {2, 0, 1, 1, 0, 0};

__device__ __forceinline__ float bf16_to_f32(__bf16 v) {
    return __builtin_bit_cast(float, (unsigned)__builtin_bit_cast(unsigned short, v) << 16);
}
// piece `piece` (0 = hi, 1 = mid, 2 = lo) of four values, taken in this order: x holds what the earlier pieces left of the values
// and, for pieces 0 and 1, is left holding the remainder for the next one.  The one definition of the pieces: the on-the-fly split
// of both GEMM operands, the image walk's split of A, the weight-image producer (vit_split_weights.hip) and the attention kernel's
// split of Q, K, V and P all make them here.
__device__ __forceinline__ u32x2 split3_piece(f32x4 &x, int piece) {
    bf16x4 b;
#pragma unroll
    for (int e = 0; e < 4; ++e) b[e] = (__bf16)x[e];  // v_cvt_pk_bf16_f32: round to nearest even
    if (piece < 2) {
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = x[e] - bf16_to_f32(b[e]);  // exact
    }
    return __builtin_bit_cast(u32x2, b);
}
// the same for eight consecutive k (x0 = k 0..3, x1 = k 4..7): piece `piece` of all eight as one 16-byte plane chunk
__device__ __forceinline__ u32x4 split3_piece8(f32x4 &x0, f32x4 &x1, int piece) {
    const u32x2 p0 = split3_piece(x0, piece), p1 = split3_piece(x1, piece);
    return u32x4{p0[0], p0[1], p1[0], p1[1]};
}
// piece `piece` of two values, value by value the arithmetic of split3_piece: a quarter of a plane chunk, for the image walk's
// finer restage slots
__device__ __forceinline__ unsigned split3_piece2(f32x2 &x, int piece) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    bf16x2 b;
#pragma unroll
    for (int e = 0; e < 2; ++e) b[e] = (__bf16)x[e];
    if (piece < 2) x = x - f32x2{bf16_to_f32(b[0]), bf16_to_f32(b[1])};  // exact
    return __builtin_bit_cast(unsigned, b);
}

}  // namespace vitsplit
