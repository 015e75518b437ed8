// csrc/vit_rope.hip -- rotary position embedding on the Q and K columns of the patch rows of a qkv buffer, in place
// (include/vit_hip_kernels.h, "Rotary position embedding"; DINOv3's apply_rotary_pos_emb).
//
// For every patch row, every head and every j < hd/2, with x1 = v[j], x2 = v[j + hd/2] and the row's table entries c, s:
//     v[j] = x1 c - x2 s        v[j + hd/2] = x2 c + x1 s
// 8 flops against 16 bytes of traffic per pair (fp32): the pass is HBM-bound, and what it must not do is read the table per element.
//   * a workgroup owns ONE patch position p and a slice of the images.  Position p has one table row for every head of every image,
//     for Q and for K: a lane loads its 4 cos and 4 sin values once (two 16-byte loads), keeps them in 8 registers and walks the
//     rows p of its images, T * ld elements apart.  The table is read once per workgroup; the walk reads and writes qkv only;
//   * the lanes cover the slots (Q | K, head, group of 4 of the head's lower half) of one token row, the group fastest: a slot is
//     the 4 elements of the lower half and the matching 4 of the upper half, one 16-byte (bf16: 8-byte) load and store each.  The
//     lanes of a head read its lower half as one run and its upper half as the run behind it, so every cache line of the Q and K
//     columns is moved whole, once in and once out;
//   * ROPE_TRIP images are in flight per lane: 2 * ROPE_TRIP loads are issued before the first fma and the first store;
//   * the grid is (P, slices): the launcher cuts the image range so that a small grid of patches still fills the device (rope_slices);
//   * no LDS, no atomics, no barrier: a lane shares nothing.  In place is safe because a lane reads both halves of its slot before
//     it stores and no other lane touches them.
// Built without packed fp32 pairs (Makefile): every product and fma below is the one-value VALU form.
#include <hip/hip_runtime.h>

#include "vit_hip_kernels.h"

namespace {

constexpr int ROPE_TRIP = 4;            // images in flight per lane
constexpr int ROPE_MAX_THREADS = 512;   // the slots of a row up to D = 2048 (Q and K) in one pass; wider rows take several
constexpr int ROPE_TARGET_BLOCKS = 2048;  // 8 workgroups per compute unit of a 256-CU device

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

template <typename T> struct rope_vec;
template <> struct rope_vec<float> { using type = f32x4; };
template <> struct rope_vec<unsigned short> { using type = u32x2; };

// 4 elements -> fp32 (bf16 -> fp32 is exact: the bits move to the upper half) and back (one rounding to nearest even)
__device__ __forceinline__ void widen(const f32x4 &p, float (&o)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = p[i];
}
__device__ __forceinline__ void widen(const u32x2 &p, float (&o)[4]) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        o[2 * i] = __builtin_bit_cast(float, p[i] << 16);
        o[2 * i + 1] = __builtin_bit_cast(float, p[i] & 0xffff0000u);
    }
}
__device__ __forceinline__ void narrow(const float (&x)[4], f32x4 &r) { r = f32x4{x[0], x[1], x[2], x[3]}; }
__device__ __forceinline__ void narrow(const float (&x)[4], u32x2 &r) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const bf16x2 b = bf16x2{(__bf16)x[2 * i], (__bf16)x[2 * i + 1]};  // v_cvt_pk_bf16_f32: round to nearest even
        r[i] = __builtin_bit_cast(unsigned, b);
    }
}

// qkv points at the first rotated column of row 0 of image 0 (Q, or K under VITHIP_ROPE_K); slots = segs * heads * (hd / 8).
// blockIdx.x = patch position, blockIdx.y = image slice of `per` images.
template <typename T>
__global__ __launch_bounds__(ROPE_MAX_THREADS) void rope_kernel(T *qkv, size_t ld, size_t image_stride, const float *cos_t,
                                                                const float *sin_t, int n_images, int per, int prefix, int heads, int hd,
                                                                int slots) {
    using V = typename rope_vec<T>::type;
    const int p = blockIdx.x, half = hd >> 1, groups = hd >> 3, per_seg = heads * groups;
    const int first = blockIdx.y * per, last = min(first + per, n_images);
    for (int slot = threadIdx.x; slot < slots; slot += blockDim.x) {
        const int seg = slot / per_seg, rem = slot - seg * per_seg, head = rem / groups, g = rem - head * groups;
        const f32x4 c = *reinterpret_cast<const f32x4 *>(cos_t + (size_t)p * half + 4 * g);
        const f32x4 s = *reinterpret_cast<const f32x4 *>(sin_t + (size_t)p * half + 4 * g);
        // the lower group of the slot in row prefix + p of image `first`; seg 1 = the same columns of K, heads * hd further on
        T *at = qkv + ((size_t)first * image_stride + (size_t)(prefix + p) * ld) + (size_t)seg * heads * hd + (size_t)head * hd + 4 * g;
        for (int img = first; img < last; img += ROPE_TRIP) {
            V lo[ROPE_TRIP], hi[ROPE_TRIP];
#pragma unroll
            for (int k = 0; k < ROPE_TRIP; ++k) {
                lo[k] = V{}; hi[k] = V{};
                if (img + k < last) {
                    lo[k] = *reinterpret_cast<const V *>(at + (size_t)k * image_stride);
                    hi[k] = *reinterpret_cast<const V *>(at + (size_t)k * image_stride + half);
                }
            }
#pragma unroll
            for (int k = 0; k < ROPE_TRIP; ++k) {
                float x1[4], x2[4], y1[4], y2[4];
                widen(lo[k], x1);
                widen(hi[k], x2);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    y1[i] = __builtin_fmaf(-x2[i], s[i], x1[i] * c[i]);
                    y2[i] = __builtin_fmaf(x1[i], s[i], x2[i] * c[i]);
                }
                if (img + k < last) {
                    V o1, o2;
                    narrow(y1, o1);
                    narrow(y2, o2);
                    __builtin_nontemporal_store(o1, reinterpret_cast<V *>(at + (size_t)k * image_stride));
                    __builtin_nontemporal_store(o2, reinterpret_cast<V *>(at + (size_t)k * image_stride + half));
                }
            }
            at += (size_t)ROPE_TRIP * image_stride;
        }
    }
}

// Image slices for P patch positions and n images: as many as bring the grid to ROPE_TARGET_BLOCKS workgroups, never more than the
// images; then evened out, so that no slice is empty and the last one is the only short one.  Returns images per slice.
int rope_slices(int n, int P, int *slices) {
    int want = (ROPE_TARGET_BLOCKS + P - 1) / P;
    if (want > n) want = n;
    const int per = (n + want - 1) / want;
    *slices = (n + per - 1) / per;
    return per;
}

template <typename T>
int rope_dispatch(vithip_stream_t stream, T *qkv, size_t ld, const float *cos_t, const float *sin_t, int n_images, int tokens,
                  int prefix, int heads, int head_dim, int which) {
    const int inv = static_cast<int>(hipErrorInvalidValue);
    if (!qkv || !cos_t || !sin_t || n_images < 1 || tokens < 1 || prefix < 0 || prefix >= tokens || heads < 1) return inv;
    if (which != VITHIP_ROPE_QK && which != VITHIP_ROPE_K) return inv;
    if (vithip_qscale(head_dim) == 0.0f) return inv;  // what the attention kernels take: 64, or a multiple of 8 from 72 to 128
    if (heads > (1 << 20) / head_dim) return inv;     // slots and column offsets stay far inside an int
    const size_t D = (size_t)heads * head_dim;
    // 4-element accesses: 16 bytes of fp32, 8 bytes of bf16; the table rows are hd/2 floats, a multiple of 4
    if (ld < 3 * D || ld % 4 || (reinterpret_cast<size_t>(qkv) & (4 * sizeof(T) - 1))) return inv;
    if ((reinterpret_cast<size_t>(cos_t) & 15) || (reinterpret_cast<size_t>(sin_t) & 15)) return inv;
    const int P = tokens - prefix, segs = which == VITHIP_ROPE_QK ? 2 : 1;
    const int slots = segs * heads * (head_dim / 8);
    int slices = 0;
    const int per = rope_slices(n_images, P, &slices);
    if (slices > 65535) return inv;  // cannot happen: slices <= ROPE_TARGET_BLOCKS
    const int threads = slots < ROPE_MAX_THREADS ? (slots + 63) / 64 * 64 : ROPE_MAX_THREADS;
    T *base = which == VITHIP_ROPE_QK ? qkv : qkv + D;
    hipLaunchKernelGGL((rope_kernel<T>), dim3(P, slices), dim3(threads), 0, static_cast<hipStream_t>(stream), base, ld,
                       (size_t)tokens * ld, cos_t, sin_t, n_images, per, prefix, heads, head_dim, slots);
    return static_cast<int>(hipGetLastError());
}

}  // namespace

extern "C" {

int vithip_rope_f32(vithip_stream_t stream, float *qkv, size_t ld, const float *cos_t, const float *sin_t, int n_images, int tokens,
                    int prefix, int heads, int head_dim, int which) {
    return rope_dispatch<float>(stream, qkv, ld, cos_t, sin_t, n_images, tokens, prefix, heads, head_dim, which);
}

int vithip_rope_bf16(vithip_stream_t stream, unsigned short *qkv, size_t ld, const float *cos_t, const float *sin_t, int n_images,
                     int tokens, int prefix, int heads, int head_dim, int which) {
    return rope_dispatch<unsigned short>(stream, qkv, ld, cos_t, sin_t, n_images, tokens, prefix, heads, head_dim, which);
}

}  // extern "C"
