// bf16_io.hpp -- bf16 tensors as bit patterns (unsigned short) at the edge of fp32 arithmetic: widened on load (exact), rounded to
// nearest even ONCE on store.  Shared by the streaming kernels with bf16 operands (spade_ops.hip, spectral_norm.hip).
// W = 8: one 16-byte access (8 bf16) per thread, for a 16-byte aligned pointer; W = 1: element by element.
#pragma once
#include <hip/hip_runtime.h>

namespace sahs {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float bf16_widen(unsigned bits) { return __builtin_bit_cast(float, bits << 16); }
__device__ __forceinline__ unsigned bf16_round(float f) { return __builtin_bit_cast(unsigned short, (__bf16)f); }      // as pack.hip: f32_to_bf16_rne

// group i (W elements) of a plane that starts at p
template <int W>
__device__ __forceinline__ void bf16_load(const unsigned short *p, long i, float (&v)[W])
{
    if constexpr (W == 8) {
        const u32x4 q = reinterpret_cast<const u32x4 *>(p)[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[2 * k] = __builtin_bit_cast(float, q[k] << 16);
            v[2 * k + 1] = __builtin_bit_cast(float, q[k] & 0xffff0000u);
        }
    } else {
        v[0] = bf16_widen(p[i]);
    }
}
template <int W>
__device__ __forceinline__ void bf16_store(unsigned short *p, long i, const float (&v)[W])
{
    if constexpr (W == 8) {
        u32x4 q;
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = bf16_round(v[2 * k]) | bf16_round(v[2 * k + 1]) << 16;
        reinterpret_cast<u32x4 *>(p)[i] = q;
    } else {
        p[i] = (unsigned short)bf16_round(v[0]);
    }
}

}  // namespace sahs
