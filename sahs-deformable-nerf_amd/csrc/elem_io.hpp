// elem_io.hpp -- the tensor operands of the streaming kernels (spade_ops.hip, spectral_norm.hip) at the edge of fp32 arithmetic: a group
// of elements is loaded into a float array, worked on in fp32 and stored from one, whatever the element type.  float: as it is.  bf16:
// bit patterns (unsigned short), widened on load (exact), rounded to nearest even ONCE on store.  elem_load / elem_store pick by the
// pointer's type, so a kernel body is written once for both; ELEM_VEC<T> elements make one 16-byte access per thread, for a 16-byte
// aligned pointer; a group of 1 goes element by element.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include "sahs_common.hpp"

namespace sahs {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

template <typename T> constexpr int ELEM_VEC = 16 / sizeof(T);      // 4 floats, 8 bf16
template <bool BF16> using elem_of = std::conditional_t<BF16, unsigned short, float>;      // (for a void pointer that travels with a bf16 flag)

__device__ __forceinline__ float bf16_widen(unsigned bits) { return __builtin_bit_cast(float, bits << 16); }
__device__ __forceinline__ unsigned bf16_round(float f) { return __builtin_bit_cast(unsigned short, (__bf16)f); }      // as pack.hip: f32_to_bf16_rne

// group i (W = 8 or 1 elements) of a plane that starts at p
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

// group g (N = 1 or a multiple of 4 floats) of the floats at p
template <int N>
__device__ __forceinline__ void f32_load(const float *p, long g, float (&v)[N])
{
    if constexpr (N == 1) {
        v[0] = p[g];
    } else {
#pragma unroll
        for (int q = 0; q < N / 4; ++q) {
            const f32x4 x = reinterpret_cast<const f32x4 *>(p)[g * (N / 4) + q];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[4 * q + k] = x[k];
        }
    }
}
template <int N>
__device__ __forceinline__ void f32_store(float *p, long g, const float (&v)[N])
{
    if constexpr (N == 1) {
        p[g] = v[0];
    } else {
#pragma unroll
        for (int q = 0; q < N / 4; ++q) {
            f32x4 x;
#pragma unroll
            for (int k = 0; k < 4; ++k) x[k] = v[4 * q + k];
            reinterpret_cast<f32x4 *>(p)[g * (N / 4) + q] = x;
        }
    }
}

template <int W> __device__ __forceinline__ void elem_load(const float *p, long i, float (&v)[W]) { f32_load<W>(p, i, v); }
template <int W> __device__ __forceinline__ void elem_load(const unsigned short *p, long i, float (&v)[W]) { bf16_load<W>(p, i, v); }
template <int W> __device__ __forceinline__ void elem_store(float *p, long i, const float (&v)[W]) { f32_store<W>(p, i, v); }
template <int W> __device__ __forceinline__ void elem_store(unsigned short *p, long i, const float (&v)[W]) { bf16_store<W>(p, i, v); }

}  // namespace sahs
