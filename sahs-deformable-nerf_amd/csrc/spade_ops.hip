// spade_ops.hip -- the elementwise core of the Stage-II refiner's SPADE layer (reference
// nerf/_init_spade.py:114-160):   out = act( InstanceNorm2d(x) * (1 + gamma) + beta ),   act = LeakyReLU(slope) of the SPADEBlock that
// follows every SPADE layer (:262-279; slope 1 = none).  The reference runs this as InstanceNorm (a batch-norm kernel), an add, a multiply,
// an add and an activation -- six passes over the (N, C, H, W) tensor; here: two statistics passes (the plane comes from L2 the second
// time) and ONE fused modulate pass.  HBM-bound: 4 B read for the statistics + 12 B read + 4 B written per element = 20 B
// per element (bench.py's `spade` leg reports the achieved GB/s against that).  The 3x3
// convolutions around it (label map -> 128 -> gamma / beta, and the block's spectral-normalised convolutions) are library work and
// stay on MIOpen through PyTorch (hand-written convolutions would buy nothing on this path).
//
// Every kernel is written ONCE, over the element type T of its tensor operands and the group width W (elem_io.hpp): float, or bf16 bit
// patterns in unsigned short (the refiner under torch.autocast: the convolutions hand over bf16 tensors).  The stats / work workspaces
// are fp32 for both, and so is all arithmetic: a loop body loads a group into float v[W] (bf16 widens, exact), works on it, and stores
// from one (bf16 rounds ONCE, to nearest even) -- the bf16 results are the fp32 results of the same operands, rounded, by construction.
// W = ELEM_VEC<T> (4 floats, 8 bf16): one 16-byte access per operand and thread, for hw % W == 0 and 16-byte aligned pointers; W = 1:
// element by element.  bf16 halves the traffic: 10 B per element forward, 8 B read per pass + 6 B written = 22 B backward.
#include <hip/hip_runtime.h>
#include "sahs_common.hpp"
#include "sahs_launchers.hpp"
#include "elem_io.hpp"

namespace sahs {

// Instance statistics in two deterministic passes over (chunk, plane) workgroups -- a workgroup per plane left 3/4 of the chip idle on the
// refiner's 64- and 128-channel maps: pass 0 writes each chunk's sum, pass 1 re-adds the plane's chunk sums in a fixed order (the mean),
// and writes each chunk's sum of squares about it; the modulate pass re-adds those.  part: [planes][SPADE_CHUNKS][2] floats.
constexpr int SPADE_CHUNKS = 8;

__device__ __forceinline__ float block_sum256(float v, float *red)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
// a group's sum, added pairwise: (v0 + v1) + (v2 + v3) for W = 4, two of those for W = 8
template <int W>
__device__ __forceinline__ float pair_sum(const float *v)
{
    if constexpr (W == 1) return v[0];
    else return pair_sum<W / 2>(v) + pair_sum<W / 2>(v + W / 2);
}
__device__ __forceinline__ float plane_mean(const float *part, long hw)
{
    float s = 0.0f;
#pragma unroll
    for (int c = 0; c < SPADE_CHUNKS; ++c) s += part[2 * c];
    return s / (float)hw;
}
// the plane's mean and 1 / sqrt(var + eps) from the statistics workspace
__device__ __forceinline__ void plane_norm(const float *pp, long hw, float eps, float &mean, float &rstd)
{
    mean = plane_mean(pp, hw);
    float var = 0.0f;
#pragma unroll
    for (int c = 0; c < SPADE_CHUNKS; ++c) var += pp[2 * c + 1];
    rstd = 1.0f / sqrtf(var / (float)hw + eps);
}

template <typename T, int W>
__global__ void __launch_bounds__(256) instance_stats_kernel(long hw, const T *__restrict__ x, float *__restrict__ part, int pass)
{
    __shared__ float red[4];
    const long plane = blockIdx.y;
    const T *p = x + plane * hw;
    float *pp = part + plane * (2 * SPADE_CHUNKS);
    const long n = hw / W, per = (n + SPADE_CHUNKS - 1) / SPADE_CHUNKS;
    const long lo = blockIdx.x * per, hi = lo + per < n ? lo + per : n;
    const float mean = pass ? plane_mean(pp, hw) : 0.0f;
    float s = 0.0f;
    for (long i = lo + threadIdx.x; i < hi; i += 256) {
        float q[W];
        elem_load<W>(p, i, q);
        if (pass) {
#pragma unroll
            for (int k = 0; k < W; ++k) { const float d = q[k] - mean; s += d * d; }
        } else {
            s += pair_sum<W>(q);
        }
    }
    s = block_sum256(s, red);
    if (threadIdx.x == 0) pp[2 * blockIdx.x + pass] = s;
}

// one element of the modulation, the same instructions in every kernel that modulates (the build forbids contraction)
__device__ __forceinline__ float spade_element(float x, float mean, float rstd, float gamma, float beta, float slope)
{
    const float v = ((x - mean) * rstd) * (1.0f + gamma) + beta;
    return v > 0.0f ? v : v * slope;
}

// the fused modulate pass: 2-D grid (chunk of the plane, plane) -- the plane index is blockIdx.y, no per-element divide -- and one group
// per operand and thread: fp32 12 B read + 4 B written per element (the statistics pass reads 4 B more)
template <typename T, int W>
__global__ void __launch_bounds__(256) spade_modulate_kernel(long hw, const T *__restrict__ x, const T *__restrict__ gamma,
                                                             const T *__restrict__ beta, const float *__restrict__ stats, float eps, float slope,
                                                             T *__restrict__ out)
{
    const long plane = blockIdx.y, base = plane * hw, n = hw / W;
    float mean, rstd;
    plane_norm(stats + plane * (2 * SPADE_CHUNKS), hw, eps, mean, rstd);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        float xv[W], gv[W], bv[W], o[W];
        elem_load<W>(x + base, i, xv);
        elem_load<W>(gamma + base, i, gv);
        elem_load<W>(beta + base, i, bv);
#pragma unroll
        for (int k = 0; k < W; ++k) o[k] = spade_element(xv[k], mean, rstd, gv[k], bv[k], slope);
        elem_store<W>(out + base, i, o);
    }
}

// ---- the frozen modulation (Stage-II inference: gamma / beta computed once from the identity photo) ----
// Same statistics, same element; what differs is who shares what.  The CHANNEL is on the grid and the batch is a loop in the kernel, so
// (a) a gamma / beta map with a batch of 1 is loaded once per (channel, position) and applied to all B frames -- fp32: 12 + 8 / B bytes
// per element where the per-frame op moves 20 -- and (b) B * C is not bounded by gridDim.y, only C is.  shared = 0: gamma / beta have the
// batch of x and are loaded per frame (the audio-modulated blocks of Generator_audio).
template <typename T, int W>
__global__ void __launch_bounds__(256) spade_modulate_frozen_kernel(long B, long C, int shared, long hw, const T *__restrict__ x,
                                                                    const T *__restrict__ gamma, const T *__restrict__ beta,
                                                                    const float *__restrict__ stats, float eps, float slope, T *__restrict__ out)
{
    const long c = blockIdx.y, n = hw / W;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        float gv[W], bv[W];
        if (shared) {
            elem_load<W>(gamma + c * hw, i, gv);
            elem_load<W>(beta + c * hw, i, bv);
        }
        for (long b = 0; b < B; ++b) {
            const long plane = b * C + c, base = plane * hw;
            float mean, rstd, xv[W], o[W];
            plane_norm(stats + plane * (2 * SPADE_CHUNKS), hw, eps, mean, rstd);
            elem_load<W>(x + base, i, xv);
            if (!shared) {
                elem_load<W>(gamma + base, i, gv);
                elem_load<W>(beta + base, i, bv);
            }
#pragma unroll
            for (int k = 0; k < W; ++k) o[k] = spade_element(xv[k], mean, rstd, gv[k], bv[k], slope);
            elem_store<W>(out + base, i, o);
        }
    }
}

// S elements of a source row: S = ELEM_VEC<T> / 2 is one 8-byte access (2 floats, 4 bf16) for an 8-byte aligned pointer, S = 1 one element
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
template <int S>
__device__ __forceinline__ void half_load(const float *p, long g, float (&v)[S])
{
    if constexpr (S == 1) {
        v[0] = p[g];
    } else {
        static_assert(S == 2);
        const f32x2_t q = reinterpret_cast<const f32x2_t *>(p)[g];
        v[0] = q[0];
        v[1] = q[1];
    }
}
template <int S>
__device__ __forceinline__ void half_load(const unsigned short *p, long g, float (&v)[S])
{
    if constexpr (S == 1) {
        v[0] = bf16_widen(p[g]);
    } else {
        static_assert(S == 4);
        const u32x2_t q = reinterpret_cast<const u32x2_t *>(p)[g];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            v[2 * k] = __builtin_bit_cast(float, q[k] << 16);
            v[2 * k + 1] = __builtin_bit_cast(float, q[k] & 0xffff0000u);
        }
    }
}
// 2 * S elements of an output row from element e on: one 16-byte group for S > 1 (e is a multiple of 2 * S there), two elements for S = 1
template <int S, typename T>
__device__ __forceinline__ void row_load(const T *p, long e, float (&v)[2 * S])
{
    if constexpr (S == 1) {
        float t[1];
        elem_load<1>(p, e, t);
        v[0] = t[0];
        elem_load<1>(p, e + 1, t);
        v[1] = t[0];
    } else {
        elem_load<2 * S>(p, e / (2 * S), v);
    }
}
template <int S, typename T>
__device__ __forceinline__ void row_store(T *p, long e, const float (&v)[2 * S])
{
    if constexpr (S == 1) {
        const float t0[1] = {v[0]}, t1[1] = {v[1]};
        elem_store<1>(p, e, t0);
        elem_store<1>(p, e + 1, t1);
    } else {
        elem_store<2 * S>(p, e / (2 * S), v);
    }
}

// The same with the nearest-neighbour 2x upsample of x read in place: x is (B, C, h, w), gamma / beta / out are (.., C, 2h, 2w), and
// X[i][j] = x[i >> 1][j >> 1] is never written anywhere.  A thread takes S source elements of row r and serves the 2 * S output elements
// above them in rows 2r and 2r + 1.  stats are the SOURCE planes' (every source value occurs four times in X: same mean, same biased
// variance), hw = h * w.  fp32: 1 + 8 / B (shared) + 4 bytes per OUTPUT element, and the statistics passes read a quarter of X.
template <typename T, int S>
__global__ void __launch_bounds__(256) spade_modulate_frozen_up_kernel(long B, long C, int shared, long h, long w, const T *__restrict__ x,
                                                                       const T *__restrict__ gamma, const T *__restrict__ beta,
                                                                       const float *__restrict__ stats, float eps, float slope,
                                                                       T *__restrict__ out)
{
    constexpr int OW = 2 * S;
    const long c = blockIdx.y, gw = w / S, n = h * gw, hw = h * w, ow = 2 * w, ohw = 4 * hw;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (long)gridDim.x * blockDim.x) {
        const long r = p / gw, e0 = 2 * r * ow + (p - r * gw) * OW, e1 = e0 + ow;      // the two output rows' first elements, in the plane
        float g0[OW], g1[OW], b0[OW], b1[OW];
        if (shared) {
            row_load<S>(gamma + c * ohw, e0, g0);
            row_load<S>(gamma + c * ohw, e1, g1);
            row_load<S>(beta + c * ohw, e0, b0);
            row_load<S>(beta + c * ohw, e1, b1);
        }
        for (long b = 0; b < B; ++b) {
            const long plane = b * C + c, obase = plane * ohw;
            float mean, rstd, xv[S], o0[OW], o1[OW];
            plane_norm(stats + plane * (2 * SPADE_CHUNKS), hw, eps, mean, rstd);
            half_load<S>(x + plane * hw, p, xv);      // (rows are whole groups: group p of the plane is group p - r * gw of row r)
            if (!shared) {
                row_load<S>(gamma + obase, e0, g0);
                row_load<S>(gamma + obase, e1, g1);
                row_load<S>(beta + obase, e0, b0);
                row_load<S>(beta + obase, e1, b1);
            }
#pragma unroll
            for (int k = 0; k < OW; ++k) {
                o0[k] = spade_element(xv[k >> 1], mean, rstd, g0[k], b0[k], slope);
                o1[k] = spade_element(xv[k >> 1], mean, rstd, g1[k], b1[k], slope);
            }
            row_store<S>(out + obase, e0, o0);
            row_store<S>(out + obase, e1, o1);
        }
    }
}

// ---- backward of the fused modulation (training of the Stage-II refiner) ----
//   dy = g * (out > 0 ? 1 : slope)     dbeta = dy     dgamma = dy * xh     dxh = dy * (1 + gamma)
//   dx = rstd * (dxh - mean(dxh) - xh * mean(dxh * xh))                     xh = (x - mean) * rstd
// The activation mask is read from the forward's OUTPUT (out > 0 exactly when y > 0 for slope >= 0; at 0 it gives slope, as ATen's
// leaky_relu_backward does), so it is the forward's own whatever the compiler contracted there, and a bf16 output's too (rounding keeps
// the sign); out == nullptr: slope 1, dy = g.
// Two launches shaped like the forward's, no atomics: a sums pass over (chunk, plane) workgroups writes each chunk's sum of dxh and of
// dxh * xh to work[plane][chunk][2], the apply pass re-adds the chunks in order.  fp32: 16 B read per element in each pass, 12 B written.
template <typename T, int W>
__global__ void __launch_bounds__(256) spade_backward_sums_kernel(long hw, const T *__restrict__ x, const T *__restrict__ gamma,
                                                                  const T *__restrict__ out, const float *__restrict__ stats,
                                                                  const T *__restrict__ grad, float eps, float slope, float *__restrict__ work)
{
    __shared__ float red[4];
    const long plane = blockIdx.y, base = plane * hw;
    float mean, rstd;
    plane_norm(stats + plane * (2 * SPADE_CHUNKS), hw, eps, mean, rstd);
    const long n = hw / W, per = (n + SPADE_CHUNKS - 1) / SPADE_CHUNKS;
    const long lo = blockIdx.x * per, hi = lo + per < n ? lo + per : n;
    float s0 = 0.0f, s1 = 0.0f;
    for (long i = lo + threadIdx.x; i < hi; i += 256) {
        float gv[W], xv[W], mv[W], ov[W];
        elem_load<W>(grad + base, i, gv);
        elem_load<W>(x + base, i, xv);
        elem_load<W>(gamma + base, i, mv);
        if (out) elem_load<W>(out + base, i, ov);
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const float dxh = ((!out || ov[k] > 0.0f) ? gv[k] : gv[k] * slope) * (1.0f + mv[k]);
            s0 += dxh;
            s1 += dxh * ((xv[k] - mean) * rstd);
        }
    }
    s0 = block_sum256(s0, red);
    s1 = block_sum256(s1, red);
    if (threadIdx.x == 0) {
        float *wp = work + plane * (2 * SPADE_CHUNKS) + 2 * blockIdx.x;
        wp[0] = s0;
        wp[1] = s1;
    }
}

// dx, dgamma, dbeta: each written where its pointer is not null; work is read only for dx
template <typename T, int W>
__global__ void __launch_bounds__(256) spade_backward_apply_kernel(long hw, const T *__restrict__ x, const T *__restrict__ gamma,
                                                                   const T *__restrict__ out, const float *__restrict__ stats,
                                                                   const T *__restrict__ grad, const float *__restrict__ work, float eps,
                                                                   float slope, T *__restrict__ dx, T *__restrict__ dgamma, T *__restrict__ dbeta)
{
    const long plane = blockIdx.y, base = plane * hw, n = hw / W;
    float mean, rstd;
    plane_norm(stats + plane * (2 * SPADE_CHUNKS), hw, eps, mean, rstd);
    float m0 = 0.0f, m1 = 0.0f;
    if (dx) {
        const float *wp = work + plane * (2 * SPADE_CHUNKS);
#pragma unroll
        for (int c = 0; c < SPADE_CHUNKS; ++c) { m0 += wp[2 * c]; m1 += wp[2 * c + 1]; }
        m0 /= (float)hw;
        m1 /= (float)hw;
    }
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        float gv[W], xv[W], ov[W], mv[W], dy[W], xh[W], o[W];
        elem_load<W>(grad + base, i, gv);
        elem_load<W>(x + base, i, xv);
        if (out) elem_load<W>(out + base, i, ov);
        if (dx) elem_load<W>(gamma + base, i, mv);
#pragma unroll
        for (int k = 0; k < W; ++k) {
            dy[k] = (!out || ov[k] > 0.0f) ? gv[k] : gv[k] * slope;
            xh[k] = (xv[k] - mean) * rstd;
        }
        if (dbeta) elem_store<W>(dbeta + base, i, dy);
        if (dgamma) {
#pragma unroll
            for (int k = 0; k < W; ++k) o[k] = dy[k] * xh[k];
            elem_store<W>(dgamma + base, i, o);
        }
        if (dx) {
#pragma unroll
            for (int k = 0; k < W; ++k) o[k] = rstd * ((dy[k] * (1.0f + mv[k]) - m0) - xh[k] * m1);
            elem_store<W>(dx + base, i, o);
        }
    }
}

// the modulate-shaped grid: a 256-thread workgroup per 256 groups of a plane, capped at ~8 k workgroups in all
static dim3 spade_plane_grid(long per, long planes)
{
    long bx = (per + 255) / 256;
    const long cap = (8192 + planes - 1) / planes;
    if (bx > cap) bx = cap;
    if (bx < 1) bx = 1;
    return dim3((unsigned)bx, (unsigned)planes);
}
// groups of ELEM_VEC<T>: where the plane divides into them and every pointer given is 16-byte aligned (a null one is never dereferenced)
template <typename T, typename... P>
static bool spade_vec(long hw, const P *...p) { return hw % ELEM_VEC<T> == 0 && (((reinterpret_cast<uintptr_t>(p) & 15u) == 0) && ...); }

template <typename T>
static int spade_modulate_launch(long planes, long hw, const T *x, const T *gamma, const T *beta, float eps, float slope, T *out, float *stats,
                                 hipStream_t stream)
{
    if (planes <= 0 || hw <= 0) return 0;
    if (planes > 65535) return -2;      // gridDim.y (capi.hip refuses it by name first)
    constexpr int V = ELEM_VEC<T>;
    const bool vec = spade_vec<T>(hw, x, gamma, beta, out);
    const dim3 sgrid(SPADE_CHUNKS, (unsigned)planes), grid = spade_plane_grid(vec ? hw / V : hw, planes);
    for (int pass = 0; pass < 2; ++pass) {
        if (vec) instance_stats_kernel<T, V><<<sgrid, 256, 0, stream>>>(hw, x, stats, pass);
        else instance_stats_kernel<T, 1><<<sgrid, 256, 0, stream>>>(hw, x, stats, pass);
    }
    if (vec) spade_modulate_kernel<T, V><<<grid, 256, 0, stream>>>(hw, x, gamma, beta, stats, eps, slope, out);
    else spade_modulate_kernel<T, 1><<<grid, 256, 0, stream>>>(hw, x, gamma, beta, stats, eps, slope, out);
    return (int)hipGetLastError();
}

// x: (B, C, h, w); gamma, beta: (shared ? 1 : B, C, H, W); out: (B, C, H, W); (H, W) = (h, w), or (2h, 2w) with up.  The statistics are
// instance_stats_kernel's over the B * C source planes, 65535 (gridDim.y) planes per launch, with the group width the per-frame op
// takes for the same x (up = 0: decided by all four pointers, as there), so mean and rstd are its bits.  Only C rides on gridDim.y.
template <typename T>
static int spade_frozen_launch(long B, long C, int shared, long h, long w, int up, const T *x, const T *gamma, const T *beta, float eps,
                               float slope, T *out, float *stats, hipStream_t stream)
{
    if (B <= 0 || C <= 0 || h <= 0 || w <= 0) return 0;
    if (C > 65535) return -2;      // gridDim.y (capi.hip refuses it by name first)
    constexpr int V = ELEM_VEC<T>;
    const long hw = h * w, planes = B * C;
    const bool aligned8 = (reinterpret_cast<uintptr_t>(x) & 7u) == 0;
    const bool vec = up ? (w % (V / 2) == 0 && aligned8 && spade_vec<T>(V, gamma, beta, out)) : spade_vec<T>(hw, x, gamma, beta, out);
    const bool svec = up ? spade_vec<T>(hw, x) : vec;
    for (long p0 = 0; p0 < planes; p0 += 65535) {
        const dim3 sgrid(SPADE_CHUNKS, (unsigned)(planes - p0 < 65535 ? planes - p0 : 65535));
        for (int pass = 0; pass < 2; ++pass) {
            if (svec) instance_stats_kernel<T, V><<<sgrid, 256, 0, stream>>>(hw, x + p0 * hw, stats + p0 * (2 * SPADE_CHUNKS), pass);
            else instance_stats_kernel<T, 1><<<sgrid, 256, 0, stream>>>(hw, x + p0 * hw, stats + p0 * (2 * SPADE_CHUNKS), pass);
        }
    }
    if (up) {
        const dim3 grid = spade_plane_grid(vec ? h * (w / (V / 2)) : hw, C);
        if (vec) spade_modulate_frozen_up_kernel<T, V / 2><<<grid, 256, 0, stream>>>(B, C, shared, h, w, x, gamma, beta, stats, eps, slope, out);
        else spade_modulate_frozen_up_kernel<T, 1><<<grid, 256, 0, stream>>>(B, C, shared, h, w, x, gamma, beta, stats, eps, slope, out);
    } else {
        const dim3 grid = spade_plane_grid(vec ? hw / V : hw, C);
        if (vec) spade_modulate_frozen_kernel<T, V><<<grid, 256, 0, stream>>>(B, C, shared, hw, x, gamma, beta, stats, eps, slope, out);
        else spade_modulate_frozen_kernel<T, 1><<<grid, 256, 0, stream>>>(B, C, shared, hw, x, gamma, beta, stats, eps, slope, out);
    }
    return (int)hipGetLastError();
}

template <typename T>
static int spade_backward_launch(long planes, long hw, const T *x, const T *gamma, const T *out, const float *stats, const T *grad, float eps,
                                 float slope, T *dx, T *dgamma, T *dbeta, float *work, hipStream_t stream)
{
    if (planes <= 0 || hw <= 0) return 0;
    if (planes > 65535) return -2;      // gridDim.y
    constexpr int V = ELEM_VEC<T>;
    const bool vec = spade_vec<T>(hw, x, gamma, out, grad, dx, dgamma, dbeta);
    const dim3 sgrid(SPADE_CHUNKS, (unsigned)planes), grid = spade_plane_grid(vec ? hw / V : hw, planes);
    if (dx) {
        if (vec) spade_backward_sums_kernel<T, V><<<sgrid, 256, 0, stream>>>(hw, x, gamma, out, stats, grad, eps, slope, work);
        else spade_backward_sums_kernel<T, 1><<<sgrid, 256, 0, stream>>>(hw, x, gamma, out, stats, grad, eps, slope, work);
    }
    if (vec) spade_backward_apply_kernel<T, V><<<grid, 256, 0, stream>>>(hw, x, gamma, out, stats, grad, work, eps, slope, dx, dgamma, dbeta);
    else spade_backward_apply_kernel<T, 1><<<grid, 256, 0, stream>>>(hw, x, gamma, out, stats, grad, work, eps, slope, dx, dgamma, dbeta);
    return (int)hipGetLastError();
}

}  // namespace sahs

extern "C" long sahs_spade_stats_words(long planes) { return planes * 2 * sahs::SPADE_CHUNKS; }

// the tensors are float or, with bf16 set, bf16 bit patterns: same launches, same grids, groups of 8 elements for groups of 4
typedef unsigned short bf;
extern "C" int sahs_spade_modulate_launch(long planes, long hw, const void *x, const void *gamma, const void *beta, float eps, float slope,
                                          void *out, float *stats, int bf16, hipStream_t stream)
{
    if (bf16) return sahs::spade_modulate_launch(planes, hw, (const bf *)x, (const bf *)gamma, (const bf *)beta, eps, slope, (bf *)out, stats, stream);
    return sahs::spade_modulate_launch(planes, hw, (const float *)x, (const float *)gamma, (const float *)beta, eps, slope, (float *)out, stats, stream);
}

extern "C" int sahs_spade_modulate_backward_launch(long planes, long hw, const void *x, const void *gamma, const void *out, const float *stats,
                                                   const void *grad, float eps, float slope, void *dx, void *dgamma, void *dbeta, float *work,
                                                   int bf16, hipStream_t stream)
{
    return bf16 ? sahs::spade_backward_launch(planes, hw, (const bf *)x, (const bf *)gamma, (const bf *)out, stats, (const bf *)grad, eps, slope,
                                              (bf *)dx, (bf *)dgamma, (bf *)dbeta, work, stream)
                : sahs::spade_backward_launch(planes, hw, (const float *)x, (const float *)gamma, (const float *)out, stats, (const float *)grad, eps,
                                              slope, (float *)dx, (float *)dgamma, (float *)dbeta, work, stream);
}

extern "C" int sahs_spade_modulate_frozen_launch(long batch, long channels, int shared, long h, long w, int up, const void *x, const void *gamma,
                                                 const void *beta, float eps, float slope, void *out, float *stats, int bf16, hipStream_t stream)
{
    if (bf16) return sahs::spade_frozen_launch(batch, channels, shared, h, w, up, (const bf *)x, (const bf *)gamma, (const bf *)beta, eps, slope,
                                               (bf *)out, stats, stream);
    return sahs::spade_frozen_launch(batch, channels, shared, h, w, up, (const float *)x, (const float *)gamma, (const float *)beta, eps, slope,
                                     (float *)out, stats, stream);
}
