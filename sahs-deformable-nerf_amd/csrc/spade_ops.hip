// spade_ops.hip -- the elementwise core of the Stage-II refiner's SPADE layer (reference
// nerf/_init_spade.py:114-160):   out = act( InstanceNorm2d(x) * (1 + gamma) + beta ),   act = LeakyReLU(slope) of the SPADEBlock that
// follows every SPADE layer (:262-279; slope 1 = none).  The reference runs this as InstanceNorm (a batch-norm kernel), an add, a multiply,
// an add and an activation -- six passes over the (N, C, H, W) tensor; here: two statistics passes (the plane comes from L2 the second
// time) and ONE fused modulate pass.  HBM-bound: 4 B read for the statistics + 12 B read + 4 B written per element = 20 B
// per element (bench.py's `spade` leg reports the achieved GB/s against that).  The 3x3
// convolutions around it (label map -> 128 -> gamma / beta, and the block's spectral-normalised convolutions) are library work and
// stay on MIOpen through PyTorch (hand-written convolutions would buy nothing on this path).
#include <hip/hip_runtime.h>
#include "sahs_common.hpp"
#include "sahs_launchers.hpp"
#include "bf16_io.hpp"

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
__device__ __forceinline__ float plane_mean(const float *part, long hw)
{
    float s = 0.0f;
#pragma unroll
    for (int c = 0; c < SPADE_CHUNKS; ++c) s += part[2 * c];
    return s / (float)hw;
}

template <bool VEC>
__global__ void __launch_bounds__(256) instance_stats_kernel(long hw, const float *__restrict__ x, float *__restrict__ part, int pass)
{
    __shared__ float red[4];
    const long plane = blockIdx.y;
    const float *p = x + plane * hw;
    float *pp = part + plane * (2 * SPADE_CHUNKS);
    const long n = VEC ? hw / 4 : hw, per = (n + SPADE_CHUNKS - 1) / SPADE_CHUNKS;
    const long lo = blockIdx.x * per, hi = lo + per < n ? lo + per : n;
    const float mean = pass ? plane_mean(pp, hw) : 0.0f;
    float s = 0.0f;
    for (long i = lo + threadIdx.x; i < hi; i += 256) {
        if (VEC) {
            const f32x4 q = reinterpret_cast<const f32x4 *>(p)[i];
            if (pass) {
#pragma unroll
                for (int k = 0; k < 4; ++k) { const float d = q[k] - mean; s += d * d; }
            } else {
                s += (q[0] + q[1]) + (q[2] + q[3]);
            }
        } else {
            const float d = p[i] - mean;
            s += pass ? d * d : p[i];
        }
    }
    s = block_sum256(s, red);
    if (threadIdx.x == 0) pp[2 * blockIdx.x + pass] = s;
}

// the fused modulate pass: 2-D grid (chunk of the plane, plane) -- the plane index is blockIdx.y, no per-element divide -- and one 16-byte
// load per operand and thread where the plane allows it: 12 B read + 4 B written per element (the statistics pass reads 4 B more)
template <bool VEC>
__global__ void __launch_bounds__(256) spade_modulate_kernel(long hw, const float *__restrict__ x, const float *__restrict__ gamma,
                                                             const float *__restrict__ beta, const float *__restrict__ stats, float eps, float slope,
                                                             float *__restrict__ out)
{
    const long plane = blockIdx.y, base = plane * hw;
    const float *pp = stats + plane * (2 * SPADE_CHUNKS);
    const float mean = plane_mean(pp, hw);
    float var = 0.0f;
#pragma unroll
    for (int c = 0; c < SPADE_CHUNKS; ++c) var += pp[2 * c + 1];
    const float rstd = 1.0f / sqrtf(var / (float)hw + eps);
    if (VEC) {
        const long n4 = hw >> 2;
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
            const f32x4 xv = reinterpret_cast<const f32x4 *>(x + base)[i], gv = reinterpret_cast<const f32x4 *>(gamma + base)[i],
                        bv = reinterpret_cast<const f32x4 *>(beta + base)[i];
            f32x4 o;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float v = ((xv[k] - mean) * rstd) * (1.0f + gv[k]) + bv[k];
                o[k] = v > 0.0f ? v : v * slope;
            }
            reinterpret_cast<f32x4 *>(out + base)[i] = o;
        }
    } else {
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += (long)gridDim.x * blockDim.x) {
            const float v = ((x[base + i] - mean) * rstd) * (1.0f + gamma[base + i]) + beta[base + i];
            out[base + i] = v > 0.0f ? v : v * slope;
        }
    }
}

// ---- backward of the fused modulation (training of the Stage-II refiner) ----
//   dy = g * (out > 0 ? 1 : slope)     dbeta = dy     dgamma = dy * xh     dxh = dy * (1 + gamma)
//   dx = rstd * (dxh - mean(dxh) - xh * mean(dxh * xh))                     xh = (x - mean) * rstd
// The activation mask is read from the forward's OUTPUT (out > 0 exactly when y > 0 for slope >= 0; at 0 it gives slope, as ATen's
// leaky_relu_backward does), so it is the forward's own whatever the compiler contracted there; out == nullptr: slope 1, dy = g.
// Two launches shaped like the forward's, no atomics: a sums pass over (chunk, plane) workgroups writes each chunk's sum of dxh and of
// dxh * xh to work[plane][chunk][2], the apply pass re-adds the chunks in order.  16 B read per element in each pass, 12 B written.

// the plane's mean and 1 / sqrt(var + eps) from the forward's statistics workspace, formed as spade_modulate_kernel forms them
__device__ __forceinline__ void plane_norm(const float *pp, long hw, float eps, float &mean, float &rstd)
{
    mean = plane_mean(pp, hw);
    float var = 0.0f;
#pragma unroll
    for (int c = 0; c < SPADE_CHUNKS; ++c) var += pp[2 * c + 1];
    rstd = 1.0f / sqrtf(var / (float)hw + eps);
}

template <bool VEC>
__global__ void __launch_bounds__(256) spade_backward_sums_kernel(long hw, const float *__restrict__ x, const float *__restrict__ gamma,
                                                                  const float *__restrict__ out, const float *__restrict__ stats,
                                                                  const float *__restrict__ grad, float eps, float slope,
                                                                  float *__restrict__ work)
{
    __shared__ float red[4];
    const long plane = blockIdx.y, base = plane * hw;
    float mean, rstd;
    plane_norm(stats + plane * (2 * SPADE_CHUNKS), hw, eps, mean, rstd);
    const long n = VEC ? hw / 4 : hw, per = (n + SPADE_CHUNKS - 1) / SPADE_CHUNKS;
    const long lo = blockIdx.x * per, hi = lo + per < n ? lo + per : n;
    float s0 = 0.0f, s1 = 0.0f;
    for (long i = lo + threadIdx.x; i < hi; i += 256) {
        if (VEC) {
            const f32x4 gv = reinterpret_cast<const f32x4 *>(grad + base)[i], xv = reinterpret_cast<const f32x4 *>(x + base)[i],
                        mv = reinterpret_cast<const f32x4 *>(gamma + base)[i];
            f32x4 ov = {1.0f, 1.0f, 1.0f, 1.0f};
            if (out) ov = reinterpret_cast<const f32x4 *>(out + base)[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float dxh = (ov[k] > 0.0f ? gv[k] : gv[k] * slope) * (1.0f + mv[k]);
                s0 += dxh;
                s1 += dxh * ((xv[k] - mean) * rstd);
            }
        } else {
            const float g = grad[base + i], dy = (!out || out[base + i] > 0.0f) ? g : g * slope;
            const float dxh = dy * (1.0f + gamma[base + i]);
            s0 += dxh;
            s1 += dxh * ((x[base + i] - mean) * rstd);
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
template <bool VEC>
__global__ void __launch_bounds__(256) spade_backward_apply_kernel(long hw, const float *__restrict__ x, const float *__restrict__ gamma,
                                                                   const float *__restrict__ out, const float *__restrict__ stats,
                                                                   const float *__restrict__ grad, const float *__restrict__ work, float eps,
                                                                   float slope, float *__restrict__ dx, float *__restrict__ dgamma,
                                                                   float *__restrict__ dbeta)
{
    const long plane = blockIdx.y, base = plane * hw;
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
    if (VEC) {
        const long n4 = hw >> 2;
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
            const f32x4 gv = reinterpret_cast<const f32x4 *>(grad + base)[i], xv = reinterpret_cast<const f32x4 *>(x + base)[i];
            f32x4 ov = {1.0f, 1.0f, 1.0f, 1.0f}, mv = {0.0f, 0.0f, 0.0f, 0.0f}, dy, xh;
            if (out) ov = reinterpret_cast<const f32x4 *>(out + base)[i];
            if (dx) mv = reinterpret_cast<const f32x4 *>(gamma + base)[i];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                dy[k] = ov[k] > 0.0f ? gv[k] : gv[k] * slope;
                xh[k] = (xv[k] - mean) * rstd;
            }
            if (dbeta) reinterpret_cast<f32x4 *>(dbeta + base)[i] = dy;
            if (dgamma) {
                f32x4 o;
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = dy[k] * xh[k];
                reinterpret_cast<f32x4 *>(dgamma + base)[i] = o;
            }
            if (dx) {
                f32x4 o;
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = rstd * ((dy[k] * (1.0f + mv[k]) - m0) - xh[k] * m1);
                reinterpret_cast<f32x4 *>(dx + base)[i] = o;
            }
        }
    } else {
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < hw; i += (long)gridDim.x * blockDim.x) {
            const float g = grad[base + i], dy = (!out || out[base + i] > 0.0f) ? g : g * slope;
            const float xh = (x[base + i] - mean) * rstd;
            if (dbeta) dbeta[base + i] = dy;
            if (dgamma) dgamma[base + i] = dy * xh;
            if (dx) dx[base + i] = rstd * ((dy * (1.0f + gamma[base + i]) - m0) - xh * m1);
        }
    }
}

// ---- bf16 I/O forms of the four kernels above (the refiner under torch.autocast: the convolutions hand over bf16 tensors) ----
// Every tensor operand is bf16 (bit patterns in unsigned short); the stats / work workspaces stay fp32 with the layout above.  All
// arithmetic is the fp32 kernels': operands are widened on load (exact), the chunk sums, mean, variance, rstd, m0 and m1 are formed as
// above, and each result is rounded to bf16 ONCE, on store (round to nearest even).  Traffic halves: 2 B read for the statistics + 6 B
// read + 2 B written = 10 B per element forward, 8 B read per pass + 6 B written = 22 B backward.  W = 8: one 16-byte access (8 bf16)
// per operand and thread, for hw % 8 == 0 and 16-byte aligned pointers; W = 1: element by element.  One loop body serves both.
// (bf16_load / bf16_store of group i, W elements, of a plane: bf16_io.hpp)

template <int W>
__global__ void __launch_bounds__(256) instance_stats_bf16_kernel(long hw, const unsigned short *__restrict__ x, float *__restrict__ part, int pass)
{
    __shared__ float red[4];
    const long plane = blockIdx.y;
    const unsigned short *p = x + plane * hw;
    float *pp = part + plane * (2 * SPADE_CHUNKS);
    const long n = hw / W, per = (n + SPADE_CHUNKS - 1) / SPADE_CHUNKS;
    const long lo = blockIdx.x * per, hi = lo + per < n ? lo + per : n;
    const float mean = pass ? plane_mean(pp, hw) : 0.0f;
    float s = 0.0f;
    for (long i = lo + threadIdx.x; i < hi; i += 256) {
        float q[W];
        bf16_load<W>(p, i, q);
        if (pass) {
#pragma unroll
            for (int k = 0; k < W; ++k) { const float d = q[k] - mean; s += d * d; }
        } else if constexpr (W == 8) {
            s += ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
        } else {
            s += q[0];
        }
    }
    s = block_sum256(s, red);
    if (threadIdx.x == 0) pp[2 * blockIdx.x + pass] = s;
}

template <int W>
__global__ void __launch_bounds__(256) spade_modulate_bf16_kernel(long hw, const unsigned short *__restrict__ x,
                                                                  const unsigned short *__restrict__ gamma,
                                                                  const unsigned short *__restrict__ beta, const float *__restrict__ stats,
                                                                  float eps, float slope, unsigned short *__restrict__ out)
{
    const long plane = blockIdx.y, base = plane * hw, n = hw / W;
    float mean, rstd;
    plane_norm(stats + plane * (2 * SPADE_CHUNKS), hw, eps, mean, rstd);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        float xv[W], gv[W], bv[W], o[W];
        bf16_load<W>(x + base, i, xv);
        bf16_load<W>(gamma + base, i, gv);
        bf16_load<W>(beta + base, i, bv);
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const float v = ((xv[k] - mean) * rstd) * (1.0f + gv[k]) + bv[k];
            o[k] = v > 0.0f ? v : v * slope;
        }
        bf16_store<W>(out + base, i, o);
    }
}

// the mask is read from the stored bf16 output (rounding keeps the sign: out > 0 exactly when the fp32 pre-activation was)
template <int W>
__global__ void __launch_bounds__(256) spade_backward_sums_bf16_kernel(long hw, const unsigned short *__restrict__ x,
                                                                       const unsigned short *__restrict__ gamma,
                                                                       const unsigned short *__restrict__ out, const float *__restrict__ stats,
                                                                       const unsigned short *__restrict__ grad, float eps, float slope,
                                                                       float *__restrict__ work)
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
        bf16_load<W>(grad + base, i, gv);
        bf16_load<W>(x + base, i, xv);
        bf16_load<W>(gamma + base, i, mv);
        if (out) bf16_load<W>(out + base, i, ov);
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

template <int W>
__global__ void __launch_bounds__(256) spade_backward_apply_bf16_kernel(long hw, const unsigned short *__restrict__ x,
                                                                        const unsigned short *__restrict__ gamma,
                                                                        const unsigned short *__restrict__ out, const float *__restrict__ stats,
                                                                        const unsigned short *__restrict__ grad, const float *__restrict__ work,
                                                                        float eps, float slope, unsigned short *__restrict__ dx,
                                                                        unsigned short *__restrict__ dgamma, unsigned short *__restrict__ dbeta)
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
        bf16_load<W>(grad + base, i, gv);
        bf16_load<W>(x + base, i, xv);
        if (out) bf16_load<W>(out + base, i, ov);
        if (dx) bf16_load<W>(gamma + base, i, mv);
#pragma unroll
        for (int k = 0; k < W; ++k) {
            dy[k] = (!out || ov[k] > 0.0f) ? gv[k] : gv[k] * slope;
            xh[k] = (xv[k] - mean) * rstd;
        }
        if (dbeta) bf16_store<W>(dbeta + base, i, dy);
        if (dgamma) {
#pragma unroll
            for (int k = 0; k < W; ++k) o[k] = dy[k] * xh[k];
            bf16_store<W>(dgamma + base, i, o);
        }
        if (dx) {
#pragma unroll
            for (int k = 0; k < W; ++k) o[k] = rstd * ((dy[k] * (1.0f + mv[k]) - m0) - xh[k] * m1);
            bf16_store<W>(dx + base, i, o);
        }
    }
}

}  // namespace sahs

// the modulate-shaped grid: a 256-thread workgroup per 256 elements (or vectors) of a plane, capped at ~8 k workgroups in all
static dim3 spade_plane_grid(long per, long planes)
{
    long bx = (per + 255) / 256;
    const long cap = (8192 + planes - 1) / planes;
    if (bx > cap) bx = cap;
    if (bx < 1) bx = 1;
    return dim3((unsigned)bx, (unsigned)planes);
}

extern "C" long sahs_spade_stats_words(long planes) { return planes * 2 * sahs::SPADE_CHUNKS; }

extern "C" int sahs_spade_modulate_backward_launch(long planes, long hw, const float *x, const float *gamma, const float *out, const float *stats,
                                                   const float *grad, float eps, float slope, float *dx, float *dgamma, float *dbeta, float *work,
                                                   hipStream_t stream)
{
    if (planes <= 0 || hw <= 0) return 0;
    if (planes > 65535) return -2;      // gridDim.y
    auto al = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };      // (a null pointer is never dereferenced)
    const bool vec = (hw % 4 == 0) && al(x) && al(gamma) && al(out) && al(grad) && al(dx) && al(dgamma) && al(dbeta);
    if (dx) {
        const dim3 sgrid(sahs::SPADE_CHUNKS, (unsigned)planes);
        if (vec) sahs::spade_backward_sums_kernel<true><<<sgrid, 256, 0, stream>>>(hw, x, gamma, out, stats, grad, eps, slope, work);
        else sahs::spade_backward_sums_kernel<false><<<sgrid, 256, 0, stream>>>(hw, x, gamma, out, stats, grad, eps, slope, work);
    }
    const dim3 grid = spade_plane_grid(vec ? hw / 4 : hw, planes);
    if (vec) sahs::spade_backward_apply_kernel<true><<<grid, 256, 0, stream>>>(hw, x, gamma, out, stats, grad, work, eps, slope, dx, dgamma, dbeta);
    else sahs::spade_backward_apply_kernel<false><<<grid, 256, 0, stream>>>(hw, x, gamma, out, stats, grad, work, eps, slope, dx, dgamma, dbeta);
    return (int)hipGetLastError();
}

extern "C" int sahs_spade_modulate_launch(long planes, long hw, const float *x, const float *gamma, const float *beta, float eps, float slope,
                                          float *out, float *stats, hipStream_t stream)
{
    if (planes <= 0 || hw <= 0) return 0;
    if (planes > 65535) return -2;      // gridDim.y
    auto al = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
    const bool vec = (hw % 4 == 0) && al(x) && al(gamma) && al(beta) && al(out);
    const dim3 sgrid(sahs::SPADE_CHUNKS, (unsigned)planes);
    for (int pass = 0; pass < 2; ++pass) {
        if (vec) sahs::instance_stats_kernel<true><<<sgrid, 256, 0, stream>>>(hw, x, stats, pass);
        else sahs::instance_stats_kernel<false><<<sgrid, 256, 0, stream>>>(hw, x, stats, pass);
    }
    const dim3 grid = spade_plane_grid(vec ? hw / 4 : hw, planes);
    if (vec) sahs::spade_modulate_kernel<true><<<grid, 256, 0, stream>>>(hw, x, gamma, beta, stats, eps, slope, out);
    else sahs::spade_modulate_kernel<false><<<grid, 256, 0, stream>>>(hw, x, gamma, beta, stats, eps, slope, out);
    return (int)hipGetLastError();
}

// ---- the bf16 forms: same launches, same grids, groups of 8 elements where the fp32 forms take 4 ----
extern "C" int sahs_spade_modulate_bf16_launch(long planes, long hw, const unsigned short *x, const unsigned short *gamma,
                                               const unsigned short *beta, float eps, float slope, unsigned short *out, float *stats,
                                               hipStream_t stream)
{
    if (planes <= 0 || hw <= 0) return 0;
    if (planes > 65535) return -2;      // gridDim.y (capi.hip refuses it by name first)
    auto al = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
    const bool vec = (hw % 8 == 0) && al(x) && al(gamma) && al(beta) && al(out);
    const dim3 sgrid(sahs::SPADE_CHUNKS, (unsigned)planes);
    for (int pass = 0; pass < 2; ++pass) {
        if (vec) sahs::instance_stats_bf16_kernel<8><<<sgrid, 256, 0, stream>>>(hw, x, stats, pass);
        else sahs::instance_stats_bf16_kernel<1><<<sgrid, 256, 0, stream>>>(hw, x, stats, pass);
    }
    const dim3 grid = spade_plane_grid(vec ? hw / 8 : hw, planes);
    if (vec) sahs::spade_modulate_bf16_kernel<8><<<grid, 256, 0, stream>>>(hw, x, gamma, beta, stats, eps, slope, out);
    else sahs::spade_modulate_bf16_kernel<1><<<grid, 256, 0, stream>>>(hw, x, gamma, beta, stats, eps, slope, out);
    return (int)hipGetLastError();
}

extern "C" int sahs_spade_modulate_backward_bf16_launch(long planes, long hw, const unsigned short *x, const unsigned short *gamma,
                                                        const unsigned short *out, const float *stats, const unsigned short *grad, float eps,
                                                        float slope, unsigned short *dx, unsigned short *dgamma, unsigned short *dbeta,
                                                        float *work, hipStream_t stream)
{
    if (planes <= 0 || hw <= 0) return 0;
    if (planes > 65535) return -2;      // gridDim.y
    auto al = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };      // (a null pointer is never dereferenced)
    const bool vec = (hw % 8 == 0) && al(x) && al(gamma) && al(out) && al(grad) && al(dx) && al(dgamma) && al(dbeta);
    if (dx) {
        const dim3 sgrid(sahs::SPADE_CHUNKS, (unsigned)planes);
        if (vec) sahs::spade_backward_sums_bf16_kernel<8><<<sgrid, 256, 0, stream>>>(hw, x, gamma, out, stats, grad, eps, slope, work);
        else sahs::spade_backward_sums_bf16_kernel<1><<<sgrid, 256, 0, stream>>>(hw, x, gamma, out, stats, grad, eps, slope, work);
    }
    const dim3 grid = spade_plane_grid(vec ? hw / 8 : hw, planes);
    if (vec) sahs::spade_backward_apply_bf16_kernel<8><<<grid, 256, 0, stream>>>(hw, x, gamma, out, stats, grad, work, eps, slope, dx, dgamma, dbeta);
    else sahs::spade_backward_apply_bf16_kernel<1><<<grid, 256, 0, stream>>>(hw, x, gamma, out, stats, grad, work, eps, slope, dx, dgamma, dbeta);
    return (int)hipGetLastError();
}
