// spectral_norm.hip -- torch.nn.utils.spectral_norm's weight computation for a TABLE of weights, fused (the Stage-II refiner normalises 18
// convolutions per step; torch runs ~14 launches and 6 autograd nodes for each).  A job is one weight as a row-major h x w matrix W
// (h = out channels, w = in * kh * kw) with its vectors u (h) and v (w); SpectralNorm.compute_weight with n_power_iterations = 1 is
//   t = W^T u,  v <- t / max(|t|, eps);    s = W v,  u <- s / max(|s|, eps);    sigma = u . s;    out = W / sigma
// (power_iteration = 0, eval: u, v as given, sigma = u . (W v)).  The backward, u and v being constants of the graph as in torch:
//   dW = G / sigma - (sum(G o W) / sigma^2) u v^T.
// Launches, whatever the number of jobs: forward two -- the VECTORS kernel, one 1024-thread workgroup per job (every step needs a
// norm over the whole of the step before: one workgroup holds them all without a workspace or a flag), leaves u, v, sigma in the job's
// saved area, and the SCALE kernel, 64 workgroups per job, streams out = W / sigma; backward one, a workgroup per job.  The table
// travels as kernel arguments.  All sums have a fixed order (lane-sequential, a 64-lane butterfly, the 16 waves in order): no atomics,
// the same bits every run.  fp32 arithmetic throughout; a bf16 output is the fp32 quotient rounded once on store, a bf16 gradient is
// widened on load.
#include <hip/hip_runtime.h>
#include "sahs_common.hpp"
#include "sahs_launchers.hpp"
#include "elem_io.hpp"
#include "../../include/sahs_nerf.h"

namespace sahs {

constexpr int SN_MAX_JOBS = SAHS_SPECTRAL_NORM_MAX_JOBS, SN_THREADS = 1024, SN_WAVES = SN_THREADS / 64, SN_SCALE_CHUNKS = 64;
// vec: 16-byte accesses to W and the saved v (w % 4 == 0, both aligned); vec_out: 16-byte accesses of the scale pass (W and out)
struct SnJob { const float *W; float *u, *v; void *out; float *saved; int h, w, vec, vec_out; };
struct SnBatch { SnJob j[SN_MAX_JOBS]; };
struct SnGradJob { const float *W; const float *saved; const void *G; float *dW; int h, w, vec, pad; };
struct SnGradBatch { SnGradJob j[SN_MAX_JOBS]; };
static_assert(sizeof(SnBatch) <= 3072 && sizeof(SnGradBatch) <= 3072, "kernel-argument budget");

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// every thread gets the sum over the workgroup's SN_THREADS values
__device__ __forceinline__ float block_sum1024(float v, float *red)
{
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < SN_WAVES; ++k) s += red[k];
    return s;
}
// a wave's dot product of a row of w floats with x
template <int N>
__device__ __forceinline__ float row_dot(const float *row, const float *x, int w, int lane)
{
    float acc = 0.0f;
    for (int g = lane; g < w / N; g += 64) {
        float a[N], b[N];
        f32_load<N>(row, g, a);
        f32_load<N>(x, g, b);
#pragma unroll
        for (int k = 0; k < N; ++k) acc += a[k] * b[k];
    }
    return wave_sum(acc);
}

// t = W^T u -> tv[0 .. w): tiles of 64 column groups; wave k adds rows k, k + 16, ... of its lane's group, the 16 waves' sums meet in LDS
template <int N>
__device__ __forceinline__ void columns_dot(const float *W, const float *u, int h, int w, float *tv, float *tile, int wave, int lane)
{
    const int ncg = w / N;
    for (int c0 = 0; c0 < ncg; c0 += 64) {
        float acc[N];
#pragma unroll
        for (int k = 0; k < N; ++k) acc[k] = 0.0f;
        if (c0 + lane < ncg) {
            for (int i = wave; i < h; i += SN_WAVES) {
                float a[N];
                f32_load<N>(W + (long)i * w, c0 + lane, a);
                const float ui = u[i];
#pragma unroll
                for (int k = 0; k < N; ++k) acc[k] += a[k] * ui;
            }
        }
        __syncthreads();      // (the tile before this one has been read)
#pragma unroll
        for (int k = 0; k < N; ++k) tile[(wave * N + k) * 64 + lane] = acc[k];
        __syncthreads();
        if ((int)threadIdx.x < 64 * N) {
            const int k = threadIdx.x >> 6;
            float s = 0.0f;
#pragma unroll
            for (int wv = 0; wv < SN_WAVES; ++wv) s += tile[(wv * N + k) * 64 + lane];
            if (c0 + lane < ncg) tv[(c0 + lane) * N + k] = s;
        }
    }
    __syncthreads();
}

template <int N>
__device__ __forceinline__ void vectors_body(const SnJob &J, int power_iteration, float eps, float *tile, float *red)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), h = J.h, w = J.w;
    float *su = J.saved, *sv = J.saved + h;
    if (power_iteration) {
        columns_dot<N>(J.W, J.u, h, w, sv, tile, wave, lane);
        float q = 0.0f;
        for (int j = tid; j < w; j += SN_THREADS) q += sv[j] * sv[j];
        const float d = fmaxf(sqrtf(block_sum1024(q, red)), eps);
        for (int j = tid; j < w; j += SN_THREADS) {
            const float vj = sv[j] / d;
            sv[j] = vj;
            J.v[j] = vj;
        }
    } else {
        for (int j = tid; j < w; j += SN_THREADS) sv[j] = J.v[j];
        for (int i = tid; i < h; i += SN_THREADS) su[i] = J.u[i];
    }
    __syncthreads();
    // s = W v, a wave per row.  Training: s to the saved u's place, normalised below; eval: only u . s is wanted
    float part = 0.0f;
    for (int i = wave; i < h; i += SN_WAVES) {
        const float s = row_dot<N>(J.W + (long)i * w, sv, w, lane);
        if (lane == 0) {
            if (power_iteration) su[i] = s;
            else part += su[i] * s;
        }
    }
    if (power_iteration) {
        __syncthreads();
        float q = 0.0f;
        for (int i = tid; i < h; i += SN_THREADS) q += su[i] * su[i];
        const float d = fmaxf(sqrtf(block_sum1024(q, red)), eps);
        for (int i = tid; i < h; i += SN_THREADS) {      // (each thread rewrites the elements it alone reads)
            const float s = su[i], ui = s / d;
            part += ui * s;
            su[i] = ui;
            J.u[i] = ui;
        }
    }
    const float sigma = block_sum1024(part, red);
    if (tid == 0) sv[w] = sigma;
}

__global__ void __launch_bounds__(SN_THREADS) spectral_norm_vectors_kernel(SnBatch jobs, int power_iteration, float eps)
{
    __shared__ float tile[SN_WAVES * 4 * 64];
    __shared__ float red[SN_WAVES];
    const SnJob J = jobs.j[blockIdx.x];
    if (J.vec) vectors_body<4>(J, power_iteration, eps, tile, red);
    else vectors_body<1>(J, power_iteration, eps, tile, red);
}

template <int N, bool BF16>
__device__ __forceinline__ void scale_body(const SnJob &J, float sigma)
{
    const long groups = (long)J.h * J.w / N;
    for (long g = (long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (long)gridDim.x * blockDim.x) {
        float a[N];
        f32_load<N>(J.W, g, a);
#pragma unroll
        for (int k = 0; k < N; ++k) a[k] = a[k] / sigma;
        elem_store<N>(static_cast<elem_of<BF16> *>(J.out), g, a);
    }
}
// out = W / sigma: grid (chunk, job)
template <bool BF16>
__global__ void __launch_bounds__(256) spectral_norm_scale_kernel(SnBatch jobs)
{
    const SnJob J = jobs.j[blockIdx.y];
    const float sigma = J.saved[J.h + J.w];
    if (J.vec_out) scale_body<BF16 ? 8 : 4, BF16>(J, sigma);
    else scale_body<1, BF16>(J, sigma);
}

template <int N, bool BF16>
__device__ __forceinline__ void backward_body(const SnGradJob &J, float *red)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), h = J.h, w = J.w, ng = w / N;
    const float *su = J.saved, *sv = J.saved + h;
    const elem_of<BF16> *G = static_cast<const elem_of<BF16> *>(J.G);
    const float sigma = sv[w];
    float acc = 0.0f;
    for (int i = wave; i < h; i += SN_WAVES) {
        for (int g = lane; g < ng; g += 64) {
            float a[N], b[N];
            elem_load<N>(G, (long)i * ng + g, a);
            f32_load<N>(J.W, (long)i * ng + g, b);
#pragma unroll
            for (int k = 0; k < N; ++k) acc += a[k] * b[k];
        }
    }
    const float c = block_sum1024(acc, red) / (sigma * sigma);
    for (int i = wave; i < h; i += SN_WAVES) {
        const float cu = c * su[i];
        for (int g = lane; g < ng; g += 64) {
            float a[N], b[N];
            elem_load<N>(G, (long)i * ng + g, a);
            f32_load<N>(sv, g, b);
#pragma unroll
            for (int k = 0; k < N; ++k) a[k] = a[k] / sigma - cu * b[k];
            f32_store<N>(J.dW, (long)i * ng + g, a);
        }
    }
}
template <bool BF16>
__global__ void __launch_bounds__(SN_THREADS) spectral_norm_backward_kernel(SnGradBatch jobs)
{
    __shared__ float red[SN_WAVES];
    const SnGradJob J = jobs.j[blockIdx.x];
    if (J.vec) backward_body<BF16 ? 8 : 4, BF16>(J, red);
    else backward_body<1, BF16>(J, red);
}

}  // namespace sahs

static bool sn_aligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// capi.hip has validated the table: 1 <= jobs <= SN_MAX_JOBS, no null pointer, h, w >= 1, h * w < 2^31
extern "C" int sahs_spectral_norm_forward_launch(int jobs, const float *const *W, float *const *u, float *const *v, void *const *out,
                                                 float *const *saved, const int *h, const int *w, int out_bf16, int power_iteration,
                                                 float eps, hipStream_t stream)
{
    if (jobs < 1 || jobs > sahs::SN_MAX_JOBS) return -2;
    sahs::SnBatch b = {};
    for (int k = 0; k < jobs; ++k) {
        const bool vec = w[k] % 4 == 0 && sn_aligned(W[k]) && sn_aligned(saved[k] + h[k]);      // (u, v: element by element always)
        const bool vec_out = w[k] % (out_bf16 ? 8 : 4) == 0 && sn_aligned(W[k]) && sn_aligned(out[k]);
        b.j[k] = sahs::SnJob{W[k], u[k], v[k], out[k], saved[k], h[k], w[k], vec, vec_out};
    }
    sahs::spectral_norm_vectors_kernel<<<jobs, sahs::SN_THREADS, 0, stream>>>(b, power_iteration, eps);
    const dim3 grid(sahs::SN_SCALE_CHUNKS, (unsigned)jobs);
    if (out_bf16) sahs::spectral_norm_scale_kernel<true><<<grid, 256, 0, stream>>>(b);
    else sahs::spectral_norm_scale_kernel<false><<<grid, 256, 0, stream>>>(b);
    return (int)hipGetLastError();
}

extern "C" int sahs_spectral_norm_backward_launch(int jobs, const float *const *W, const float *const *saved, const void *const *grad_out,
                                                  float *const *dW, const int *h, const int *w, int grad_bf16, hipStream_t stream)
{
    if (jobs < 1 || jobs > sahs::SN_MAX_JOBS) return -2;
    sahs::SnGradBatch b = {};
    for (int k = 0; k < jobs; ++k) {
        const bool vec = w[k] % (grad_bf16 ? 8 : 4) == 0 && sn_aligned(W[k]) && sn_aligned(saved[k] + h[k]) && sn_aligned(grad_out[k]) &&
                         sn_aligned(dW[k]);
        b.j[k] = sahs::SnGradJob{W[k], saved[k], grad_out[k], dW[k], h[k], w[k], vec, 0};
    }
    if (grad_bf16) sahs::spectral_norm_backward_kernel<true><<<jobs, sahs::SN_THREADS, 0, stream>>>(b);
    else sahs::spectral_norm_backward_kernel<false><<<jobs, sahs::SN_THREADS, 0, stream>>>(b);
    return (int)hipGetLastError();
}
