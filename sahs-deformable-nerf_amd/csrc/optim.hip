// optim.hip -- the optimiser step over the canonical flat parameter buffer (include/sahs_nerf.h: sahs_adam_step).
//
// torch.optim.Adam (weight_decay 0, amsgrad off, maximize off) as ONE streaming launch over n contiguous fp32 values: reads p, g, m, v,
// writes p, m, v -- 28 bytes per parameter, nothing else, so the kernel is bound by HBM and has no arithmetic worth hiding.  The update is
// torch's own single-tensor fp32 statement, operation for operation (torch/optim/adam.py: _single_tensor_adam), with the scalars formed in
// double on the host:
//     m  <- m + (g - m) * (1 - beta1)                      (Tensor.lerp_: that form, not beta1 * m + (1 - beta1) * g)
//     v  <- v * beta2 + (1 - beta2) * (g * g)
//     p  <- p - step_size * (m / (sqrt(v) / sqrt(1 - beta2^t) + eps)),      step_size = lr / (1 - beta1^t)
// sqrt and / are the correctly rounded ones (no rcp / rsq forms; the build has -ffp-contract=off, so nothing is fused either).
#include <hip/hip_runtime.h>
#include "sahs_launchers.hpp"

namespace sahs {

struct AdamScalars {
    float w1;          // 1 - beta1
    float beta2, w2;   // beta2, 1 - beta2
    float step_size;   // lr / (1 - beta1^t)
    float bc2_sqrt;    // sqrt(1 - beta2^t)
    float eps;
    float grad_scale;  // multiplies the gradient as it is read (1 / world after a summed all-reduce)
};

__device__ __forceinline__ void adam_update(float &p, float g, float &m, float &v, const AdamScalars &s)
{
    g = g * s.grad_scale;
    const float d = g - m;
    m = s.w1 < 0.5f ? m + s.w1 * d : g - d * (1.0f - s.w1);      // at::lerp's two branches
    v = v * s.beta2 + s.w2 * (g * g);
    const float denom = sqrtf(v) / s.bc2_sqrt + s.eps;
    p = p + (-s.step_size) * (m / denom);
}

// head: elements [0, head) one by one (up to the first 16-byte boundary, the same for all four pointers -- the launcher passes head = n
// when their alignments differ); body: n4 float4 groups, grid-stride; tail: the last (n - head) % 4 elements.
__global__ __launch_bounds__(256) void adam_step_kernel(float *__restrict__ params, const float *__restrict__ grad, float *__restrict__ exp_avg,
                                                        float *__restrict__ exp_avg_sq, long n, long head, AdamScalars s)
{
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long nthreads = (long)gridDim.x * blockDim.x;
    const long n4 = (n - head) >> 2;
    float4 *p4 = reinterpret_cast<float4 *>(params + head);
    const float4 *g4 = reinterpret_cast<const float4 *>(grad + head);
    float4 *m4 = reinterpret_cast<float4 *>(exp_avg + head);
    float4 *v4 = reinterpret_cast<float4 *>(exp_avg_sq + head);
    for (long i = tid; i < n4; i += nthreads) {
        float4 p = p4[i], m = m4[i], v = v4[i];
        const float4 g = g4[i];
        adam_update(p.x, g.x, m.x, v.x, s);
        adam_update(p.y, g.y, m.y, v.y, s);
        adam_update(p.z, g.z, m.z, v.z, s);
        adam_update(p.w, g.w, m.w, v.w, s);
        p4[i] = p;
        m4[i] = m;
        v4[i] = v;
    }
    // the scalar ends: [0, head) and [head + 4 * n4, n) -- at most 3 + 3 elements on the vector path, everything on the other
    const long tail0 = head + (n4 << 2);
    const long ends = head + (n - tail0);
    for (long j = tid; j < ends; j += nthreads) {
        const long i = j < head ? j : tail0 + (j - head);
        float p = params[i], m = exp_avg[i], v = exp_avg_sq[i];
        adam_update(p, grad[i], m, v, s);
        params[i] = p;
        exp_avg[i] = m;
        exp_avg_sq[i] = v;
    }
}

}  // namespace sahs

extern "C" int sahs_adam_step_launch(float *params, const float *grad, float *exp_avg, float *exp_avg_sq, long n, float w1, float beta2,
                                     float w2, float step_size, float bc2_sqrt, float eps, float grad_scale, hipStream_t stream)
{
    if (n <= 0) return 0;
    const uintptr_t a = reinterpret_cast<uintptr_t>(params) & 15u;
    const bool same = (reinterpret_cast<uintptr_t>(grad) & 15u) == a && (reinterpret_cast<uintptr_t>(exp_avg) & 15u) == a &&
                      (reinterpret_cast<uintptr_t>(exp_avg_sq) & 15u) == a;
    long head = same ? (long)(((16u - a) & 15u) >> 2) : n;      // pointers are 4-byte aligned (capi.hip checks)
    if (head > n) head = n;
    const long n4 = (n - head) >> 2;
    const long work = n4 > 0 ? n4 : n;
    long blocks = (work + 255) / 256;
    if (blocks > 2048) blocks = 2048;      // 8 workgroups per CU on 256 CUs, grid-stride beyond
    const sahs::AdamScalars s{w1, beta2, w2, step_size, bc2_sqrt, eps, grad_scale};
    sahs::adam_step_kernel<<<dim3((unsigned)blocks), 256, 0, stream>>>(params, grad, exp_avg, exp_avg_sq, n, head, s);
    return (int)hipGetLastError();
}
