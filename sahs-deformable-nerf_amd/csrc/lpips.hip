// lpips.hip -- the two fused ends of LPIPS (net = alex, v0.1; the reference scores frames with it: nerf/metrics.py:95-100).  The five
// AlexNet feature maps between them are MIOpen convolutions (metrics.py: LPIPS); here are
//   PREPARE kernel   one launch: both image batches, uint8 or fp32 and read in place through four element strides, become ONE
//                    contiguous (2B, 3, H, W) fp32 tensor (rows [0, B) from a, [B, 2B) from b) that has been through the scaling layer:
//                    x / 255 for uint8, the optional 2x - 1, then (x - shift) / scale per channel.  A thread per pixel: it reads the
//                    pixel's three channels and writes one float into each plane, consecutive threads consecutive addresses.  Every
//                    operation is one correctly rounded fp32 operation in the order written (no contraction: 2x is exact anyway).
//   DISTANCE         two launches whatever the batch and the number of layers.  A job is one layer: its (2B, C, h, w) contiguous fp32
//                    features, its C channel weights w, C and h * w; the table of up to five jobs travels as kernel arguments.
//     TILE kernel      a workgroup owns LP_T consecutive pixels of one (image, layer), a thread one pixel.  It walks the channels, reading
//                      each feature value ONCE (consecutive threads consecutive addresses of a channel plane; w staged in LDS), and keeps five
//                      float64 sums: sum a^2, sum b^2, sum w a^2, sum w b^2, sum w a b (a product of two fp32 values is exact in float64).
//                      With na = sqrt(sum a^2) + 1e-10 the pixel's distance  sum_c w_c (a_c / na - b_c / nb)^2  is, expanded,
//                          sum w a^2 / na^2 + sum w b^2 / nb^2 - 2 sum w a b / (na nb):
//                      exactly 0 for equal features (x + x - 2x), and 0, not NaN, for a pixel that ReLU left all zero (0 / 1e-20).
//                      The workgroup adds its pixels -- a 64-lane butterfly, then the four waves in order -- into one float64 record.
//     FINALIZE kernel  a workgroup per image adds each layer's records in a fixed order, divides by h * w and writes
//                      [LPIPS, d_0 .. d_4] (layers beyond the job count: 0).
// No atomics, every sum in an order that does not depend on the batch: the same bits every run, and a batch gives the bits of its
// single calls.
// The same two ends as a training term (ops.lpips_prepare_loss, ops.lpips_head): gradients flow to the FIRST operand only.
//   PREPARE, loss form     the first operand is fp32 and may be clamped to [0, 1] ahead of the scaling layer; the second is uint8 or fp32.
//   PREPARE GRAD kernel    one launch, a thread per pixel: grad_pred[c] = gx[c] / scale[c] (one correctly rounded division), doubled under
//                          normalize (exact), +0 where the clamp is on and pred is not in [0, 1] (a NaN pred passes nothing).
//   HEAD, two operands     the tile and finalize kernels with each layer's two operands as two pointers.  With a stats buffer the tile
//                          kernel also stores, per (image, layer, pixel), ra = 1 / na, rb = 1 / nb and
//                              q = S / (sqrt(sa) na),   S = swa / na - swab / nb = sum_c w_c (a^_c - b^_c) a_c,   q = 0 where sa == 0
//                          (there a -> a / (|a| + 1e-10) has the Jacobian I / 1e-10: 0 is the derivative, not a patch), as three planes
//                          of doubles: consecutive threads write consecutive addresses.
//   HEAD BACKWARD kernel   one launch over all layers with the forward's job table and tile mapping, a thread per pixel walking the
//                          channels: grad_a[c] = (float)( (2 g_i / hw) ra ( w_c (a_c ra - b_c rb) - a_c q ) ), float64 arithmetic rounded to
//                          fp32 once, every element written by exactly one thread.  For equal operands a_c ra - b_c rb and S are
//                          differences of identical values: the gradient is exactly 0.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>
#include "sahs_common.hpp"
#include "sahs_launchers.hpp"
#include "../../include/sahs_nerf.h"

namespace sahs {

constexpr int LP_T = SAHS_LPIPS_TILE, LP_THREADS = 256, LP_WAVES = LP_THREADS / 64, LP_JOBS = SAHS_LPIPS_MAX_JOBS;
constexpr int LP_MAX_C = SAHS_LPIPS_MAX_CHANNELS;
static_assert(LP_T == LP_THREADS, "a thread per pixel of the tile");

struct LpPrepArgs {
    const void *a, *b;
    long sa[4], sb[4];      // element strides: batch, row, column, channel
    long B, pixels;      // pixels = 2 B H W
    int H, W, normalize, clamp;      // clamp: the first operand only
    float *out;
};

struct LpPrepGradArgs {
    const float *pred, *gx;      // gx: contiguous (B, 3, H, W)
    float *grad;
    long sp[4], sg[4];      // element strides of pred and grad: batch, row, column, channel
    long pixels;      // B H W
    int H, W, normalize, clamp;
};

// tile0: the layer's first record within an image's records; pix0: its first pixel within an image's stats
struct LpJob { const float *fa, *fb, *w; int C, hw, tiles, tile0; long pix0; };
struct LpBatch { LpJob j[LP_JOBS]; long B, pixels_per_image; int jobs, tiles_per_image; };
static_assert(sizeof(LpBatch) <= 512, "kernel-argument budget");
struct LpGrads { float *ga[LP_JOBS]; const void *g; int g_is_double; };

__device__ __forceinline__ double lp_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <class T>
__device__ __forceinline__ float lp_load(const void *base, long off)
{
    if constexpr (std::is_same<T, float>::value) return static_cast<const float *>(base)[off];
    else return (float)static_cast<const uint8_t *>(base)[off] / 255.0f;
}

template <class TA, class TB>
__global__ __launch_bounds__(LP_THREADS) void lpips_prepare_kernel(LpPrepArgs p)
{
    const long i = (long)blockIdx.x * LP_THREADS + threadIdx.x;
    if (i >= p.pixels) return;
    const long plane = (long)p.H * p.W, row = i / plane, rest = i % plane;
    const int y = (int)(rest / p.W), x = (int)(rest % p.W);
    const bool second = row >= p.B;
    const long *s = second ? p.sb : p.sa;
    const long off = (second ? row - p.B : row) * s[0] + y * s[1] + x * s[2];
    const float shift[3] = {-0.030f, -0.088f, -0.188f}, scale[3] = {0.458f, 0.448f, 0.450f};
    float *out = p.out + row * 3 * plane + rest;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v = second ? lp_load<TB>(p.b, off + c * s[3]) : lp_load<TA>(p.a, off + c * s[3]);
        if (p.clamp && !second) v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);      // (a NaN stays a NaN, as torch.clamp leaves it)
        if (p.normalize) v = 2.0f * v - 1.0f;
        out[c * plane] = (v - shift[c]) / scale[c];
    }
}

__global__ __launch_bounds__(LP_THREADS) void lpips_prepare_grad_kernel(LpPrepGradArgs p)
{
    const long i = (long)blockIdx.x * LP_THREADS + threadIdx.x;
    if (i >= p.pixels) return;
    const long plane = (long)p.H * p.W, row = i / plane, rest = i % plane;
    const int y = (int)(rest / p.W), x = (int)(rest % p.W);
    const float *pred = p.pred + row * p.sp[0] + y * p.sp[1] + x * p.sp[2];
    float *grad = p.grad + row * p.sg[0] + y * p.sg[1] + x * p.sg[2];
    const float *gx = p.gx + row * 3 * plane + rest;
    const float scale[3] = {0.458f, 0.448f, 0.450f};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float g = gx[c * plane] / scale[c];
        if (p.normalize) g = 2.0f * g;
        if (p.clamp) {      // torch's rule: the gradient passes where 0 <= pred <= 1, both ends included (a NaN passes nothing)
            const float v = pred[c * p.sp[3]];
            if (!(v >= 0.0f && v <= 1.0f)) g = 0.0f;
        }
        grad[c * p.sg[3]] = g;
    }
}

// stats: null, or three planes of B * pixels_per_image doubles [ra | rb | q], a pixel at img * pixels_per_image + pix0 + pix
__global__ __launch_bounds__(LP_THREADS) void lpips_distance_tile_kernel(LpBatch p, double *records, double *stats)
{
    __shared__ float w_s[LP_MAX_C];
    __shared__ double red[LP_WAVES];
    const long img = blockIdx.x / p.tiles_per_image;
    const int r = blockIdx.x % p.tiles_per_image;
    int l = 0;
#pragma unroll
    for (int k = 1; k < LP_JOBS; ++k)
        if (k < p.jobs && r >= p.j[k].tile0) l = k;
    const float *fa = p.j[l].fa, *fb = p.j[l].fb, *w = p.j[l].w;
    const int C = p.j[l].C, hw = p.j[l].hw, pix = (r - p.j[l].tile0) * LP_T + (int)threadIdx.x;
    for (int c = threadIdx.x; c < C; c += LP_THREADS) w_s[c] = w[c];
    __syncthreads();

    double d = 0.0;
    if (pix < hw) {
        const float *pa = fa + img * C * hw + pix, *pb = fb + img * C * hw + pix;      // (long arithmetic: img is long)
        double sa = 0.0, sb = 0.0, swa = 0.0, swb = 0.0, swab = 0.0;
        int c = 0;
        for (; c + 4 <= C; c += 4) {      // four channels' loads in flight; the sums stay in channel order
            float va[4], vb[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) { va[k] = pa[(long)(c + k) * hw]; vb[k] = pb[(long)(c + k) * hw]; }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double a = va[k], b = vb[k], wc = w_s[c + k], aa = a * a, bb = b * b, ab = a * b;
                sa += aa;
                sb += bb;
                swa += wc * aa;
                swb += wc * bb;
                swab += wc * ab;
            }
        }
        for (; c < C; ++c) {
            const double a = pa[(long)c * hw], b = pb[(long)c * hw], wc = w_s[c], aa = a * a, bb = b * b, ab = a * b;
            sa += aa;
            sb += bb;
            swa += wc * aa;
            swb += wc * bb;
            swab += wc * ab;
        }
        const double na = sqrt(sa) + 1e-10, nb = sqrt(sb) + 1e-10;
        d = swa / (na * na) + swb / (nb * nb) - 2.0 * (swab / (na * nb));
        if (stats) {      // what the backward needs of the five sums (equal operands: swa == swab and na == nb, so S is exactly 0)
            const long plane = p.B * p.pixels_per_image, at = img * p.pixels_per_image + p.j[l].pix0 + pix;
            const double S = swa / na - swab / nb;
            stats[at] = 1.0 / na;
            stats[plane + at] = 1.0 / nb;
            stats[2 * plane + at] = sa == 0.0 ? 0.0 : S / (sqrt(sa) * na);
        }
    }
    d = lp_wave_sum(d);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = d;
    __syncthreads();
    if (threadIdx.x == 0) records[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// out row of image i: [LPIPS, d_0 .. d_4]
__global__ __launch_bounds__(LP_THREADS) void lpips_distance_finalize_kernel(LpBatch p, const double *records, double *out)
{
    __shared__ double red[LP_WAVES][LP_JOBS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double *rec = records + (long)blockIdx.x * p.tiles_per_image;
    for (int l = 0; l < p.jobs; ++l) {
        double s = 0.0;
        for (int t = threadIdx.x; t < p.j[l].tiles; t += LP_THREADS) s += rec[p.j[l].tile0 + t];
        s = lp_wave_sum(s);
        if (lane == 0) red[wave][l] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double *o = out + (long)blockIdx.x * (1 + LP_JOBS), total = 0.0;
        for (int l = 0; l < LP_JOBS; ++l) {
            double dl = 0.0;
            if (l < p.jobs) dl = (((red[0][l] + red[1][l]) + red[2][l]) + red[3][l]) / (double)p.j[l].hw;
            o[1 + l] = dl;
            total += dl;
        }
        o[0] = total;
    }
}

// the forward's mapping of workgroups to (image, layer, tile); grad_a[l] has fa[l]'s layout
__global__ __launch_bounds__(LP_THREADS) void lpips_head_backward_kernel(LpBatch p, LpGrads o, const double *stats)
{
    __shared__ float w_s[LP_MAX_C];
    const long img = blockIdx.x / p.tiles_per_image;
    const int r = blockIdx.x % p.tiles_per_image;
    int l = 0;
#pragma unroll
    for (int k = 1; k < LP_JOBS; ++k)
        if (k < p.jobs && r >= p.j[k].tile0) l = k;
    const float *w = p.j[l].w;
    const int C = p.j[l].C, hw = p.j[l].hw, pix = (r - p.j[l].tile0) * LP_T + (int)threadIdx.x;
    for (int c = threadIdx.x; c < C; c += LP_THREADS) w_s[c] = w[c];
    __syncthreads();
    if (pix >= hw) return;

    const long plane = p.B * p.pixels_per_image, at = img * p.pixels_per_image + p.j[l].pix0 + pix;
    const double ra = stats[at], rb = stats[plane + at], q = stats[2 * plane + at];
    const double gi = o.g_is_double ? static_cast<const double *>(o.g)[img] : (double)static_cast<const float *>(o.g)[img];
    const double k = (2.0 * gi / (double)hw) * ra;
    const float *pa = p.j[l].fa + img * C * hw + pix, *pb = p.j[l].fb + img * C * hw + pix;      // (long arithmetic: img is long)
    float *pg = o.ga[l] + img * C * hw + pix;
    int c = 0;
    for (; c + 4 <= C; c += 4) {      // four channels' loads in flight
        float va[4], vb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { va[u] = pa[(long)(c + u) * hw]; vb[u] = pb[(long)(c + u) * hw]; }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double a = va[u], b = vb[u], wc = w_s[c + u];
            pg[(long)(c + u) * hw] = (float)(k * (wc * (a * ra - b * rb) - a * q));
        }
    }
    for (; c < C; ++c) {
        const double a = pa[(long)c * hw], b = pb[(long)c * hw], wc = w_s[c];
        pg[(long)c * hw] = (float)(k * (wc * (a * ra - b * rb) - a * q));
    }
}

}      // namespace sahs

// arguments already validated (capi.hip): C == 3, 31 <= H, W <= 32768, 2 B H W < 2^31 * 256
int sahs_lpips_prepare_launch(const void *a, const void *b, int a_is_float, int b_is_float, long B, int H, int W, const long *stride_a,
                              const long *stride_b, int normalize, int clamp, float *out, hipStream_t stream)
{
    using namespace sahs;
    LpPrepArgs args;
    args.a = a;
    args.b = b;
    for (int k = 0; k < 4; ++k) { args.sa[k] = stride_a[k]; args.sb[k] = stride_b[k]; }
    args.B = B;
    args.pixels = 2 * B * (long)H * W;
    args.H = H;
    args.W = W;
    args.normalize = normalize;
    args.clamp = clamp;
    args.out = out;
    const unsigned grid = (unsigned)((args.pixels + LP_THREADS - 1) / LP_THREADS);
    if (a_is_float && b_is_float) hipLaunchKernelGGL((lpips_prepare_kernel<float, float>), dim3(grid), dim3(LP_THREADS), 0, stream, args);
    else if (a_is_float) hipLaunchKernelGGL((lpips_prepare_kernel<float, uint8_t>), dim3(grid), dim3(LP_THREADS), 0, stream, args);
    else hipLaunchKernelGGL((lpips_prepare_kernel<uint8_t, uint8_t>), dim3(grid), dim3(LP_THREADS), 0, stream, args);
    return (int)hipGetLastError();
}

// arguments already validated (capi.hip): 31 <= H, W <= 32768, B H W < 2^39
int sahs_lpips_prepare_grad_launch(const float *pred, const float *gx, long B, int H, int W, const long *stride_pred, int normalize, int clamp,
                                   float *grad, const long *stride_grad, hipStream_t stream)
{
    using namespace sahs;
    LpPrepGradArgs args;
    args.pred = pred;
    args.gx = gx;
    args.grad = grad;
    for (int k = 0; k < 4; ++k) { args.sp[k] = stride_pred[k]; args.sg[k] = stride_grad[k]; }
    args.pixels = B * (long)H * W;
    args.H = H;
    args.W = W;
    args.normalize = normalize;
    args.clamp = clamp;
    const unsigned grid = (unsigned)((args.pixels + LP_THREADS - 1) / LP_THREADS);
    hipLaunchKernelGGL(lpips_prepare_grad_kernel, dim3(grid), dim3(LP_THREADS), 0, stream, args);
    return (int)hipGetLastError();
}

long sahs_lpips_distance_tiles(int jobs, const long *hw)
{
    long t = 0;
    for (int k = 0; k < jobs; ++k) t += (hw[k] + sahs::LP_T - 1) / sahs::LP_T;
    return t;
}

long sahs_lpips_head_pixels(int jobs, const long *hw)
{
    long n = 0;
    for (int k = 0; k < jobs; ++k) n += hw[k];
    return n;
}

static sahs::LpBatch lp_batch(int jobs, const float *const *fa, const float *const *fb, const float *const *weights, const int *C, const long *hw,
                              long B)
{
    using namespace sahs;
    LpBatch p = {};
    int tile0 = 0;
    long pix0 = 0;
    for (int k = 0; k < jobs; ++k) {
        LpJob &j = p.j[k];
        j.fa = fa[k];
        j.fb = fb[k];
        j.w = weights[k];
        j.C = C[k];
        j.hw = (int)hw[k];
        j.tiles = (int)((hw[k] + LP_T - 1) / LP_T);
        j.tile0 = tile0;
        j.pix0 = pix0;
        tile0 += j.tiles;
        pix0 += hw[k];
    }
    p.B = B;
    p.pixels_per_image = pix0;
    p.jobs = jobs;
    p.tiles_per_image = tile0;
    return p;
}

// arguments already validated (capi.hip): 1 <= jobs <= 5, 1 <= C <= SAHS_LPIPS_MAX_CHANNELS, 1 <= hw <= 2^30, B * tiles < 2^31;
// records: B * sahs_lpips_distance_tiles(jobs, hw) doubles; stats: null, or 3 * B * sahs_lpips_head_pixels(jobs, hw) doubles
int sahs_lpips_head_forward_launch(int jobs, const float *const *fa, const float *const *fb, const float *const *weights, const int *C,
                                   const long *hw, long B, double *out, double *stats, double *records, hipStream_t stream)
{
    using namespace sahs;
    const LpBatch p = lp_batch(jobs, fa, fb, weights, C, hw, B);
    hipLaunchKernelGGL(lpips_distance_tile_kernel, dim3((unsigned)(B * p.tiles_per_image)), dim3(LP_THREADS), 0, stream, p, records, stats);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(lpips_distance_finalize_kernel, dim3((unsigned)B), dim3(LP_THREADS), 0, stream, p, (const double *)records, out);
    return (int)hipGetLastError();
}

// arguments validated as the forward's; g: B doubles or floats; grad_a[l]: fa[l]'s (B, C, h, w)
int sahs_lpips_head_backward_launch(int jobs, const float *const *fa, const float *const *fb, const float *const *weights, const int *C,
                                    const long *hw, long B, const void *g, int g_is_double, const double *stats, float *const *grad_a,
                                    hipStream_t stream)
{
    using namespace sahs;
    const LpBatch p = lp_batch(jobs, fa, fb, weights, C, hw, B);
    LpGrads o = {};
    for (int k = 0; k < jobs; ++k) o.ga[k] = grad_a[k];
    o.g = g;
    o.g_is_double = g_is_double;
    hipLaunchKernelGGL(lpips_head_backward_kernel, dim3((unsigned)(B * p.tiles_per_image)), dim3(LP_THREADS), 0, stream, p, o, stats);
    return (int)hipGetLastError();
}
