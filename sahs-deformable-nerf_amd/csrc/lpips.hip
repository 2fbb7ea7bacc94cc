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
    int H, W, normalize;
    float *out;
};

struct LpJob { const float *f, *w; int C, hw, tiles, tile0; };      // tile0: the layer's first record within an image's records
struct LpBatch { LpJob j[LP_JOBS]; long B; int jobs, tiles_per_image; };
static_assert(sizeof(LpBatch) <= 512, "kernel-argument budget");

__device__ __forceinline__ double lp_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <class T>
__global__ __launch_bounds__(LP_THREADS) void lpips_prepare_kernel(LpPrepArgs p)
{
    const long i = (long)blockIdx.x * LP_THREADS + threadIdx.x;
    if (i >= p.pixels) return;
    const long plane = (long)p.H * p.W, row = i / plane, rest = i % plane;
    const int y = (int)(rest / p.W), x = (int)(rest % p.W);
    const bool second = row >= p.B;
    const long *s = second ? p.sb : p.sa;
    const T *src = static_cast<const T *>(second ? p.b : p.a) + (second ? row - p.B : row) * s[0] + y * s[1] + x * s[2];
    const float shift[3] = {-0.030f, -0.088f, -0.188f}, scale[3] = {0.458f, 0.448f, 0.450f};
    float *out = p.out + row * 3 * plane + rest;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float v;
        if constexpr (std::is_same<T, float>::value) v = src[c * s[3]];
        else v = (float)src[c * s[3]] / 255.0f;
        if (p.normalize) v = 2.0f * v - 1.0f;
        out[c * plane] = (v - shift[c]) / scale[c];
    }
}

__global__ __launch_bounds__(LP_THREADS) void lpips_distance_tile_kernel(LpBatch p, double *records)
{
    __shared__ float w_s[LP_MAX_C];
    __shared__ double red[LP_WAVES];
    const long img = blockIdx.x / p.tiles_per_image;
    const int r = blockIdx.x % p.tiles_per_image;
    int l = 0;
#pragma unroll
    for (int k = 1; k < LP_JOBS; ++k)
        if (k < p.jobs && r >= p.j[k].tile0) l = k;
    const float *f = p.j[l].f, *w = p.j[l].w;
    const int C = p.j[l].C, hw = p.j[l].hw, pix = (r - p.j[l].tile0) * LP_T + (int)threadIdx.x;
    for (int c = threadIdx.x; c < C; c += LP_THREADS) w_s[c] = w[c];
    __syncthreads();

    double d = 0.0;
    if (pix < hw) {
        const float *pa = f + img * C * hw + pix, *pb = f + (p.B + img) * C * hw + pix;      // (long arithmetic: img is long)
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

}      // namespace sahs

// arguments already validated (capi.hip): C == 3, 31 <= H, W <= 32768, 2 B H W < 2^31 * 256
int sahs_lpips_prepare_launch(const void *a, const void *b, int is_float, long B, int H, int W, const long *stride_a, const long *stride_b,
                              int normalize, float *out, hipStream_t stream)
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
    args.out = out;
    const unsigned grid = (unsigned)((args.pixels + LP_THREADS - 1) / LP_THREADS);
    if (is_float) hipLaunchKernelGGL(lpips_prepare_kernel<float>, dim3(grid), dim3(LP_THREADS), 0, stream, args);
    else hipLaunchKernelGGL(lpips_prepare_kernel<uint8_t>, dim3(grid), dim3(LP_THREADS), 0, stream, args);
    return (int)hipGetLastError();
}

long sahs_lpips_distance_tiles(int jobs, const long *hw)
{
    long t = 0;
    for (int k = 0; k < jobs; ++k) t += (hw[k] + sahs::LP_T - 1) / sahs::LP_T;
    return t;
}

// arguments already validated (capi.hip): 1 <= jobs <= 5, 1 <= C <= SAHS_LPIPS_MAX_CHANNELS, 1 <= hw <= 2^30, B * tiles < 2^31;
// records: B * sahs_lpips_distance_tiles(jobs, hw) doubles
int sahs_lpips_distance_launch(int jobs, const float *const *features, const float *const *weights, const int *C, const long *hw, long B,
                               double *out, double *records, hipStream_t stream)
{
    using namespace sahs;
    LpBatch p = {};
    int tile0 = 0;
    for (int k = 0; k < jobs; ++k) {
        LpJob &j = p.j[k];
        j.f = features[k];
        j.w = weights[k];
        j.C = C[k];
        j.hw = (int)hw[k];
        j.tiles = (int)((hw[k] + LP_T - 1) / LP_T);
        j.tile0 = tile0;
        tile0 += j.tiles;
    }
    p.B = B;
    p.jobs = jobs;
    p.tiles_per_image = tile0;
    hipLaunchKernelGGL(lpips_distance_tile_kernel, dim3((unsigned)(B * tile0)), dim3(LP_THREADS), 0, stream, p, records);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(lpips_distance_finalize_kernel, dim3((unsigned)B), dim3(LP_THREADS), 0, stream, p, (const double *)records, out);
    return (int)hipGetLastError();
}
