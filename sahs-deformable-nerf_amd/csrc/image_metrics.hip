// image_metrics.hip -- L1, MSE and windowed SSIM of two image batches in one pass (the reference scores frames with scikit-image:
// nerf/metrics.py; structural_similarity's defaults are a 7x7 box filter over five moment planes, sample covariance, and the mean over
// the windows that lie wholly inside the image).  Two launches per call, whatever the batch:
//   TILE kernel      a workgroup owns one IM_T x IM_T block of window origins of one image.  It stages the (IM_T+6)^2 x C halo of both
//                    images in LDS (one read of each image element per tile that needs it), forms the five 7x7 moments separably --
//                    a thread walks 10 halo rows of one column, sums 7 taps per row and adds the row sums into its 4 windows -- and
//                    evaluates S per window and channel.  While staging it also adds |a-b| and (a-b)^2 over the block of PIXELS it
//                    owns: a different domain from the windows (the last tile row / column own the image's last 6 rows / columns
//                    too), every pixel in exactly one workgroup.  One record of doubles per (image, tile): [sum S per channel,
//                    sum |d|, sum d^2].
//   FINALIZE kernel  a workgroup per image adds the records in a fixed order in float64 and writes [mean SSIM, MSE, L1, SSIM per channel].
// No atomics, every sum in a fixed order that does not depend on the batch: the same bits every run, and a batch gives the bits of
// its single calls.
// Numerics.  uint8: the moments are integers -- sum x <= 49*255, sum x^2 <= 49*255^2, and n = 49 sum x^2 - (sum x)^2 < 2^31 -- so the
// variances and the covariance are exact in int32 and are converted once; sum |d| and sum d^2 of a tile are exact in uint32.
// fp32: E[x^2] - E[x]^2 from raw fp32 moments cancels (5e-6 of SSIM on a flat bright pair), so the moments are CENTRED: each tile
// subtracts a per-channel shift near its local level (the mean of an 8x8 sample of its halo; any value is a valid shift, a close one
// makes x' = x - shift small), x' is formed exactly in float64 and the sums of x', x'^2, x'y' run in float64, which costs the vector ALU less than the staging does.
// With n = 49 sum x'^2 - (sum x')^2 = 49*48 var and m = 49 shift + sum x' = 49 mean, in the image's own units (scale 255 for uint8, 1 for float):
//   S = (2 mx my + K1)(2 nxy + K2) / ((mx^2 + my^2 + K1)(nx + ny + K2)),   K1 = 49^2 C1 scale^2,  K2 = 49*48 C2 scale^2.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>
#include "sahs_common.hpp"
#include "sahs_launchers.hpp"
#include "../../include/sahs_nerf.h"

namespace sahs {

constexpr int IM_T = SAHS_IMAGE_METRICS_TILE, IM_WIN = 7, IM_HALO = IM_T + IM_WIN - 1, IM_THREADS = 256, IM_WAVES = IM_THREADS / 64;
constexpr int IM_ROWS = 4;      // windows per thread: rows 4g .. 4g+3 of column x, from halo rows 4g .. 4g+9
static_assert(IM_T == 32 && IM_THREADS == IM_T * (IM_T / IM_ROWS), "a thread per (column, group of IM_ROWS rows)");
static_assert(2 * 4 * IM_HALO * IM_HALO * 4 <= 65536, "LDS: both halos at four channels");

struct ImArgs {
    const void *a, *b;
    long sa[4], sb[4];      // element strides: batch, row, column, channel
    int H, W, tiles_x, tiles_y;
    int c_fastest;      // staging order: channel innermost (channels-last memory) or column innermost
    double K1, K2;
    double *records;
};

template <class T> struct ImTraits;
template <> struct ImTraits<uint8_t> { typedef int word; typedef int acc; typedef unsigned int dsum; };
template <> struct ImTraits<float> { typedef float word; typedef double acc; typedef double dsum; };

__device__ __forceinline__ double wave_sum_f64(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <class T, int C>
__global__ __launch_bounds__(IM_THREADS) void image_metrics_tile_kernel(ImArgs p)
{
    typedef typename ImTraits<T>::word word;
    typedef typename ImTraits<T>::acc acc;
    typedef typename ImTraits<T>::dsum dsum;
    constexpr bool kFloat = std::is_same<T, float>::value;
    constexpr int PLANE = IM_HALO * IM_HALO;
    __shared__ word tile_a[C * PLANE], tile_b[C * PLANE];
    __shared__ double red[IM_WAVES][C + 2];

    const int tiles = p.tiles_x * p.tiles_y;
    const long img = blockIdx.x / tiles;
    const int tile = blockIdx.x % tiles, ty = tile / p.tiles_x, tx = tile % p.tiles_x;
    const int y0 = ty * IM_T, x0 = tx * IM_T;
    const int in_h = min(IM_HALO, p.H - y0), in_w = min(IM_HALO, p.W - x0);      // the part of the halo inside the image (>= 7 each)
    const int own_h = ty == p.tiles_y - 1 ? in_h : IM_T, own_w = tx == p.tiles_x - 1 ? in_w : IM_T;      // the pixels this tile owns
    const T *a = static_cast<const T *>(p.a) + img * p.sa[0] + y0 * p.sa[1] + x0 * p.sa[2];
    const T *b = static_cast<const T *>(p.b) + img * p.sb[0] + y0 * p.sb[1] + x0 * p.sb[2];

    // ---- stage both halos (zero outside the image: only invalid windows read those), and the pixel sums of the owned block ----
    dsum d1 = 0, d2 = 0;
    for (int i = threadIdx.x; i < C * PLANE; i += IM_THREADS) {
        int c, r, x;
        if (p.c_fastest) { c = i % C; x = (i / C) % IM_HALO; r = i / (C * IM_HALO); }
        else { x = i % IM_HALO; r = (i / IM_HALO) % IM_HALO; c = i / PLANE; }
        word va = 0, vb = 0;
        if (r < in_h && x < in_w) {
            va = a[r * p.sa[1] + x * p.sa[2] + c * p.sa[3]];
            vb = b[r * p.sb[1] + x * p.sb[2] + c * p.sb[3]];
            if (r < own_h && x < own_w) {
                if constexpr (kFloat) {
                    const double d = (double)va - (double)vb;
                    d1 += fabs(d);
                    d2 += d * d;
                } else {
                    const int d = va - vb;
                    d1 += (unsigned)abs(d);
                    d2 += (unsigned)(d * d);
                }
            }
        }
        tile_a[c * PLANE + r * IM_HALO + x] = va;
        tile_b[c * PLANE + r * IM_HALO + x] = vb;
    }
    __syncthreads();

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wx = threadIdx.x % IM_T, g = threadIdx.x / IM_T;      // this thread's window column and row group
    const int valid_h = p.H - (IM_WIN - 1) - y0, valid_w = p.W - (IM_WIN - 1) - x0;      // window origins inside: row < valid_h, column < valid_w
#pragma unroll 1      // (one channel's 20 accumulators at a time: unrolled, the channels interleave and the registers run out)
    for (int c = 0; c < C; ++c) {
        const word *pa = tile_a + c * PLANE, *pb = tile_b + c * PLANE;
        word shift_a = 0, shift_b = 0;
        if constexpr (kFloat) {      // the mean of an 8x8 sample of the in-image halo, formed by every wave alike
            const int o = ((lane >> 3) * in_h / 8) * IM_HALO + (lane & 7) * in_w / 8;
            float ma = pa[o], mb = pb[o];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) { ma += __shfl_xor(ma, off, 64); mb += __shfl_xor(mb, off, 64); }
            shift_a = ma * (1.0f / 64.0f);
            shift_b = mb * (1.0f / 64.0f);
        }
        acc sx[IM_ROWS] = {}, sy[IM_ROWS] = {}, sxx[IM_ROWS] = {}, syy[IM_ROWS] = {}, sxy[IM_ROWS] = {};
#pragma unroll
        for (int r = 0; r < IM_ROWS + IM_WIN - 1; ++r) {
            const word *ra = pa + (IM_ROWS * g + r) * IM_HALO + wx, *rb = pb + (IM_ROWS * g + r) * IM_HALO + wx;
            acc rx = 0, ry = 0, rxx = 0, ryy = 0, rxy = 0;
#pragma unroll
            for (int k = 0; k < IM_WIN; ++k) {
                const acc x = (acc)ra[k] - (acc)shift_a, y = (acc)rb[k] - (acc)shift_b;      // (exact in float64: centring costs no rounding)
                rx += x;
                ry += y;
                rxx += x * x;
                ryy += y * y;
                rxy += x * y;
            }
#pragma unroll
            for (int j = 0; j < IM_ROWS; ++j)
                if (r >= j && r < j + IM_WIN) { sx[j] += rx; sy[j] += ry; sxx[j] += rxx; syy[j] += ryy; sxy[j] += rxy; }
        }
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < IM_ROWS; ++j) {
            const acc nx = 49 * sxx[j] - sx[j] * sx[j], ny = 49 * syy[j] - sy[j] * sy[j], nxy = 49 * sxy[j] - sx[j] * sy[j];
            const double mx = 49.0 * (double)shift_a + (double)sx[j], my = 49.0 * (double)shift_b + (double)sy[j];
            const double S = ((2.0 * mx * my + p.K1) * (2.0 * (double)nxy + p.K2)) / ((mx * mx + my * my + p.K1) * ((double)nx + (double)ny + p.K2));
            if (IM_ROWS * g + j < valid_h && wx < valid_w) s += S;
        }
        s = wave_sum_f64(s);
        if (lane == 0) red[wave][c] = s;
    }

    // ---- the workgroup's record: lanes by butterfly (above for the channels' S), then the four waves in order ----
    const double w1 = wave_sum_f64((double)d1), w2 = wave_sum_f64((double)d2);
    if (lane == 0) { red[wave][C] = w1; red[wave][C + 1] = w2; }
    __syncthreads();
    if (threadIdx.x < C + 2) {
        double w = red[0][threadIdx.x];
#pragma unroll
        for (int k = 1; k < IM_WAVES; ++k) w += red[k][threadIdx.x];
        p.records[(long)blockIdx.x * (C + 2) + threadIdx.x] = w;
    }
}

// out row of image b: [mean SSIM, MSE, L1, SSIM of channel 0 .. C-1]; MSE and L1 in units of the data range 1 (uint8: x / 255)
__global__ __launch_bounds__(IM_THREADS) void image_metrics_finalize_kernel(const double *records, int tiles, int C, double windows, double pixels,
                                                                            double scale, double *out)
{
    __shared__ double red[IM_WAVES][6];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, K = C + 2;
    const double *rec = records + (long)blockIdx.x * tiles * K;
    for (int k = 0; k < K; ++k) {
        double s = 0.0;
        for (int t = threadIdx.x; t < tiles; t += IM_THREADS) s += rec[(long)t * K + k];
        s = wave_sum_f64(s);
        if (lane == 0) red[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot[6];
        for (int k = 0; k < K; ++k) tot[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
        double *o = out + (long)blockIdx.x * (3 + C);
        double mean = 0.0;
        for (int c = 0; c < C; ++c) {
            o[3 + c] = tot[c] / windows;
            mean += o[3 + c];
        }
        o[0] = mean / C;
        o[1] = tot[C + 1] / (pixels * scale * scale);
        o[2] = tot[C] / (pixels * scale);
    }
}

template <class T>
static hipError_t tile_launch(int C, unsigned grid, const ImArgs &args, hipStream_t stream)
{
    switch (C) {
    case 1: hipLaunchKernelGGL((image_metrics_tile_kernel<T, 1>), dim3(grid), dim3(IM_THREADS), 0, stream, args); break;
    case 2: hipLaunchKernelGGL((image_metrics_tile_kernel<T, 2>), dim3(grid), dim3(IM_THREADS), 0, stream, args); break;
    case 3: hipLaunchKernelGGL((image_metrics_tile_kernel<T, 3>), dim3(grid), dim3(IM_THREADS), 0, stream, args); break;
    default: hipLaunchKernelGGL((image_metrics_tile_kernel<T, 4>), dim3(grid), dim3(IM_THREADS), 0, stream, args); break;
    }
    return hipGetLastError();
}

}      // namespace sahs

long sahs_image_metrics_tiles(int H, int W)
{
    const long tx = (W - 6 + sahs::IM_T - 1) / sahs::IM_T, ty = (H - 6 + sahs::IM_T - 1) / sahs::IM_T;
    return tx * ty;
}

// arguments already validated (capi.hip): 7 <= H, W; 1 <= C <= 4; B * tiles < 2^31
int sahs_image_metrics_launch(const void *a, const void *b, int is_float, long B, int H, int W, int C, const long *stride_a,
                              const long *stride_b, double ssim_data_range, double *out, double *records, hipStream_t stream)
{
    using namespace sahs;
    ImArgs args;
    args.a = a;
    args.b = b;
    for (int k = 0; k < 4; ++k) { args.sa[k] = stride_a[k]; args.sb[k] = stride_b[k]; }
    args.H = H;
    args.W = W;
    args.tiles_x = (W - 6 + IM_T - 1) / IM_T;
    args.tiles_y = (H - 6 + IM_T - 1) / IM_T;
    args.c_fastest = stride_a[3] <= stride_a[2];
    const double scale = is_float ? 1.0 : 255.0, C1 = 0.01 * ssim_data_range, C2 = 0.03 * ssim_data_range;
    args.K1 = 49.0 * 49.0 * C1 * C1 * scale * scale;
    args.K2 = 49.0 * 48.0 * C2 * C2 * scale * scale;
    args.records = records;
    const int tiles = args.tiles_x * args.tiles_y;
    const unsigned grid = (unsigned)(B * tiles);
    hipError_t e = is_float ? tile_launch<float>(C, grid, args, stream) : tile_launch<uint8_t>(C, grid, args, stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(image_metrics_finalize_kernel, dim3((unsigned)B), dim3(IM_THREADS), 0, stream, records, tiles, C,
                       (double)(H - 6) * (double)(W - 6), (double)H * (double)W * (double)C, scale, out);
    return (int)hipGetLastError();
}
