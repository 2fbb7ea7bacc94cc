// image_loss.hip -- the refiner's objective and its gradient in one pass:
//   loss = w_l2 MSE(x, t) + w_l1 L1(x, t) + w_ssim (1 - SSIM(x, t)),   x = clamp(pred, 0, 1) or pred,
// with image_metrics.hip's SSIM (7x7 box window, sample covariance, mean over the windows inside the image, then channels).  Two launches
// per call, whatever the batch:
//   TILE kernel      a workgroup owns one IL_T x IL_T block of PIXELS of one image, and the windows whose origins are those pixels.  A
//                    pixel's SSIM gradient gathers from the 49 windows that contain it, so the workgroup recomputes the windows on the
//                    halo of origins its pixels need -- IL_T + 6 per side, from IL_T + 12 of pixels -- instead of scattering with
//                    atomics.  Per channel: stage x and t (fp32, zero outside the image), form the five centred 7x7 moments
//                    separably in registers as image_metrics_tile_kernel does (a thread walks 13 halo rows of one column, sums 7 taps per
//                    row and adds the row sums into its 7 windows), evaluate S and the three coefficients of
//                        dS/dx_p = alpha_w + beta_w x_p + gamma_w y_p
//                    per window into LDS, box-sum them separably over the 7x7 origins of each pixel (7 taps per row, 7 rows) and write
//                        g_p = mask_p (2 w_l2 d_p + w_l1 sign(d_p)) / (H W C) - w_ssim (box alpha + x_p box beta + y_p box gamma) / (C (H-6)(W-6)),
//                    once, from one thread.  One record of doubles per (image, tile): [sum S per channel, sum |d|, sum d^2].
//   FINALIZE kernel  one workgroup: a wave per image adds that image's records in a fixed order in float64 into its row
//                    [MSE, L1, mean SSIM]; then one thread averages the rows in image order into [loss, MSE, L1, mean SSIM].
// The gradient is that of ONE image's loss (no 1 / B in it): the kernels never see B in their arithmetic, so a batch gives the bits of
// its single calls, loss rows and gradient alike; the caller's backward scales by grad_out / B.  No atomics, every sum in a fixed order.
// A null gradient pointer skips the gradient's work -- the halo of origins above and left of the tile is neither read nor evaluated --
// and leaves every loss bit as it is with one: the owned windows are evaluated by the same threads from the same shift.  With
// w_ssim == 0 the halo, the coefficients and the box sums are skipped as well: the gradient is the pixel's own MSE and L1 terms.
// Numerics.  The moments are centred on a per-tile, per-channel shift (the mean of an 8x8 sample of the tile's own
// pixels), x' = x - shift is exact in float64 and every sum runs in float64.  S is invariant under the shift, and so are beta and gamma;
// alpha is formed in the shifted frame, alpha' = (dS/dmu_x) / 49 - beta mu_x' - gamma mu_y', so that alpha' + beta x'_p + gamma y'_p adds
// small terms where alpha + beta x_p + gamma y_p would cancel on bright flat regions.  The gradient is rounded to fp32 once.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "sahs_common.hpp"
#include "sahs_launchers.hpp"
#include "../../include/sahs_nerf.h"

namespace sahs {

constexpr int IL_T = SAHS_IMAGE_LOSS_TILE, IL_WIN = 7, IL_PAD = IL_WIN - 1, IL_THREADS = 256, IL_WAVES = IL_THREADS / 64;
constexpr int IL_ORG = IL_T + IL_PAD;      // origins per side: the windows that contain a pixel of the tile
constexpr int IL_ROWS = 7;      // windows per thread in the moment pass: rows 7g .. 7g+6 of one column, from pixel rows 7g .. 7g+12
constexpr int IL_GROUPS = (IL_ORG + IL_ROWS - 1) / IL_ROWS;
constexpr int IL_PW = IL_ORG + IL_PAD, IL_PH = IL_GROUPS * IL_ROWS + IL_PAD;      // the staged pixel plane (rows past IL_PW: zero, read by no valid window)
constexpr int IL_BOX = 4;      // pixels per thread in the box pass: rows 4g .. 4g+3 of one column, from origin rows 4g .. 4g+9
static_assert(IL_ORG * IL_GROUPS <= IL_THREADS, "moment pass: a thread per (origin column, group of IL_ROWS rows)");
static_assert(IL_T * (IL_T / IL_BOX) == IL_THREADS && IL_T % IL_BOX == 0, "box pass: a thread per (pixel column, group of IL_BOX rows)");
static_assert(2 * IL_PW * IL_PH * 4 + 3 * IL_ORG * IL_ORG * 8 + IL_WAVES * 6 * 8 <= 65536, "LDS: two pixel planes, three coefficient planes");
constexpr int IL_FIN_THREADS = 1024;

struct IlArgs {
    const float *pred, *target;
    float *grad;      // null: no gradient work
    long sp[4], st[4], sg[4];      // element strides: batch, row, column, channel
    int H, W, C, tiles_x, tiles_y, clamp;
    double C1, C2;
    double g_l2, g_l1, g_ssim;      // 2 w_l2 / (H W C), w_l1 / (H W C), -w_ssim / (C (H-6)(W-6))
    double *records;
};

__device__ __forceinline__ double il_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(IL_THREADS) void image_loss_tile_kernel(IlArgs p)
{
    __shared__ float px[IL_PH * IL_PW], pt[IL_PH * IL_PW];      // x (clamped) and t of one channel; plane (r, c) is pixel (y0 - 6 + r, x0 - 6 + c)
    __shared__ double coef[3][IL_ORG * IL_ORG];      // alpha', beta, gamma of origin (y0 - 6 + r, x0 - 6 + c); 0 where the window is not inside the image
    __shared__ double red[IL_WAVES][6];

    const int tiles = p.tiles_x * p.tiles_y;
    const long img = blockIdx.x / tiles;
    const int tile = blockIdx.x % tiles, ty = tile / p.tiles_x, tx = tile % p.tiles_x;
    const int y0 = ty * IL_T, x0 = tx * IL_T;
    const int own_h = min(IL_T, p.H - y0), own_w = min(IL_T, p.W - x0);      // the pixels this tile owns (>= 1 each)
    const int in_h = min(IL_T + IL_PAD, p.H - y0), in_w = min(IL_T + IL_PAD, p.W - x0);      // the image below and right of (y0, x0) that is staged
    const bool want_grad = p.grad != nullptr;
    const bool want_box = want_grad && p.g_ssim != 0.0;      // the windows around the tile serve SSIM's gradient alone: a zero weight skips them
    const float *pred = p.pred + img * p.sp[0], *target = p.target + img * p.st[0];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // moment pass: this thread's origin column and row group; box pass: its pixel column and row group
    const int ox = threadIdx.x % IL_ORG, og = threadIdx.x / IL_ORG;
    const int bx = threadIdx.x % IL_T, bg = threadIdx.x / IL_T;
    const int valid_h = p.H - IL_PAD, valid_w = p.W - IL_PAD;      // window origins inside the image: row < valid_h, column < valid_w

    double d1 = 0.0, d2 = 0.0;
#pragma unroll 1      // (one channel's 35 accumulators at a time, as in image_metrics_tile_kernel)
    for (int c = 0; c < p.C; ++c) {
        // ---- stage the channel: x = clamp(pred), t; zero outside the image and, where SSIM's gradient is not formed, above and left of the tile ----
        for (int i = threadIdx.x; i < IL_PH * IL_PW; i += IL_THREADS) {
            const int r = i / IL_PW, k = i % IL_PW;
            const int gy = y0 - IL_PAD + r, gx = x0 - IL_PAD + k;
            float vx = 0.0f, vt = 0.0f;
            if (r < IL_PW && gy >= 0 && gy < p.H && gx >= 0 && gx < p.W && (want_box || (r >= IL_PAD && k >= IL_PAD))) {
                const float v = pred[gy * p.sp[1] + gx * p.sp[2] + c * p.sp[3]];
                vx = p.clamp ? (v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v)) : v;      // (a NaN stays a NaN, as torch.clamp leaves it)
                vt = target[gy * p.st[1] + gx * p.st[2] + c * p.st[3]];
                if (r >= IL_PAD && r < IL_PAD + own_h && k >= IL_PAD && k < IL_PAD + own_w) {
                    const double d = (double)vx - (double)vt;
                    d1 += fabs(d);
                    d2 += d * d;
                }
            }
            px[i] = vx;
            pt[i] = vt;
        }
        __syncthreads();

        // ---- the shift: the mean of an 8x8 sample of the staged pixels from (y0, x0) on, formed by every wave alike ----
        double shift_x, shift_t;
        {
            const int o = (IL_PAD + (lane >> 3) * in_h / 8) * IL_PW + IL_PAD + (lane & 7) * in_w / 8;
            float mx = px[o], mt = pt[o];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) { mx += __shfl_xor(mx, off, 64); mt += __shfl_xor(mt, off, 64); }
            mx *= 1.0f / 64.0f;
            mt *= 1.0f / 64.0f;
            shift_x = (mx == mx && fabsf(mx) <= 3.0e38f) ? (double)mx : 0.0;      // (any finite value is a valid shift)
            shift_t = (mt == mt && fabsf(mt) <= 3.0e38f) ? (double)mt : 0.0;
        }

        // ---- moments, S and the coefficients of the origins (7 og + j, ox) ----
        double s = 0.0;
        if (og < IL_GROUPS && (want_box || ox >= IL_PAD)) {
            double sx[IL_ROWS] = {}, sy[IL_ROWS] = {}, sxx[IL_ROWS] = {}, syy[IL_ROWS] = {}, sxy[IL_ROWS] = {};
#pragma unroll
            for (int r = 0; r < IL_ROWS + IL_PAD; ++r) {
                const float *ra = px + (IL_ROWS * og + r) * IL_PW + ox, *rb = pt + (IL_ROWS * og + r) * IL_PW + ox;
                double rx = 0, ry = 0, rxx = 0, ryy = 0, rxy = 0;
#pragma unroll
                for (int k = 0; k < IL_WIN; ++k) {
                    const double x = (double)ra[k] - shift_x, y = (double)rb[k] - shift_t;      // (exact in float64: centring costs no rounding)
                    rx += x;
                    ry += y;
                    rxx += x * x;
                    ryy += y * y;
                    rxy += x * y;
                }
#pragma unroll
                for (int j = 0; j < IL_ROWS; ++j)
                    if (r >= j && r < j + IL_WIN) { sx[j] += rx; sy[j] += ry; sxx[j] += rxx; syy[j] += ryy; sxy[j] += rxy; }
            }
            const int gx = x0 - IL_PAD + ox;
#pragma unroll
            for (int j = 0; j < IL_ROWS; ++j) {
                const int orow = IL_ROWS * og + j, gy = y0 - IL_PAD + orow;
                const bool valid = orow < IL_ORG && gy >= 0 && gy < valid_h && gx >= 0 && gx < valid_w;
                const double mxs = sx[j] * (1.0 / 49.0), mys = sy[j] * (1.0 / 49.0);      // the means in the shifted frame
                const double mx = shift_x + mxs, my = shift_t + mys;
                const double vx = (sxx[j] - sx[j] * mxs) * (1.0 / 48.0), vy = (syy[j] - sy[j] * mys) * (1.0 / 48.0),
                             vxy = (sxy[j] - sx[j] * mys) * (1.0 / 48.0);
                const double A1 = 2.0 * mx * my + p.C1, A2 = 2.0 * vxy + p.C2, B1 = mx * mx + my * my + p.C1, B2 = vx + vy + p.C2;
                const double iB = 1.0 / (B1 * B2), S = A1 * A2 * iB;
                if (valid && orow >= IL_PAD && ox >= IL_PAD) s += S;      // the windows this tile owns
                if (want_box && orow < IL_ORG) {
                    const double beta = -2.0 * S / (48.0 * B2), gamma = 2.0 * A1 * iB * (1.0 / 48.0);
                    const double alpha = (2.0 * my * A2 * iB - 2.0 * mx * S / B1) * (1.0 / 49.0) - beta * mxs - gamma * mys;
                    coef[0][orow * IL_ORG + ox] = valid ? alpha : 0.0;
                    coef[1][orow * IL_ORG + ox] = valid ? beta : 0.0;
                    coef[2][orow * IL_ORG + ox] = valid ? gamma : 0.0;
                }
            }
        }
        s = il_wave_sum(s);
        if (lane == 0) red[wave][c] = s;

        // ---- the gradient of the pixels (4 bg + j, bx): 7x7 box sums of the coefficients, rows of 7 taps added into 4 pixels ----
        if (want_grad) {
            double ba[IL_BOX] = {}, bb[IL_BOX] = {}, bc[IL_BOX] = {};
            if (want_box) __syncthreads();
#pragma unroll
            for (int r = 0; want_box && r < IL_BOX + IL_PAD; ++r) {
                const int o = (IL_BOX * bg + r) * IL_ORG + bx;
                double ra = 0, rb = 0, rc = 0;
#pragma unroll
                for (int k = 0; k < IL_WIN; ++k) { ra += coef[0][o + k]; rb += coef[1][o + k]; rc += coef[2][o + k]; }
#pragma unroll
                for (int j = 0; j < IL_BOX; ++j)
                    if (r >= j && r < j + IL_WIN) { ba[j] += ra; bb[j] += rb; bc[j] += rc; }
            }
            if (bx < own_w) {
#pragma unroll
                for (int j = 0; j < IL_BOX; ++j) {
                    const int row = IL_BOX * bg + j;
                    if (row < own_h) {
                        const int o = (IL_PAD + row) * IL_PW + IL_PAD + bx;
                        const double x = (double)px[o], t = (double)pt[o], d = x - t;
                        const double sign = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
                        double g = p.g_l2 * d + p.g_l1 * sign;
                        if (want_box) g += p.g_ssim * (ba[j] + (x - shift_x) * bb[j] + (t - shift_t) * bc[j]);
                        if (p.clamp) {      // torch's rule: the gradient passes where 0 <= pred <= 1, both ends included (a NaN passes nothing)
                            const float v = pred[(long)(y0 + row) * p.sp[1] + (long)(x0 + bx) * p.sp[2] + c * p.sp[3]];
                            if (!(v >= 0.0f && v <= 1.0f)) g = 0.0;
                        }
                        p.grad[img * p.sg[0] + (long)(y0 + row) * p.sg[1] + (long)(x0 + bx) * p.sg[2] + c * p.sg[3]] = (float)g;
                    }
                }
            }
        }
        __syncthreads();      // the planes are free for the next channel
    }

    // ---- the workgroup's record: lanes by butterfly (above for the channels' S), then the four waves in order ----
    const double w1 = il_wave_sum(d1), w2 = il_wave_sum(d2);
    if (lane == 0) { red[wave][p.C] = w1; red[wave][p.C + 1] = w2; }
    __syncthreads();
    if ((int)threadIdx.x < p.C + 2) {
        double w = red[0][threadIdx.x];
#pragma unroll
        for (int k = 1; k < IL_WAVES; ++k) w += red[k][threadIdx.x];
        p.records[(long)blockIdx.x * (p.C + 2) + threadIdx.x] = w;
    }
}

// out: [loss, MSE, L1, mean SSIM] of the batch, then one row [MSE, L1, mean SSIM] per image
__global__ __launch_bounds__(IL_FIN_THREADS) void image_loss_finalize_kernel(const double *records, long B, int tiles, int C, double windows, double pixels,
                                                                             double w_l2, double w_l1, double w_ssim, double *out)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, K = C + 2;
    for (long b = wave; b < B; b += IL_FIN_THREADS / 64) {
        const double *rec = records + b * tiles * K;
        double tot[6];
        for (int k = 0; k < K; ++k) {
            double s = 0.0;
            for (int t = lane; t < tiles; t += 64) s += rec[(long)t * K + k];
            tot[k] = il_wave_sum(s);
        }
        if (lane == 0) {
            double mean = 0.0;
            for (int c = 0; c < C; ++c) mean += tot[c] / windows;
            double *o = out + 4 + 3 * b;
            o[0] = tot[C + 1] / pixels;
            o[1] = tot[C] / pixels;
            o[2] = mean / C;
        }
    }
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x == 0) {
        double m[3] = {0.0, 0.0, 0.0};
        for (long b = 0; b < B; ++b)
            for (int k = 0; k < 3; ++k) m[k] += out[4 + 3 * b + k];
        for (int k = 0; k < 3; ++k) m[k] /= (double)B;
        out[0] = w_l2 * m[0] + w_l1 * m[1] + w_ssim * (1.0 - m[2]);
        out[1] = m[0];
        out[2] = m[1];
        out[3] = m[2];
    }
}

}      // namespace sahs

long sahs_image_loss_tiles(int H, int W)
{
    const long tx = (W + sahs::IL_T - 1) / sahs::IL_T, ty = (H + sahs::IL_T - 1) / sahs::IL_T;
    return tx * ty;
}

// arguments already validated (capi.hip): 7 <= H, W; 1 <= C <= 4; 1 <= B; B * tiles < 2^31
int sahs_image_loss_launch(const float *pred, const float *target, long B, int H, int W, int C, const long *stride_pred,
                           const long *stride_target, double w_l2, double w_l1, double w_ssim, int clamp, double ssim_data_range,
                           float *grad, const long *stride_grad, double *out, double *records, hipStream_t stream)
{
    using namespace sahs;
    IlArgs args;
    args.pred = pred;
    args.target = target;
    args.grad = grad;
    for (int k = 0; k < 4; ++k) { args.sp[k] = stride_pred[k]; args.st[k] = stride_target[k]; args.sg[k] = grad ? stride_grad[k] : 0; }
    args.H = H;
    args.W = W;
    args.C = C;
    args.tiles_x = (W + IL_T - 1) / IL_T;
    args.tiles_y = (H + IL_T - 1) / IL_T;
    args.clamp = clamp != 0;
    args.C1 = (0.01 * ssim_data_range) * (0.01 * ssim_data_range);
    args.C2 = (0.03 * ssim_data_range) * (0.03 * ssim_data_range);
    const double pixels = (double)H * (double)W * (double)C, windows = (double)(H - 6) * (double)(W - 6);
    args.g_l2 = 2.0 * w_l2 / pixels;
    args.g_l1 = w_l1 / pixels;
    args.g_ssim = -w_ssim / ((double)C * windows);
    args.records = records;
    const int tiles = args.tiles_x * args.tiles_y;
    hipLaunchKernelGGL(image_loss_tile_kernel, dim3((unsigned)(B * tiles)), dim3(IL_THREADS), 0, stream, args);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(image_loss_finalize_kernel, dim3(1), dim3(IL_FIN_THREADS), 0, stream, records, B, tiles, C, windows, pixels, w_l2, w_l1,
                       w_ssim, out);
    return (int)hipGetLastError();
}
