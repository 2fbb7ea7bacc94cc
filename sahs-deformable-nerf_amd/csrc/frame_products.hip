// frame_products.hip -- what Stage-I evaluation writes to disk for a rendered frame, as bytes, in two launches per call whatever the
// batch (evaluation.py: cast_to_image, label2color, normal_map, cast_to_disparity_image are the statement this is held to):
//   TILE kernel      a workgroup owns one FP_T x FP_T block of pixels of one frame and walks it in strips of FP_ROWS rows, a pixel per
//                    thread.  Per strip it reads the strip's rgb rows (60 bytes per pixel for the renderer's [rgb3 | seg12] layout) as
//                    consecutive dwords into LDS, lets each thread pick its pixel there, and forms the image bytes (clamp, x255,
//                    truncate), the mask bytes (colour of the arg-max class) and the normal (back-projection of the disparity tile and
//                    its d-wide halo to the right and below, staged once in LDS; row and column differences; cross product; normalise;
//                    whiten / blend by the background weight).  Bytes leave through LDS: a row of a tile is <= 96 bytes that start
//                    at any byte address (frame b's plane starts at b*H*W*3), so each row is laid out in LDS at its global address's
//                    offset in a dword, whole dwords inside the row go out as dword stores and the <= 3 bytes at either end as byte
//                    stores (a neighbouring tile or frame owns the rest of those dwords).  It also leaves one record per tile:
//                    [min, max, saw-NaN] of the disparity pixels it owns.
//   DISPARITY kernel every workgroup of a frame reduces that frame's records (min and max are exact in any order), then maps its share
//                    of the plane: (t - min) / (max - min) as an fp32 subtraction and a correctly rounded fp32 division, clamp, x255,
//                    truncate; four pixels per thread, one dword store, head and tail of the frame's plane as byte stores.
// No atomics and no completion counter; a batch gives the bits of its single calls.
// Arithmetic: every step is ONE correctly rounded fp32 operation in the order evaluation.py writes it (the build keeps -ffp-contract=off),
// so the planes differ from torch's on the CPU only where its kernels contract or reorder.
// NaN rule: a NaN that reaches a byte conversion is stored as 0 (torch leaves that conversion undefined).  The min / max of the
// disparity propagate NaN as torch.min / torch.max do -- the hardware's v_min / v_max return the other operand -- through the record's
// third word: a frame with one NaN has min = max = NaN and so an all-zero plane; a constant frame (0 / 0) likewise.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "sahs_common.hpp"
#include "sahs_launchers.hpp"
#include "../../include/sahs_nerf.h"

namespace sahs {

constexpr int FP_T = SAHS_FRAME_PRODUCTS_TILE, FP_THREADS = 256, FP_WAVES = FP_THREADS / 64, FP_ROWS = FP_THREADS / FP_T, FP_STRIPS = FP_T / FP_ROWS;
constexpr int FP_HALO = FP_T + 2;      // the disparity tile and its halo at d = 2
constexpr int FP_ROW_BYTES = FP_T * 3, FP_ROW_DWORDS = (FP_ROW_BYTES + 3 + 3) / 4, FP_PITCH = FP_ROW_DWORDS * 4;      // a row at any offset 0 .. 3 in a dword
static_assert(FP_T == 32 && FP_ROWS == 8 && FP_ROWS * FP_ROW_DWORDS <= FP_THREADS, "a thread per pixel of a strip, and per dword of its byte rows");

struct FpArgs {
    const float *rgb, *disp, *w_bg;
    long srgb[3];      // element strides of rgb: batch, row, column (channel: 1)
    int H, W, tiles_x, tiles_y, d, clean;
    float fx, fy, cxw, cyh;      // cxw = cx * W, cyh = cy * H: one fp32 product each, as evaluation.normal_map forms them
    uint8_t *image, *seg, *normals_u8, *disparity;
    float *normals_f32;
    float4 *records;
};

// class index -> colour byte: evaluation.SEG_COLOURS.  The torch path writes trunc(fl(fl(c / 255) * 255)), which is c for each of these
// (formed the same way here, at compile time, so the table states that rather than assumes it).
constexpr uint8_t seg_byte(int c) { return (uint8_t)(((float)c / 255.0f) * 255.0f); }
__constant__ const uint8_t FP_SEG[12][3] = {
    {seg_byte(0), seg_byte(0), seg_byte(0)}, {seg_byte(0), seg_byte(0), seg_byte(204)}, {seg_byte(0), seg_byte(153), seg_byte(76)},
    {seg_byte(0), seg_byte(204), seg_byte(204)}, {seg_byte(255), seg_byte(51), seg_byte(51)}, {seg_byte(255), seg_byte(255), seg_byte(0)},
    {seg_byte(0), seg_byte(51), seg_byte(102)}, {seg_byte(0), seg_byte(204), seg_byte(102)}, {seg_byte(0), seg_byte(255), seg_byte(255)},
    {seg_byte(204), seg_byte(0), seg_byte(0)}, {seg_byte(51), seg_byte(153), seg_byte(255)}, {seg_byte(0), seg_byte(204), seg_byte(0)}};

// clamp(v, 0, hi) * scale truncated to a byte, as torch's clamp, product and conversion; NaN -> 0, spelled out (fminf / fmaxf return
// the other operand for a NaN, which would be 0 only by the choice of the lower bound)
__device__ __forceinline__ uint8_t to_byte(float v, float hi, float scale)
{
    if (v != v) return 0;
    return (uint8_t)(int)(fminf(fmaxf(v, 0.0f), hi) * scale);
}

// Rows of <= FP_ROW_BYTES bytes from their LDS image to global memory.  Row r starts at g0 + r * pitch (any byte address); in LDS it
// sits at s + r * FP_PITCH + (that address & 3), so LDS dword k of the row is global dword (address & ~3) + 4k.  One thread per dword.
__device__ __forceinline__ void store_byte_rows(const uint8_t *s, uint8_t *g0, long pitch, int rows, int nbytes)
{
    const int r = threadIdx.x / FP_ROW_DWORDS, k = threadIdx.x % FP_ROW_DWORDS;
    if (r < rows) {
        uint8_t *g = g0 + (long)r * pitch;
        const int lo = 4 * k - (int)(reinterpret_cast<uintptr_t>(g) & 3u);      // this dword's first byte, relative to the row's
        const uint8_t *src = s + r * FP_PITCH + 4 * k;
        if (lo >= 0 && lo + 4 <= nbytes) {
            *reinterpret_cast<uint32_t *>(g + lo) = *reinterpret_cast<const uint32_t *>(src);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (lo + j >= 0 && lo + j < nbytes) g[lo + j] = src[j];
        }
    }
}

template <int C>
__global__ __launch_bounds__(FP_THREADS) void frame_products_tile_kernel(FpArgs p)
{
    __shared__ float s_rgb[FP_ROWS * FP_T * C];
    __shared__ float s_disp[FP_HALO * FP_HALO];
    __shared__ float s_nf[FP_ROWS * FP_T * 3];
    __shared__ __attribute__((aligned(4))) uint8_t s_img[FP_ROWS * FP_PITCH], s_seg[FP_ROWS * FP_PITCH], s_nrm[FP_ROWS * FP_PITCH];
    __shared__ float s_red[FP_WAVES][3];

    const int tiles = p.tiles_x * p.tiles_y;
    const long b = blockIdx.x / tiles;
    const int tile = blockIdx.x % tiles, ty = tile / p.tiles_x, tx = tile % p.tiles_x;
    const int y0 = ty * FP_T, x0 = tx * FP_T, H = p.H, W = p.W, d = p.d;
    const int th = min(FP_T, H - y0), tw = min(FP_T, W - x0);      // this tile's pixels (>= 1 each)
    const int Hn = H - d, Wn = W - d;      // the normal plane
    const int nh = max(0, min(FP_T, Hn - y0)), nw = max(0, min(FP_T, Wn - x0));      // this tile's part of it
    const bool want_rgb = p.image != nullptr || p.seg != nullptr;
    const bool want_n = (p.normals_u8 != nullptr || p.normals_f32 != nullptr) && nh > 0 && nw > 0;
    const int lx = threadIdx.x % FP_T, lr = threadIdx.x / FP_T;

    // ---- the disparity tile with its halo to the right and below (inside the frame; what lies outside feeds no pixel of a plane) ----
    if (p.disp != nullptr) {
        const float *dp = p.disp + (b * H + y0) * (long)W + x0;
        const int hh = min(FP_T + d, H - y0), hw = min(FP_T + d, W - x0);
        for (int i = threadIdx.x; i < FP_HALO * FP_HALO; i += FP_THREADS) {
            const int r = i / FP_HALO, x = i % FP_HALO;
            s_disp[i] = r < hh && x < hw ? dp[(long)r * W + x] : 0.0f;
        }
    }

    float mn = __builtin_inff(), mx = -__builtin_inff();
    int saw_nan = 0;
#pragma unroll 1
    for (int strip = 0; strip < FP_STRIPS; ++strip) {
        const int r0 = strip * FP_ROWS;      // first tile row of the strip
        if (r0 >= th) break;      // (uniform over the workgroup)
        const int rows = min(FP_ROWS, th - r0);
        // ---- stage the strip's rgb rows: lane j of a row reads dword j of its tw * C (contiguous when the column stride is C) ----
        if (want_rgb) {
            const float *rp = p.rgb + b * p.srgb[0] + (long)(y0 + r0) * p.srgb[1] + (long)x0 * p.srgb[2];
            for (int r = 0; r < rows; ++r)
                for (int j = threadIdx.x; j < tw * C; j += FP_THREADS)
                    s_rgb[r * (FP_T * C) + j] = rp[r * p.srgb[1] + (j / C) * p.srgb[2] + (j % C)];
        }
        __syncthreads();      // s_rgb (and, in the first strip, s_disp) written; the previous strip's byte rows stored

        const int y = y0 + r0 + lr, x = x0 + lx;
        const bool inside = lr < rows && lx < tw;
        if (inside && want_rgb) {
            const float *px = s_rgb + (lr * FP_T + lx) * C;
            if (p.image != nullptr) {
                const int o = lr * FP_PITCH + (int)(reinterpret_cast<uintptr_t>(p.image + ((b * H + y) * (long)W + x0) * 3) & 3u) + lx * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) s_img[o + c] = to_byte(px[c], 1.0f, 255.0f);
            }
            if constexpr (C == 15) {
                if (p.seg != nullptr) {
                    // numpy's argmax: the first maximum wins, a NaN counts as the maximum (so the first NaN wins)
                    int best = 0;
                    float bv = px[3];
#pragma unroll
                    for (int c = 1; c < 12; ++c) {
                        const float v = px[3 + c];
                        if (bv == bv && (v > bv || v != v)) { bv = v; best = c; }
                    }
                    const int o = lr * FP_PITCH + (int)(reinterpret_cast<uintptr_t>(p.seg + ((b * H + y) * (long)W + x0) * 3) & 3u) + lx * 3;
#pragma unroll
                    for (int c = 0; c < 3; ++c) s_seg[o + c] = FP_SEG[best][c];
                }
            }
        }
        if (inside && p.disp != nullptr) {
            const float t = s_disp[(r0 + lr) * FP_HALO + lx];
            if (t != t) saw_nan = 1;
            else { mn = fminf(mn, t); mx = fmaxf(mx, t); }
        }
        if (want_n && r0 + lr < nh && lx < nw) {
            // evaluation.normal_map, operation by operation: pts = [((col - cx W) t) / fx, -((row - cy H) t) / fy, t]
            const float *sd = s_disp + (r0 + lr) * FP_HALO + lx;
            const float t0 = sd[0], tr = sd[d], tb = sd[d * FP_HALO];      // here, d to the right, d below
            const float u0 = (float)x - p.cxw, u1 = (float)(x + d) - p.cxw, v0 = (float)y - p.cyh, v1 = (float)(y + d) - p.cyh;
            const float X0 = (u0 * t0) / p.fx, Y0 = -(v0 * t0) / p.fy;
            const float Xr = (u1 * tr) / p.fx, Yr = -(v0 * tr) / p.fy;
            const float Xb = (u0 * tb) / p.fx, Yb = -(v1 * tb) / p.fy;
            const float a0 = Xr - X0, a1 = Yr - Y0, a2 = tr - t0;      // dy: the column difference
            const float b0 = Xb - X0, b1 = Yb - Y0, b2 = tb - t0;      // dx: the row difference
            float n[3] = {a1 * b2 - a2 * b1, a2 * b0 - a0 * b2, a0 * b1 - a1 * b0};      // cross(dy, dx)
            const float len = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
            float m = 0.0f;
            const bool blend = p.clean && p.w_bg != nullptr;
            if (blend) m = p.w_bg[(b * H + y) * (long)W + x];
            const long gy = b * Hn + y;
            const int o = lr * FP_PITCH + (p.normals_u8 != nullptr ? (int)(reinterpret_cast<uintptr_t>(p.normals_u8 + (gy * Wn + x0) * 3) & 3u) : 0) + lx * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float v = (n[c] / len) * 0.5f + 0.5f;
                if (blend) {
                    if (m > 0.22f) v = 1.0f;
                    v = (1.0f - m) * v + m;
                }
                v = v * 255.0f;
                s_nf[(lr * FP_T + lx) * 3 + c] = v;
                s_nrm[o + c] = to_byte(v, 255.0f, 1.0f);
            }
        }
        __syncthreads();      // the strip's byte rows and normals are in LDS; s_rgb is free for the next strip

        if (p.image != nullptr) store_byte_rows(s_img, p.image + ((b * H + y0 + r0) * (long)W + x0) * 3, (long)W * 3, rows, tw * 3);
        if constexpr (C == 15)
            if (p.seg != nullptr) store_byte_rows(s_seg, p.seg + ((b * H + y0 + r0) * (long)W + x0) * 3, (long)W * 3, rows, tw * 3);
        if (want_n && r0 < nh) {
            const int nrows = min(FP_ROWS, nh - r0);
            const long first = ((b * Hn + y0 + r0) * (long)Wn + x0) * 3;
            if (p.normals_u8 != nullptr) store_byte_rows(s_nrm, p.normals_u8 + first, (long)Wn * 3, nrows, nw * 3);
            if (p.normals_f32 != nullptr)
                for (int r = 0; r < nrows; ++r)
                    for (int j = threadIdx.x; j < nw * 3; j += FP_THREADS)
                        p.normals_f32[first + (long)r * Wn * 3 + j] = s_nf[r * (FP_T * 3) + j];
        }
    }

    // ---- the tile's record: lanes by butterfly, then the four waves ----
    if (p.records != nullptr) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            mn = fminf(mn, __shfl_xor(mn, off, 64));
            mx = fmaxf(mx, __shfl_xor(mx, off, 64));
            saw_nan |= __shfl_xor(saw_nan, off, 64);
        }
        if (lane == 0) { s_red[wave][0] = mn; s_red[wave][1] = mx; s_red[wave][2] = saw_nan ? 1.0f : 0.0f; }
        __syncthreads();
        if (threadIdx.x == 0) {
            float4 rec = make_float4(s_red[0][0], s_red[0][1], s_red[0][2], 0.0f);
#pragma unroll
            for (int k = 1; k < FP_WAVES; ++k) {
                rec.x = fminf(rec.x, s_red[k][0]);
                rec.y = fmaxf(rec.y, s_red[k][1]);
                rec.z = fmaxf(rec.z, s_red[k][2]);
            }
            p.records[blockIdx.x] = rec;
        }
    }
}

// grid: B * chunks workgroups; workgroup (b, chunk) maps dwords chunk * 256 + thread, + chunks * 256, ... of frame b's byte plane
__global__ __launch_bounds__(FP_THREADS) void frame_products_disparity_kernel(const float *disp, const float4 *records, int tiles, long hw, int chunks,
                                                                              uint8_t *out)
{
    __shared__ float s_red[FP_WAVES][3];
    const long b = blockIdx.x / chunks;
    const int chunk = blockIdx.x % chunks, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float mn = __builtin_inff(), mx = -__builtin_inff(), nan = 0.0f;
    for (int t = threadIdx.x; t < tiles; t += FP_THREADS) {
        const float4 rec = records[b * tiles + t];
        mn = fminf(mn, rec.x);
        mx = fmaxf(mx, rec.y);
        nan = fmaxf(nan, rec.z);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, off, 64));
        mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        nan = fmaxf(nan, __shfl_xor(nan, off, 64));
    }
    if (lane == 0) { s_red[wave][0] = mn; s_red[wave][1] = mx; s_red[wave][2] = nan; }
    __syncthreads();
    mn = fminf(fminf(s_red[0][0], s_red[1][0]), fminf(s_red[2][0], s_red[3][0]));
    mx = fmaxf(fmaxf(s_red[0][1], s_red[1][1]), fmaxf(s_red[2][1], s_red[3][1]));
    nan = fmaxf(fmaxf(s_red[0][2], s_red[1][2]), fmaxf(s_red[2][2], s_red[3][2]));
    if (nan != 0.0f) mn = mx = __builtin_nanf("");      // torch.min / torch.max of a frame that holds a NaN
    const float range = mx - mn;

    const float *src = disp + b * hw;
    uint8_t *dst = out + b * hw;
    const int mis = (int)(reinterpret_cast<uintptr_t>(dst) & 3u);
    const long dwords = (hw + mis + 3) / 4;
    for (long q = (long)chunk * FP_THREADS + threadIdx.x; q < dwords; q += (long)chunks * FP_THREADS) {
        const long first = 4 * q - mis;      // pixel of this dword's first byte
        uint32_t word = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long i = first + j;
            if (i >= 0 && i < hw) {
                const float v = (src[i] - mn) / range;
                word |= (uint32_t)to_byte(v, 1.0f, 255.0f) << (8 * j);
            }
        }
        if (first >= 0 && first + 4 <= hw) {
            *reinterpret_cast<uint32_t *>(dst + first) = word;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (first + j >= 0 && first + j < hw) dst[first + j] = (uint8_t)(word >> (8 * j));
        }
    }
}

}      // namespace sahs

long sahs_frame_products_tiles(int H, int W)
{
    return (long)((H + sahs::FP_T - 1) / sahs::FP_T) * (long)((W + sahs::FP_T - 1) / sahs::FP_T);
}

// arguments already validated (capi.hip): 1 <= H, W <= 32768; B >= 1; B * tiles < 2^31; C is 3 or 15; pointers null where a plane is
// not asked for (normals: also where the plane is empty); records non-null exactly when disparity is
int sahs_frame_products_launch(const float *rgb, int C, const long *stride_rgb, const float *disp, const float *w_bg, const float *intrinsics,
                               long B, int H, int W, int clean, int central_difference, uint8_t *image, uint8_t *seg, uint8_t *normals_u8,
                               float *normals_f32, uint8_t *disparity, void *records, hipStream_t stream)
{
    using namespace sahs;
    FpArgs args;
    args.rgb = rgb;
    args.disp = disp;
    args.w_bg = w_bg;
    for (int k = 0; k < 3; ++k) args.srgb[k] = stride_rgb ? stride_rgb[k] : 0;
    args.H = H;
    args.W = W;
    args.tiles_x = (W + FP_T - 1) / FP_T;
    args.tiles_y = (H + FP_T - 1) / FP_T;
    args.d = central_difference ? 2 : 1;
    args.clean = clean != 0;
    args.fx = intrinsics ? intrinsics[0] : 1.0f;
    args.fy = intrinsics ? intrinsics[1] : 1.0f;
    args.cxw = intrinsics ? intrinsics[2] * (float)W : 0.0f;
    args.cyh = intrinsics ? intrinsics[3] * (float)H : 0.0f;
    args.image = image;
    args.seg = seg;
    args.normals_u8 = normals_u8;
    args.normals_f32 = normals_f32;
    args.disparity = disparity;
    args.records = disparity ? static_cast<float4 *>(records) : nullptr;
    const int tiles = args.tiles_x * args.tiles_y;
    if (image || seg || normals_u8 || normals_f32 || disparity) {
        const unsigned grid = (unsigned)(B * tiles);
        if (C == 15) hipLaunchKernelGGL((frame_products_tile_kernel<15>), dim3(grid), dim3(FP_THREADS), 0, stream, args);
        else hipLaunchKernelGGL((frame_products_tile_kernel<3>), dim3(grid), dim3(FP_THREADS), 0, stream, args);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    if (disparity) {
        const long hw = (long)H * W, dwords = (hw + 3 + 3) / 4;
        long chunks = (dwords + FP_THREADS - 1) / FP_THREADS;
        const long cap = 2147483647L / B < 1024 ? 2147483647L / B : 1024;      // (B * tiles < 2^31 and tiles >= 1: cap >= 1)
        if (chunks > cap) chunks = cap;
        hipLaunchKernelGGL(frame_products_disparity_kernel, dim3((unsigned)(B * chunks)), dim3(FP_THREADS), 0, stream, disp,
                           static_cast<const float4 *>(records), tiles, hw, (int)chunks, disparity);
    }
    return (int)hipGetLastError();
}
