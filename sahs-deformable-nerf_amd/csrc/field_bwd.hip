// field_bwd.hip -- gradients of the per-sample field (BASELINE.json configs[4]: training step through the HIP ops).
//
// What depends on the model's layout, built once per model (sahs_model.hpp): the small kernels for the positional-encoding, tanh and
// trilinear-grid derivatives, and the two walks over the layers --
//   the per-layer walk over the activations saved by field_forward_f32_kernel<SAVE> (sahs::act layout: one dense [P x width] array per
//   layer): for every dense layer   dW += dY^T X (+ db = column sums of dY, fused),   dX = (dY W) * act'(X)   as one GEMM launch each
//   over all samples of the call.  Not fused across layers: activations and per-layer gradients go through HBM;
//   the fused walk (further down): the data-gradient chain in one kernel, every weight gradient of a part in one job table.
// The GEMM kernels themselves, the job-table launches and the copy / axpy / constant-column helpers read no layout constant: they are
// built once -- the per-layer walk's GEMMs and the helpers in field_bwd_gemm.hip, the fused walk's job-table kernels in
// field_bwd_tn_jobs.hip -- and called here through the launchers of field_bwd_gemm.hpp as sahs::...
// Conventions follow autograd of the reference graph
// (models.py:514-528, modules.py:371-390 / 444-462 / 254-295): the per-frame constant inputs (driving, pose
// encoding) get their weight-column gradients from the bias gradient (their value is the same for every sample:
// dW[:, const] = db (x) c) and their own gradient from W[:, const]^T db.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "sahs_common.hpp"
#include "field_bwd_gemm.hpp"
#include "sahs_launchers.hpp"
#include "sahs_layout.hpp"
#include "bwd_program.hpp"

namespace SAHS_NS {

// ---- positional-encoding backward: d(enc)/d(coord) from the saved sin/cos rows -----------------------------
// enc = [v | sin(2^k v) | cos(2^k v)]_k (nerf_helpers.py:322-349): d sin = 2^k cos, d cos = -2^k sin.
template <int D, int L, int INC>
__device__ __forceinline__ void pe_grad(const float *enc, const float *denc, float *dv)
{
    constexpr int D0 = INC ? D : 0;    // include_input: the raw coordinates come first
#pragma unroll
    for (int a = 0; a < D; ++a) {
        float g = INC ? denc[a] : 0.0f;
#pragma unroll
        for (int k = 0; k < L; ++k) {
            const int si = D0 + 2 * D * k + a, ci = si + D;
            g += (float)(1 << k) * (denc[si] * enc[ci] - denc[ci] * enc[si]);
        }
        dv[a] = g;
    }
}

constexpr int DIN_AMB = 16 * KB_XYZ;             // where the PE(w) part of a DIN_LD-wide row starts

// one coordinate's gradient through its encoding (pe_grad, one axis)
template <int D, int L, int INC>
__device__ __forceinline__ float pe_grad_axis(const float *enc, const float *denc, int a)
{
    constexpr int D0 = INC ? D : 0;
    float g = INC ? denc[a] : 0.0f;
#pragma unroll
    for (int k = 0; k < L; ++k) {
        const int si = D0 + 2 * D * k + a, ci = si + D;
        g += (float)(1 << k) * (denc[si] * enc[ci] - denc[ci] * enc[si]);
    }
    return g;
}

// Per sample: d_in [P x DIN_LD] = gradient wrt [PE(x') blocks | PE(w) blocks] (d_in2, optional: a second contribution, added).  d_xw [P x 4] +=
// dL/dx' through PE63 (the trilinear part was written by grid_backward_kernel), d_w [P x 4] = dL/dw; seam8 (optional): the same as (P,8) rows
// [dx'0 dx'1 dx'2 0 | dw0 dw1 0 0], the form in which the seam gradient leaves the radiance part of a split walk.
// A workgroup takes 64 samples at a time: their gradient rows and saved encodings (contiguous blocks of the planes) come in as coalesced
// 16-byte loads and are parked in LDS; then four threads per sample -- one per coordinate of x', one for w -- walk the octaves.  (Round 4,
// first form: one thread per sample reading its own 384-byte rows, a line per lane and load: 1.5 TB/s of useful bytes, 270 us per step.)
constexpr int EB_SAMPLES = 64, EB_ROW = DIN_LD + 4;      // LDS row stride (floats): 16-byte aligned rows, the four threads of a sample on four banks of their own
__global__ void __launch_bounds__(256) encode_backward_kernel(long P, const float *__restrict__ actbuf, const float *__restrict__ d_in,
                                                              const float *__restrict__ d_in2, float *__restrict__ d_xw, float *__restrict__ d_w,
                                                              float *__restrict__ seam8)
{
    __shared__ __attribute__((aligned(16))) float s_din[EB_SAMPLES * EB_ROW], s_enc[EB_SAMPLES * EB_ROW];
    const int tid = threadIdx.x, sl = tid >> 2, r = tid & 3;
    const long nblk = (P + EB_SAMPLES - 1) / EB_SAMPLES;
    for (long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const long p0 = blk * EB_SAMPLES;
        const int nv = (int)((P - p0 < EB_SAMPLES) ? P - p0 : EB_SAMPLES);
        __syncthreads();      // (the previous block's readers are done)
        for (int i = tid; i < nv * (DIN_LD / 4); i += 256) {
            const int row = i / (DIN_LD / 4), c4 = i - row * (DIN_LD / 4);
            f32x4 v = *reinterpret_cast<const f32x4 *>(d_in + p0 * DIN_LD + 4 * (long)i);
            if (d_in2 != nullptr) {
                const f32x4 u = *reinterpret_cast<const f32x4 *>(d_in2 + p0 * DIN_LD + 4 * (long)i);
                v[0] += u[0]; v[1] += u[1]; v[2] += u[2]; v[3] += u[3];
            }
            *reinterpret_cast<f32x4 *>(s_din + row * EB_ROW + 4 * c4) = v;
        }
        for (int i = tid; i < nv * (4 * KB_XYZ); i += 256) {
            const int row = i / (4 * KB_XYZ), c4 = i - row * (4 * KB_XYZ);
            const f32x4 v = *reinterpret_cast<const f32x4 *>(actbuf + (long)act::PEX * P + p0 * (16 * KB_XYZ) + 4 * (long)i);
            *reinterpret_cast<f32x4 *>(s_enc + row * EB_ROW + 4 * c4) = v;
        }
#if SAHS_MODEL != 2
        for (int i = tid; i < nv * (4 * KB_AMB); i += 256) {
            const int row = i / (4 * KB_AMB), c4 = i - row * (4 * KB_AMB);
            const f32x4 v = *reinterpret_cast<const f32x4 *>(actbuf + (long)act::PEW * P + p0 * (16 * KB_AMB) + 4 * (long)i);
            *reinterpret_cast<f32x4 *>(s_enc + row * EB_ROW + DIN_AMB + 4 * c4) = v;
        }
#endif
        __syncthreads();
        if (sl < nv) {
            const long p = p0 + sl;
            const float *enc = s_enc + sl * EB_ROW, *din = s_din + sl * EB_ROW;
            if (r < 3) {
                const float t = d_xw[p * 4 + r] + pe_grad_axis<3, L_XYZ, 1>(enc, din, r);
                d_xw[p * 4 + r] = t;
                if (seam8 != nullptr) seam8[p * 8 + r] = t;
            } else {
                float gw[2] = {0.0f, 0.0f};
#if SAHS_MODEL != 2
#pragma unroll
                for (int a = 0; a < AMB_DIM; ++a) gw[a] = pe_grad_axis<AMB_DIM, L_AMB, AMB_INC>(enc + DIN_AMB, din + DIN_AMB, a);
#endif
                *reinterpret_cast<f32x4 *>(d_w + p * 4) = f32x4{gw[0], gw[1], 0.0f, 0.0f};
                if (seam8 != nullptr) {
                    seam8[p * 8 + 3] = d_xw[p * 4 + 3];
                    *reinterpret_cast<f32x4 *>(seam8 + p * 8 + 4) = f32x4{gw[0], gw[1], 0.0f, 0.0f};
                }
            }
        }
    }
}

// Trilinear feature-grid backward (ATen grid_sampler_3d backward, align_corners=True, zeros padding; models.py:346-365).
// Half a wave per sample, lane = channel: the 32 channel gradients of one corner are one 128-byte atomic burst into the
// CHANNEL-LAST accumulator d_grid_cl [voxel][32] (transposed into the channel-first parameter gradient afterwards); the
// coordinate gradient is the 32-lane reduction of dg * grid.  Writes d_xw[p][0:3] = trilinear part, [3] = 0.
__global__ void __launch_bounds__(256) grid_backward_kernel(long P, const float *__restrict__ actbuf, const float *__restrict__ d_gridf,
                                                            const float *__restrict__ grid_cl, float *__restrict__ d_grid_cl,
                                                            float *__restrict__ d_xw)
{
    // Consecutive samples are consecutive depths of one ray and a ray crosses a 1/16-wide cell in ~13 of its 128 samples, so each
    // half-wave walks a run of GCH samples and keeps the eight corner contributions of the CURRENT cell in registers, flushing
    // them (one 128-byte atomic burst per corner) only when the cell changes: ~10x fewer atomics than one flush per sample.
    constexpr int GCH = 16;
    const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
    const long wave = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((long)gridDim.x * blockDim.x) >> 6;
    const float R1 = (float)(G_RES - 1);
    auto flush = [&](int key, const float *acc) {
        if (key < 0) return;
        const int xi = (key & 255) - 2, yi = ((key >> 8) & 255) - 2, zi = (key >> 16) - 2;
#pragma unroll
        for (int n = 0; n < 8; ++n) {
            const int cx = xi + (n & 1), cy = yi + ((n >> 1) & 1), cz = zi + (n >> 2);
            if (cx >= 0 && cx < G_RES && cy >= 0 && cy < G_RES && cz >= 0 && cz < G_RES)
                atomicAdd(d_grid_cl + (((long)cz * G_RES + cy) * G_RES + cx) * D_GRID + c, acc[n]);
        }
    };
    for (long chunk = wave * 2 + h; chunk * GCH < P; chunk += nwaves * 2) {
        float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        int cur = -1;
        for (int k = 0; k < GCH; ++k) {
            const long p = chunk * GCH + k;
            const bool live = p < P;
            const long pc = live ? p : P - 1;
            const float *a = actbuf + (long)act::XW * P + pc * 16;
            const float x = a[0], y = a[1], z = a[2];
            const float ix = ((x + 1.0f) / 2.0f) * R1, iy = ((y + 1.0f) / 2.0f) * R1, iz = ((z + 1.0f) / 2.0f) * R1;
            const float fx = floorf(ix), fy = floorf(iy), fz = floorf(iz);
            const float wx0 = (fx + 1.0f) - ix, wx1 = ix - fx, wy0 = (fy + 1.0f) - iy, wy1 = iy - fy, wz0 = (fz + 1.0f) - iz, wz1 = iz - fz;
            const bool ok = live && fx >= -1.0f && fx <= (float)G_RES && fy >= -1.0f && fy <= (float)G_RES && fz >= -1.0f && fz <= (float)G_RES;
            const int xi = ok ? (int)fx : -2, yi = ok ? (int)fy : -2, zi = ok ? (int)fz : -2;
            const int key = ok ? (((zi + 2) << 16) | ((yi + 2) << 8) | (xi + 2)) : -1;
            if (key != cur) {
                flush(cur, acc);
#pragma unroll
                for (int n = 0; n < 8; ++n) acc[n] = 0.0f;
                cur = key;
            }
            const float g = live ? d_gridf[pc * 32 + c] : 0.0f;
            float gix = 0.0f, giy = 0.0f, giz = 0.0f;
#pragma unroll
            for (int n = 0; n < 8; ++n) {
                const int bx = n & 1, by = (n >> 1) & 1, bz = n >> 2;
                const int cx = xi + bx, cy = yi + by, cz = zi + bz;
                const bool in = ok && cx >= 0 && cx < G_RES && cy >= 0 && cy < G_RES && cz >= 0 && cz < G_RES;
                const float wxb = bx ? wx1 : wx0, wyb = by ? wy1 : wy0, wzb = bz ? wz1 : wz0;
                acc[n] += g * ((wxb * wyb) * wzb);
                if (in) {
                    const float t = g * grid_cl[(((long)cz * G_RES + cy) * G_RES + cx) * D_GRID + c];
                    gix += t * (bx ? 1.0f : -1.0f) * wyb * wzb;
                    giy += t * (by ? 1.0f : -1.0f) * wxb * wzb;
                    giz += t * (bz ? 1.0f : -1.0f) * wxb * wyb;
                }
            }
#pragma unroll
            for (int off = 16; off >= 1; off >>= 1) {
                gix += __shfl_xor(gix, off, 64);
                giy += __shfl_xor(giy, off, 64);
                giz += __shfl_xor(giz, off, 64);
            }
            if (live && c == 0) {
                const float sc = R1 / 2.0f;
                *reinterpret_cast<f32x4 *>(d_xw + p * 4) = f32x4{gix * sc, giy * sc, giz * sc, 0.0f};
            }
        }
        flush(cur, acc);
    }
}

// channel-first [32][vox] <-> channel-last [vox][32] (mode 0: dst_cl = src_cf;  mode 1: dst_cf += src_cl, skipping blocks of 32 voxels that
// received no gradient: the rays of a batch cross a few per cent of the grid, and 4 MB of float atomics per walk cost 0.3-1.6 ms)
__global__ void __launch_bounds__(256) grid_transpose_kernel(const float *__restrict__ src, float *__restrict__ dst, int mode)
{
    __shared__ float t[32][33];
    const long vox = (long)G_RES * G_RES * G_RES;
    const long v0 = (long)blockIdx.x * 32;
    const int i = threadIdx.x & 31, j = threadIdx.x >> 5;   // 8 rows per pass
    if (mode == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) { const int ch = j + 8 * r; t[ch][i] = src[(long)ch * vox + v0 + i]; }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) { const int vv = j + 8 * r; dst[(v0 + vv) * 32 + i] = t[i][vv]; }
    } else {
        int any = 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) { const int vv = j + 8 * r; const float v = src[(v0 + vv) * 32 + i]; t[vv][i] = v; any |= (v != 0.0f); }
        if (!__syncthreads_or(any)) return;
#pragma unroll
        for (int r = 0; r < 4; ++r) {      // (both levels' walks add here, possibly at once)
            const int ch = j + 8 * r;
            const float v = t[i][ch];
            if (v != 0.0f) atomicAdd(dst + (long)ch * vox + v0 + i, v);
        }
    }
}

// g3[p][i] = d_xw[p][i] * (1 - dx_i^2)   (x' = x + tanh(.), models.py:304-305)
__global__ void tanh_backward_kernel(long P, const float *__restrict__ actbuf, const float *__restrict__ d_xw, float *__restrict__ g3)
{
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < P; p += (long)gridDim.x * blockDim.x) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const float dx = actbuf[(long)act::DX * P + p * 16 + i];
            g3[p * 4 + i] = d_xw[p * 4 + i] * (1.0f - dx * dx);
        }
        g3[p * 4 + 3] = 0.0f;
    }
}

}  // namespace SAHS_NS

using namespace SAHS_NS;
// job types and limits of the built-once launchers (field_bwd_gemm.hpp); the launchers themselves are called as sahs::...
using sahs::GT; using sahs::GK; using sahs::TnList;
using sahs::CopyJob; using sahs::CopyBatch; using sahs::MAX_COPY_JOBS;
using sahs::ConstJob; using sahs::ConstBatch; using sahs::MAX_CONST_JOBS;
using sahs::AxpyJob; using sahs::AxpyBatch; using sahs::MAX_AXPY_JOBS;

// Precision of the backward GEMMs of this model build: 0 = f32 MFMA (exact products), 3 = bf16 pipe with split operands (default;
// SAHS_BWD_GEMM=f32 in the environment selects 0 at first use).  set < 0 queries.  Process-wide (one atomic), set through
// sahs_backward_gemm_precision() of the C ABI.
extern "C" int SAHS_SYM(sahs_bwd_gemm_precision_state)(int set)
{
    static std::atomic<int> state{-1};
    int cur = state.load(std::memory_order_relaxed);
    if (cur < 0) {
        const char *e = getenv("SAHS_BWD_GEMM");
        cur = (e != nullptr && e[0] == 'f') ? 0 : 3;
        state.store(cur, std::memory_order_relaxed);
    }
    if (set >= 0) { state.store(set ? 3 : 0, std::memory_order_relaxed); cur = set ? 3 : 0; }
    return cur;
}

namespace {

struct Bwd {
    hipStream_t st;
    long P;
    const float *zero;     // 16-byte zero page (DMA source for out-of-range tile rows/columns)
    float *wal;            // scratch for 16-byte aligned copies of weight sub-matrices (the flat parameter buffer is not aligned)
    long wal_cap = 0;
    long walo = 0;
    int err = 0;
    unsigned char *sign_bits = nullptr;      // P x 32 bytes: the bit matrix of the activation the last tn() staged as its X operand ...
    const float *bits_of = nullptr;          // ... which is this matrix, N = bits_n columns (null: none)
    int bits_n = 0;
    bool dry = false;      // the collecting pass: nothing is launched, nn() records the aligned copies it will need
    CopyBatch copies; int ncopy = 0;
    ConstBatch consts; int nconst = 0, const_maxcols = 0;
    AxpyBatch axpys; int naxpy = 0;
    void check() { if (!err) err = (int)hipGetLastError(); }
    void flush_copies()
    {
        // more jobs than a batch holds would leave the heads' zero-padded weight copies unmade (head_copy only records): fail loudly
        if (ncopy > MAX_COPY_JOBS) { if (!err) err = (int)hipErrorOutOfMemory; return; }
        if (ncopy > 0) {
            sahs::copy2d_batch(st, copies, ncopy, 0); check();
            sahs::copy2d_batch(st, copies, ncopy, 1); check();
        }
    }
    void flush_deferred()
    {
        if (nconst > 0) { sahs::const_cols_batch(st, consts, nconst); check(); }      // (cols <= 256: D_DRV 76, D_POSE 36)
        if (naxpy > 0) { sahs::axpy_batch(st, axpys, naxpy); check(); }
        nconst = naxpy = 0;
    }
    static bool x3() { return SAHS_SYM(sahs_bwd_gemm_precision_state)(-1) != 0; }
    // dX[P x N] (mode) = dY[P x K] * W[K x N] (* mask).  The bookkeeping of sahs::gemm_nn: its LDS-DMA kernels want W as a 16-byte aligned
    // copy (f32 products) or pre-split (x3), made in the scratch `wal` by the batched copy launch in front of the walk.
    void nn(const float *dY, long ldy, int K, const float *W, long ldw, int N, float *dX, long ldx, int mode, const float *mask = nullptr,
            long ldm = 0, float slope = 0.0f)
    {
        const int nbn = (N + GT - 1) / GT;
        unsigned char *mb = nullptr;
        if (K % GK == 0 && sahs::gemm_aligned(dY, ldy)) {
            if (x3()) {      // the B operand pre-split into bf16 hi / lo in MFMA fragment order (CopyJob pack), one batched launch per walk
                const long words = (long)K * nbn * GT;
                if (walo + words > wal_cap) { if (!err) err = (int)hipErrorOutOfMemory; return; }
                float *dst = wal + walo;
                walo += words;
                if (dry) {
                    if (ncopy < MAX_COPY_JOBS) copies.j[ncopy] = CopyJob{W, dst, ldw, 0, K, N, 1};
                    ++ncopy;       // (more than MAX_COPY_JOBS: flush_copies fails the walk before the real pass)
                    return;
                }
                W = dst; ldw = 0;
            } else if (!sahs::gemm_aligned(W, ldw)) {
                const long ldb = (N + 3) / 4 * 4;
                if (walo + (long)K * ldb > wal_cap) { if (!err) err = (int)hipErrorOutOfMemory; return; }   // scratch sized for one level's weights
                float *dst = wal + walo;
                walo += (long)K * ldb;
                if (dry) {
                    if (ncopy < MAX_COPY_JOBS) copies.j[ncopy] = CopyJob{W, dst, ldw, ldb, K, N, 0};
                    ++ncopy;
                    return;
                }
                W = dst; ldw = ldb;
            }
            // the layer's weight-gradient GEMM has just staged this very mask matrix and left its sign bits (tn)
            mb = (mask != nullptr && mask == bits_of && N == bits_n && N % 8 == 0) ? sign_bits : nullptr;
        }
        if (dry) return;
        sahs::gemm_nn(st, x3(), P, dY, ldy, K, W, ldw, N, dX, ldx, mode, mask, ldm, slope, zero, mb);
        check();
    }
    // dW[M x N] += dY[P x M]^T * X[P x N];  db != null: db[M] += column sums of dY (fused: the dY tiles are staged anyway).
    void tn(const float *dY, long ldy, int M, const float *X, long ldx, int N, float *dW, long ldw, float *db = nullptr)
    {
        if (dry) return;
        bool wrote_bits = false;
        const int e = sahs::gemm_tn(st, x3(), P, dY, ldy, M, X, ldx, N, dW, ldw, db, zero, sign_bits, &wrote_bits);
        if (!err) err = e;
        bits_of = wrote_bits ? X : nullptr;
        bits_n = N;
    }
    void copy(const float *src, long lds_, int N, float *dst, long ldd, int mode)
    {
        if (dry) return;
        sahs::copy2d(st, 2048, P, N, src, lds_, dst, ldd, mode);
        check();
    }
    // ---- the fused walk: a part's job table from the backward's layer table (bwd_program.hpp: kFwd) ----
    const float *flat = nullptr, *frame = nullptr, *actbuf = nullptr;
    float *grad_flat = nullptr, *grad_cond = nullptr;
    float *db = nullptr;   // bias-gradient scratch (DB_SCRATCH floats, zeroed)
    int dbo = 0;           // running offset into it
    float *scratch_db(int n) { float *p = db + dbo; dbo += (n + 3) / 4 * 4; return p; }
    void defer_add(const float *src, float *dst, int n)
    {
        if (naxpy < MAX_AXPY_JOBS) axpys.j[naxpy++] = AxpyJob{src, dst, n};
        else if (!err) err = (int)hipErrorOutOfMemory;
    }
    void defer_consts(long woff, long ld, int rows, int col0, int cols, const float *dbl, const float *c, float *dc)
    {
        if (nconst < MAX_CONST_JOBS) {
            consts.j[nconst++] = ConstJob{flat + woff, grad_flat + woff, dbl, c, dc, ld, rows, cols, col0};
            const_maxcols = cols > const_maxcols ? cols : const_maxcols;
        } else if (!err) err = (int)hipErrorOutOfMemory;
    }
    // The jobs of layer E: dW[:, an input segment's columns] += dZ^T X per input segment, X the segment's saved plane, the bias gradient
    // riding on the first; then per range of per-frame-constant columns their gradients from the bias gradient -- which such a layer
    // leaves in scratch (this call's db on its own), added to dbias at the end of the walk.
    void layer_jobs(TnList &L, const bwp::Dense &E, int level, const float *dZ, long ldz, int M, float *dW, float *dbias)
    {
        float *dl = E.nfold ? scratch_db(E.rows) : dbias;
        for (int s = 0; s < E.nin; ++s)
            L.add(dZ, ldz, M, actbuf + (long)E.in[s].plane * P, E.in[s].width, E.in[s].valid, dW + E.in[s].col0, E.ld, s == 0 ? dl : nullptr);
        if (E.nfold) defer_add(dl, dbias, E.rows);
        for (int f = 0; f < E.nfold; ++f) {
            const bool pose = E.fold[f].which == 1;      // (Fold::which; grad_cond is laid out like the frame's head: [0:76] d_driving, [80:116] d_pose36)
            defer_consts(E.w_off[level], E.ld, E.rows, E.fold[f].src_col, E.fold[f].count, dl, frame + (pose ? FRAME_POSE_OFF : FRAME_DRV_OFF),
                         grad_cond + (pose ? FRAME_POSE_OFF : FRAME_DRV_OFF));
        }
    }
};

}  // namespace

// Words of workspace per call: gA, gB, dfeat (P x 256 each), din (P x 96), dgridf (P x 32), dxw, dw, g3 (P x 4 each), db scratch,
// channel-last copies of the feature grid and of its gradient accumulator
constexpr int DB_SCRATCH = 8192;   // per-call bias-gradient scratch (all layers of one level: ~5.3 K floats)
constexpr long WAL_FLOATS = 2L << 20;   // aligned weight sub-matrix copies of one level (< 1.8 M floats)
// the three output heads as 16-row matrices over the whole d_raw row [drgb3 | dseg12 | dsigma]: zero-padded weights W16 and their gradients
constexpr int HEAD_W_SEG = 0, HEAD_W_RGB = 16 * 128, HEAD_W_ALPHA = 2 * 16 * 128, HEAD_G_SEG = HEAD_W_ALPHA + 16 * 256, HEAD_G_RGB = HEAD_G_SEG + 16 * 128,
              HEAD_G_ALPHA = HEAD_G_RGB + 16 * 128, HEAD_DB = HEAD_G_ALPHA + 16 * 256;
constexpr long HEAD_FLOATS = HEAD_DB + 64;
extern "C" long SAHS_SYM(sahs_field_backward_ws_words)(long P) { return P * (256L * 3 + DIN_LD + 32 + 12) + DB_SCRATCH + 2 * GRID_FLOATS + WAL_FLOATS + P * 8 + HEAD_FLOATS; }

// The per-layer walk.  It states the network by hand -- every tensor, leading dimension, column offset and plane below -- and is NOT moved onto
// the layer table the fused walk is generated from (bwd_program.hpp): it is the reference the tests compare the fused walk against, and a
// shared table would turn a mistake in the table into a common-mode error that those tests cannot see.
// grad_cond: [0:76] d_driving, [80:116] d_pose36 (accumulated).  grad_flat: accumulated.  d_raw: (P,16).
// part (bit 1: deformation nets, bit 2: radiance nets; 0 = 3 = everything) cuts the walk at its seam, the gradient w.r.t. the deformed
// point and the ambient coordinate, (P,8) rows [dx'0 dx'1 dx'2 . dw0 dw1 . .]: the radiance part alone leaves it in xwg_out, the
// deformation part alone starts from xwg_in, and the whole walk adds xwg_in (if given) at the seam -- that is how the fine pass's
// gradient reaches the coarse samples' deformation when the forward evaluated the deformation nets once per depth (field_f32.hip MODE).
extern "C" int SAHS_SYM(sahs_field_backward_launch)(const float *flat, const float *frame, int level, long P, const float *actbuf, const float *d_raw,
                                          float *grad_flat, float *grad_cond, float *ws, hipStream_t stream)
{
    return SAHS_SYM(sahs_field_backward_split_launch)(flat, frame, level, 3, P, actbuf, d_raw, nullptr, nullptr, grad_flat, grad_cond, ws, stream);
}
extern "C" int SAHS_SYM(sahs_field_backward_split_launch)(const float *flat, const float *frame, int level, int part, long P, const float *actbuf,
                                                const float *d_raw, const float *xwg_in, float *xwg_out, float *grad_flat, float *grad_cond,
                                                float *ws, hipStream_t stream)
{
    if (P <= 0) return 0;
    if (part == 0) part = 3;
    const bool do_rad = (part & 2) != 0, do_def = (part & 1) != 0;
#if SAHS_MODEL == 2
    if (part != 3) return -3;      // no deformation nets: nothing to split
#endif
    if (P > 4000000L) return -3;   // gridDim.y of the P x N GEMMs; callers chunk larger batches
    Bwd b{stream, P};
    b.flat = flat; b.grad_flat = grad_flat;      // (what defer_consts addresses the weights and their gradient by)
    b.zero = ws + P * (256L * 3 + DIN_LD + 32 + 12) + DB_SCRATCH - 64;   // tail of the (zeroed) bias-gradient scratch, never written
    b.wal = ws + P * (256L * 3 + DIN_LD + 32 + 12) + DB_SCRATCH + 2 * GRID_FLOATS;
    b.wal_cap = WAL_FLOATS;
    float *heads = b.wal + WAL_FLOATS + P * 8;
    if (hipMemsetAsync(heads, 0, sizeof(float) * HEAD_FLOATS, stream) != hipSuccess) return (int)hipGetLastError();
    b.sign_bits = sahs_diag_env("SAHS_BWD_NOBITS") ? nullptr : reinterpret_cast<unsigned char *>(b.wal + WAL_FLOATS);     // P x 32 bytes (<= 256 columns)
    const FlatOffsets &F = kFlat;
    const FlatOffsets::Lvl &Lv = F.lvl[level];
    float *gA = ws, *gB = gA + P * 256, *dfeat = gB + P * 256, *din = dfeat + P * 256, *dgridf = din + P * DIN_LD, *dxw = dgridf + P * 32,
          *dw = dxw + P * 4, *g3 = dw + P * 4, *db = g3 + P * 4, *grid_cl = db + DB_SCRATCH, *dgrid_cl = grid_cl + GRID_FLOATS;
    // saved activations: one dense [P x width] array per layer, the array at column c of the act:: table starting at c * P
    if (hipMemsetAsync(db, 0, sizeof(float) * DB_SCRATCH, stream) != hipSuccess) return (int)hipGetLastError();
    if (hipMemsetAsync(dgrid_cl, 0, sizeof(float) * GRID_FLOATS, stream) != hipSuccess) return (int)hipGetLastError();
    const float *drv = frame + FRAME_DRV_OFF, *p36 = frame + FRAME_POSE_OFF;
    float *d_drv = grad_cond + 0, *d_p36 = grad_cond + 80;
    const float *trc = TRUNK_SEES_POSE ? p36 : drv;          // the per-frame constant the trunk sees, and its gradient slot
    float *d_trc = TRUNK_SEES_POSE ? d_p36 : d_drv;
    auto W = [&](long off) { return flat + off; };
    auto G = [&](long off) { return grad_flat + off; };
    int dbo = 0;   // running offset into db scratch
    // The walk runs twice: once dry -- nothing is launched, the data-gradient GEMMs record which weight sub-matrices they need as
    // 16-byte aligned copies -- then all of those copies in one launch, then for real.  Both passes take the same branches, so the
    // scratch offsets (walo, dbo) they hand out are the same.
    auto walk = [&]() -> int {
    dbo = 0;
    b.walo = 0;
    // bias-gradient slots of one level: BIAS_FLOATS-ish; the last 64 floats of the scratch are the DMA zero page
    static_assert(BIAS_FLOATS + 16 * 40 <= DB_SCRATCH - 64, "bias-gradient scratch too small for this model");
    // bias gradient of a layer: straight into the flat gradient (boff >= 0), or -- for the six layers whose folded per-frame
    // constants need this call's db on its own -- into a scratch slot that add_bias then adds
    auto newdb = [&](int n, long boff = -1) { if (boff >= 0) return G(boff); float *p = db + dbo; dbo += (n + 3) / 4 * 4; return p; };
    // (the deferred tables are the fused walk's, Bwd::defer_add / defer_consts: a full table fails the walk)
    auto add_bias = [&](float *dbl, long boff, int n) {      // deferred to the end of the walk, batched (nothing in the walk reads G(boff))
        if (dbl == G(boff) || b.dry) return;
        b.defer_add(dbl, G(boff), n);
    };
    auto consts = [&](long woff, long ld, int rows, int col0, int cols, const float *dbl, const float *c, float *dc) {
        if (b.dry) return;
        b.defer_consts(woff, ld, rows, col0, cols, dbl, c, dc);      // deferred as well: dW's constant columns and dc are read by nothing in the walk
    };
    // rows of a head's weights into its zero-padded 16-row copy (collected in the dry pass, one batched launch with the aligned weight
    // copies); rows of a head's gradient scratch added to the flat gradient (deferred to the end of the walk, batched)
    auto head_copy = [&](const float *src, float *dst, int rows, int cols) {
        if (!b.dry) return;
        if (b.ncopy < MAX_COPY_JOBS) b.copies.j[b.ncopy] = CopyJob{src, dst, cols, cols, rows, cols, 0};
        else b.err = (int)hipErrorOutOfMemory;
        ++b.ncopy;
    };
    auto head_add = [&](const float *src, float *dst, int n) {
        if (b.dry) return;
        b.defer_add(src, dst, n);
    };
    const float *A = actbuf;
    if (do_rad) {
    // ================= seg branch: seg = fc_seg(s3), s_i = lrelu(layers_seg[i](.)) (modules.py:289-294) =================
    {
        // the output heads read the whole 16-float d_raw row ([drgb3 | dseg12 | dsigma], 16-byte aligned, K = 16 = one LDS-DMA K-step)
        // against 16-row zero-padded copies of their weights, instead of its unaligned 3/12/1-column slices through the register-staged
        // GEMM: dW16 = d_raw^T X lands in scratch, rows 3..14 of it are fc_seg's gradient; its column sums are the three bias gradients
        static_assert(BR_H == 128 && TR_H == 256 && N_SEG == 12, "head scratch layout");
        head_copy(W(Lv.segout_w), heads + HEAD_W_SEG + 3 * BR_H, N_SEG, BR_H);
        head_copy(W(Lv.rgb_w), heads + HEAD_W_RGB, 3, BR_H);
        head_copy(W(Lv.alpha_w), heads + HEAD_W_ALPHA + 15 * TR_H, 1, TR_H);
        b.tn(d_raw, 16, 16, A + (long)(act::S + 384) * P, BR_H, BR_H, heads + HEAD_G_SEG, BR_H, heads + HEAD_DB);
        head_add(heads + HEAD_G_SEG + 3 * BR_H, G(Lv.segout_w), N_SEG * BR_H);
        head_add(heads + HEAD_DB + 3, G(Lv.segout_b), N_SEG);
        head_add(heads + HEAD_DB, G(Lv.rgb_b), 3);
        head_add(heads + HEAD_DB + 15, G(Lv.alpha_b), 1);
        b.nn(d_raw, 16, 16, heads + HEAD_W_SEG, BR_H, BR_H, gA, BR_H, 0, A + (long)(act::S + 384) * P, BR_H, 0.01f);
        float *cur = gA, *nxt = gB;
        for (int i = 3; i >= 1; --i) {   // layers_seg[i]: s_{i-1} (128) -> s_i
            float *d = newdb(BR_H, Lv.seg_b[i]);
            b.tn(cur, BR_H, BR_H, A + (long)(act::S + 128 * (i - 1)) * P, BR_H, BR_H, G(Lv.seg_w[i]), BR_H, d);
            add_bias(d, Lv.seg_b[i], BR_H);
            b.nn(cur, BR_H, BR_H, W(Lv.seg_w[i]), BR_H, BR_H, nxt, BR_H, 0, A + (long)(act::S + 128 * (i - 1)) * P, BR_H, 0.01f);
            float *t = cur; cur = nxt; nxt = t;
        }
        float *d = newdb(BR_H, Lv.seg_b[0]);   // layers_seg[0]: feat (256) -> s0
        b.tn(cur, BR_H, BR_H, A + (long)(act::FEAT) * P, TR_H, TR_H, G(Lv.seg_w[0]), TR_H, d);
        add_bias(d, Lv.seg_b[0], BR_H);
        b.nn(cur, BR_H, BR_H, W(Lv.seg_w[0]), TR_H, TR_H, dfeat, 256, 0);       // feat has no activation
    }
    // ================= colour branch (modules.py:276-287) =================
    {
        b.tn(d_raw, 16, 16, A + (long)(act::C + 384) * P, BR_H, BR_H, heads + HEAD_G_RGB, BR_H);
        head_add(heads + HEAD_G_RGB, G(Lv.rgb_w), 3 * BR_H);
        b.nn(d_raw, 16, 16, heads + HEAD_W_RGB, BR_H, BR_H, gA, BR_H, 0, A + (long)(act::C + 384) * P, BR_H, 0.01f);
        float *cur = gA, *nxt = gB;
        for (int i = 3; i >= 1; --i) {
            float *d = newdb(BR_H, Lv.dir_b[i]);
            b.tn(cur, BR_H, BR_H, A + (long)(act::C + 128 * (i - 1)) * P, BR_H, BR_H, G(Lv.dir_w[i]), BR_H, d);
            add_bias(d, Lv.dir_b[i], BR_H);
            b.nn(cur, BR_H, BR_H, W(Lv.dir_w[i]), BR_H, BR_H, nxt, BR_H, 0, A + (long)(act::C + 128 * (i - 1)) * P, BR_H, 0.01f);
            float *t = cur; cur = nxt; nxt = t;
        }
        // layers_dir[0]: [feat256 | dirPE27 | grid32] -> c0
        float *d = newdb(BR_H, Lv.dir_b[0]);
        b.tn(cur, BR_H, BR_H, A + (long)(act::FEAT) * P, TR_H, TR_H, G(Lv.dir_w[0]), D_DIR_IN, d);
        b.tn(cur, BR_H, BR_H, A + (long)(act::DIR) * P, 32, D_DIR, G(Lv.dir_w[0]) + TR_H, D_DIR_IN);
        b.tn(cur, BR_H, BR_H, A + (long)(act::GRID) * P, 32, D_GRID, G(Lv.dir_w[0]) + TR_H + D_DIR, D_DIR_IN);
        add_bias(d, Lv.dir_b[0], BR_H);
        b.nn(cur, BR_H, BR_H, W(Lv.dir_w[0]), D_DIR_IN, TR_H, dfeat, 256, 1);
        b.nn(cur, BR_H, BR_H, W(Lv.dir_w[0]) + TR_H + D_DIR, D_DIR_IN, D_GRID, dgridf, 32, 0);
    }
    // ================= sigma = fc_alpha(feat) (modules.py:275) =================
    {
        b.tn(d_raw, 16, 16, A + (long)(act::FEAT) * P, TR_H, TR_H, heads + HEAD_G_ALPHA, TR_H);
        head_add(heads + HEAD_G_ALPHA + 15 * TR_H, G(Lv.alpha_w), TR_H);
        b.nn(d_raw, 16, 16, heads + HEAD_W_ALPHA, TR_H, TR_H, dfeat, 256, 1);          // d feat += d sigma (x) w_alpha
    }
    // ================= trunk (modules.py:267-274) =================
    {
        // feat = fc_feat(t7)
        float *d = newdb(TR_H, Lv.feat_b);
        b.tn(dfeat, 256, TR_H, A + (long)(act::T + (TR_LAYERS - 1) * 256) * P, TR_H, TR_H, G(Lv.feat_w), TR_H, d);
        add_bias(d, Lv.feat_b, TR_H);
        b.nn(dfeat, 256, TR_H, W(Lv.feat_w), TR_H, TR_H, gA, 256, 0, A + (long)(act::T + (TR_LAYERS - 1) * 256) * P, TR_H, 0.01f);
        float *cur = gA, *nxt = gB;
        for (int i = TR_LAYERS - 1; i >= 1; --i) {   // layers_xyz[i]: input t_{i-1} (and, for i == 3, [PE(x') | PE(w) | pose36])
            float *dl = (i == 3) ? newdb(TR_H) : newdb(TR_H, Lv.xyz_b[i]);
            const long ldw = (i == 3) ? TR_H + D_TR_IN : TR_H;
            b.tn(cur, 256, TR_H, A + (long)(act::T + (i - 1) * 256) * P, TR_H, TR_H, G(Lv.xyz_w[i]), ldw, dl);
            add_bias(dl, Lv.xyz_b[i], TR_H);
            if (i == 3) {
                b.tn(cur, 256, TR_H, A + (long)(act::PEX) * P, 16 * KB_XYZ, D_XYZ, G(Lv.xyz_w[3]) + TR_H, ldw);
                if (D_AMB > 0) b.tn(cur, 256, TR_H, A + (long)(act::PEW) * P, 16 * KB_AMB, D_AMB, G(Lv.xyz_w[3]) + TR_H + D_XYZ, ldw);
                consts(Lv.xyz_w[3], ldw, TR_H, TR_H + D_XYZ + D_AMB, D_TR_CONST, dl, trc, d_trc);
                b.nn(cur, 256, TR_H, W(Lv.xyz_w[3]) + TR_H, ldw, D_XYZ, din, DIN_LD, 0);        // first writer of din stores,
                if (D_AMB > 0) b.nn(cur, 256, TR_H, W(Lv.xyz_w[3]) + TR_H + D_XYZ, ldw, D_AMB, din + DIN_AMB, DIN_LD, 0);   // layers_xyz[0] below accumulates
            }
            b.nn(cur, 256, TR_H, W(Lv.xyz_w[i]), ldw, TR_H, nxt, 256, 0, A + (long)(act::T + (i - 1) * 256) * P, TR_H, 0.01f);
            float *t = cur; cur = nxt; nxt = t;
        }
        // layers_xyz[0]: [PE63(x') | PE18(w) | pose36] -> t0
        float *dl = newdb(TR_H);
        b.tn(cur, 256, TR_H, A + (long)(act::PEX) * P, 16 * KB_XYZ, D_XYZ, G(Lv.xyz_w[0]), D_TR_IN, dl);
        if (D_AMB > 0) b.tn(cur, 256, TR_H, A + (long)(act::PEW) * P, 16 * KB_AMB, D_AMB, G(Lv.xyz_w[0]) + D_XYZ, D_TR_IN);
        add_bias(dl, Lv.xyz_b[0], TR_H);
        consts(Lv.xyz_w[0], D_TR_IN, TR_H, D_XYZ + D_AMB, D_TR_CONST, dl, trc, d_trc);
        b.nn(cur, 256, TR_H, W(Lv.xyz_w[0]), D_TR_IN, D_XYZ, din, DIN_LD, 1);
        if (D_AMB > 0) b.nn(cur, 256, TR_H, W(Lv.xyz_w[0]) + D_XYZ, D_TR_IN, D_AMB, din + DIN_AMB, DIN_LD, 1);
    }
    // ================= encodings + feature grid -> d x', d w =================
    {
        const int tb = (int)(GRID_FLOATS / 32 / 32);   // 32 voxels x 32 channels per block
        if (!b.dry) {
        grid_transpose_kernel<<<tb, 256, 0, stream>>>(W(F.grid), grid_cl, 0); b.check();
        const long gb = (P + 127) / 128;                // 4 waves x 2 runs of 16 samples per block pass
        grid_backward_kernel<<<(unsigned)(gb < 8192 ? gb : 8192), 256, 0, stream>>>(P, actbuf, dgridf, grid_cl, dgrid_cl, dxw); b.check();
        grid_transpose_kernel<<<tb, 256, 0, stream>>>(dgrid_cl, G(F.grid), 1); b.check();
        encode_backward_kernel<<<2048, 256, 0, stream>>>(P, actbuf, din, nullptr, dxw, dw, nullptr); b.check();
        }
    }
    }   // do_rad
    // ---- the seam: d x' (P,4) and d w (P,4) ----
    if (do_rad && !do_def && xwg_out != nullptr) { b.copy(dxw, 4, 4, xwg_out, 8, 0); b.copy(dw, 4, 4, xwg_out + 4, 8, 0); }
    if (xwg_in != nullptr && do_def) { b.copy(xwg_in, 8, 4, dxw, 4, do_rad ? 1 : 0); b.copy(xwg_in + 4, 8, 4, dw, 4, do_rad ? 1 : 0); }
    if (!do_def) { if (!b.dry) b.flush_deferred(); if (!b.err && dbo > DB_SCRATCH - 64) b.err = (int)hipErrorOutOfMemory; return b.err; }
#if SAHS_MODEL != 2
    // ================= hyper sheet (modules.py:444-462): w = fc_ambient(g5) =================
    {
        float *dbl = newdb(4, F.hyp_fb);
        b.tn(dw, 4, AMB_DIM, A + (long)(act::HH + 5 * 64) * P, HYP_H, HYP_H, G(F.hyp_fw), HYP_H, dbl);
        add_bias(dbl, F.hyp_fb, AMB_DIM);
        b.nn(dw, 4, AMB_DIM, W(F.hyp_fw), HYP_H, HYP_H, gA, HYP_H, 0, A + (long)(act::HH + 5 * 64) * P, HYP_H, 0.0f);
        float *cur = gA, *nxt = gB;
        for (int i = 5; i >= 1; --i) {
            float *dl = (i == 4) ? newdb(HYP_H) : newdb(HYP_H, F.hyp_b[i]);
            const long ldw = (i == 4) ? HYP_H + D_DEF_IN : HYP_H;
            b.tn(cur, HYP_H, HYP_H, A + (long)(act::HH + (i - 1) * 64) * P, HYP_H, HYP_H, G(F.hyp_w[i]), ldw, dl);
            add_bias(dl, F.hyp_b[i], HYP_H);
            if (i == 4) {
                b.tn(cur, HYP_H, HYP_H, A + (long)(act::E) * P, 16 * KB_XYZ, D_XYZ, G(F.hyp_w[4]) + HYP_H, ldw);
                consts(F.hyp_w[4], ldw, HYP_H, HYP_H + D_XYZ, D_DRV, dl, drv, d_drv);
                consts(F.hyp_w[4], ldw, HYP_H, HYP_H + D_XYZ + D_DRV, D_POSE, dl, p36, d_p36);
            }
            b.nn(cur, HYP_H, HYP_H, W(F.hyp_w[i]), ldw, HYP_H, nxt, HYP_H, 0, A + (long)(act::HH + (i - 1) * 64) * P, HYP_H, 0.0f);
            float *t = cur; cur = nxt; nxt = t;
        }
        float *dl = newdb(HYP_H);
        b.tn(cur, HYP_H, HYP_H, A + (long)(act::E) * P, 16 * KB_XYZ, D_XYZ, G(F.hyp_w[0]), D_DEF_IN, dl);
        add_bias(dl, F.hyp_b[0], HYP_H);
        consts(F.hyp_w[0], D_DEF_IN, HYP_H, D_XYZ, D_DRV, dl, drv, d_drv);
        consts(F.hyp_w[0], D_DEF_IN, HYP_H, D_XYZ + D_DRV, D_POSE, dl, p36, d_p36);
    }
    // ================= warp field (modules.py:371-390): x' = x + tanh(fc_final(h5)) =================
    {
        if (!b.dry) { tanh_backward_kernel<<<2048, 256, 0, stream>>>(P, actbuf, dxw, g3); b.check(); }
        float *dbl = newdb(4, F.warp_fb);
        b.tn(g3, 4, 3, A + (long)(act::WH + 5 * 128) * P, WARP_H, WARP_H, G(F.warp_fw), WARP_H, dbl);
        add_bias(dbl, F.warp_fb, 3);
        b.nn(g3, 4, 3, W(F.warp_fw), WARP_H, WARP_H, gA, WARP_H, 0, A + (long)(act::WH + 5 * 128) * P, WARP_H, 0.0f);
        float *cur = gA, *nxt = gB;
        for (int i = 5; i >= 1; --i) {
            float *dl = (i == 4) ? newdb(WARP_H) : newdb(WARP_H, F.warp_b[i]);
            const long ldw = (i == 4) ? WARP_H + D_DEF_IN : WARP_H;
            b.tn(cur, WARP_H, WARP_H, A + (long)(act::WH + (i - 1) * 128) * P, WARP_H, WARP_H, G(F.warp_w[i]), ldw, dl);
            add_bias(dl, F.warp_b[i], WARP_H);
            if (i == 4) {
                b.tn(cur, WARP_H, WARP_H, A + (long)(act::E) * P, 16 * KB_XYZ, D_XYZ, G(F.warp_w[4]) + WARP_H, ldw);
                consts(F.warp_w[4], ldw, WARP_H, WARP_H + D_XYZ, D_DRV, dl, drv, d_drv);
                consts(F.warp_w[4], ldw, WARP_H, WARP_H + D_XYZ + D_DRV, D_POSE, dl, p36, d_p36);
            }
            b.nn(cur, WARP_H, WARP_H, W(F.warp_w[i]), ldw, WARP_H, nxt, WARP_H, 0, A + (long)(act::WH + (i - 1) * 128) * P, WARP_H, 0.0f);
            float *t = cur; cur = nxt; nxt = t;
        }
        float *dl = newdb(WARP_H);
        b.tn(cur, WARP_H, WARP_H, A + (long)(act::E) * P, 16 * KB_XYZ, D_XYZ, G(F.warp_w[0]), D_DEF_IN, dl);
        add_bias(dl, F.warp_b[0], WARP_H);
        consts(F.warp_w[0], D_DEF_IN, WARP_H, D_XYZ, D_DRV, dl, drv, d_drv);
        consts(F.warp_w[0], D_DEF_IN, WARP_H, D_XYZ + D_DRV, D_POSE, dl, p36, d_p36);
    }
#else
    (void)drv; (void)d_p36; (void)p36; (void)g3;   // no deformation nets: the gradient stops at the (input) point
#endif
    if (!b.dry) b.flush_deferred();
    if (!b.err && dbo > DB_SCRATCH - 64) b.err = (int)hipErrorOutOfMemory;
    return b.err;
    };      // walk
    b.dry = true;
    if (int e = walk()) return e;
    b.flush_copies();
    if (b.err) return b.err;
    b.dry = false;
    return walk();
}

// ================================================================================================================================
// The fused walk (round 4: AudioFaceModel; NeRFaceModels since): per part of the field TWO GEMM-class launches instead of ~38 --
//   1. field_backward_chain_{rad,def}_kernel (field_bwd_chain.hip): the whole data-gradient chain, sample-major, every layer's dZ stored once
//      into its plane of `dact` (the act:: layout), masks from the sign bits the saving forward wrote;
//   2. gemm_tn_jobs_kernel: every layer's dW (+ db) = dZ^T X from those planes and the saved activations, one job table;
// around them the small kernels of the per-layer walk (feature-grid scatter, encodings, per-frame-constant columns, deferred adds).
// part 1: deformation nets (seam gradient xwg_in (P,8) -> parameters); part 2: radiance nets of `level` (d_raw (P,16) -> parameters, seam
// gradient to xwg_out); part 3: part 2, then part 1 on (its seam gradient + xwg_in).  actbuf / bits: the buffers the saving forward of that
// part wrote (a plane of column c at actbuf + c * P; for part 3 bits = [deformation planes | radiance planes]).
// The NeRFaceModel without deformation nets (SAHS_MODEL 2) has part 3 only, which is its radiance part: no deformation chain, and no seam
// gradient (nothing upstream of the raw sample point has parameters: its chain stops at dT0, the encodings' backward is not run).
// ================================================================================================================================

namespace {
constexpr long RAD_PLANES = act::STRIDE - act::XW, DEF_PLANES = act::XW;        // floats per sample of the dZ planes of a part
struct FusedWs {      // workspace of one part, in floats
    // the part's transposed weight stream: split bf16 (hi + lo halfwords) or fp32, whichever the walk's arithmetic is
    static long stream(int part) { const long a = SAHS_SYM(sahs_bwd_chain_stream_hw)(part) / 2, b = SAHS_SYM(sahs_bwd_chain_f32_stream_floats)(part); return a > b ? a : b; }
    static long rad(long P) { return P * (RAD_PLANES + 32 + 2 * DIN_LD + 8) + DB_SCRATCH + 2 * GRID_FLOATS + stream(2) + HEAD_FLOATS; }
    static long def(long P) { return P * (DEF_PLANES + 8) + DB_SCRATCH + stream(1); }
};

}  // namespace

// floats of workspace of a fused walk of `part` over P samples; -1: a part the model does not have
extern "C" long SAHS_SYM(sahs_field_backward_fused_ws_words)(int part, long P)
{
    if (!USE_DEFORM) return part == 3 ? FusedWs::rad(P) : -1;
    return part == 1 ? FusedWs::def(P) : (part == 2 ? FusedWs::rad(P) : FusedWs::rad(P) + FusedWs::def(P) + P * 8);
}

static int fused_rad(const float *flat, const float *frame, int level, long P, const float *actbuf, const uint32_t *bits, const float *d_raw,
                     float *xwg_out, float *grad_flat, float *grad_cond, float *ws, int num_cu, hipStream_t stream)
{
    Bwd b{stream, P};
    const FlatOffsets &F = kFlat;
    float *dact_mem = ws, *dgridf = dact_mem + P * RAD_PLANES, *din_a = dgridf + P * 32, *din_b = din_a + P * DIN_LD, *dxw = din_b + P * DIN_LD,
          *dw = dxw + P * 4, *db = dw + P * 4, *grid_cl = db + DB_SCRATCH, *dgrid_cl = grid_cl + GRID_FLOATS, *bstream = dgrid_cl + GRID_FLOATS,
          *heads = bstream + FusedWs::stream(2);
    float *dact = dact_mem - (long)act::XW * P;              // plane of act:: column c at dact + c * P (columns >= XW are backed)
    b.zero = db + DB_SCRATCH - 64;
    if (hipMemsetAsync(db, 0, sizeof(float) * DB_SCRATCH, stream) != hipSuccess) return (int)hipGetLastError();
    if (hipMemsetAsync(dgrid_cl, 0, sizeof(float) * GRID_FLOATS, stream) != hipSuccess) return (int)hipGetLastError();
    if (hipMemsetAsync(heads, 0, sizeof(float) * HEAD_FLOATS, stream) != hipSuccess) return (int)hipGetLastError();
    const bool f32 = !Bwd::x3();      // exact fp32 products (ops.backward_gemm_precision("fp32")): the fp32 chain and job kernels
    int e = f32 ? SAHS_SYM(sahs_bwd_chain_f32_pack_launch)(flat, bstream, level, 2, stream) : SAHS_SYM(sahs_bwd_chain_pack_launch)(flat, bstream, level, 2, stream);
    if (e) return e;
    e = f32 ? SAHS_SYM(sahs_bwd_chain_f32_rad_launch)(bstream, P, d_raw, bits, dact, dgridf, din_a, din_b, num_cu, stream)
            : SAHS_SYM(sahs_bwd_chain_rad_launch)(bstream, P, d_raw, bits, dact, dgridf, din_a, din_b, num_cu, stream);
    if (e) return e;
    // ---- encodings + feature grid -> the seam gradient (what the deformation part waits for) ----
    {
        const int tb = (int)(GRID_FLOATS / 32 / 32);
        grid_transpose_kernel<<<tb, 256, 0, stream>>>(flat + F.grid, grid_cl, 0); b.check();
        const long gb = (P + 127) / 128;
        grid_backward_kernel<<<(unsigned)(gb < 8192 ? gb : 8192), 256, 0, stream>>>(P, actbuf, dgridf, grid_cl, dgrid_cl, dxw); b.check();
        grid_transpose_kernel<<<tb, 256, 0, stream>>>(dgrid_cl, grad_flat + F.grid, 1); b.check();
        if (USE_DEFORM) { encode_backward_kernel<<<2048, 256, 0, stream>>>(P, actbuf, din_a, din_b, dxw, dw, xwg_out); b.check(); }
    }
    // ---- every weight gradient of the part: one job table, in this order (TnList cuts items by cost in list order, tiles of one job share an XCD) ----
    b.flat = flat; b.frame = frame; b.actbuf = actbuf; b.grad_flat = grad_flat; b.grad_cond = grad_cond; b.db = db;
    auto G = [&](long off) { return grad_flat + off; };
    int order[hb::NUM_LAYERS_H], n = 0;
    for (int id : {hb::H_SEG, hb::H_RGB, hb::H_ALPHA, hb::H_S3, hb::H_D3, hb::H_S2, hb::H_D2, hb::H_S1, hb::H_D1, hb::H_S0, hb::H_D0, hb::H_FEAT}) order[n++] = id;
    for (int i = TR_LAYERS - 1; i >= 0; --i) order[n++] = hb::H_T0 + i;
    TnList L;
    float *head_db = heads + HEAD_DB;      // the column sums of d_raw = the three heads' bias gradients: with the first head's job
    for (int k = 0; k < n; ++k) {
        const bwp::Dense &E = bwp::kFwd.d[order[k]];
        if (E.out != bwp::HEAD) {
            b.layer_jobs(L, E, level, dact + (long)E.out * P, E.rows, E.rows, G(E.w_off[level]), G(E.b_off[level]));
            continue;
        }
        // a head reads the whole d_raw row against a 16-row scratch gradient, of which rows kshift .. are its own (3..14 fc_seg, 0..2 fc_rgb, 15 fc_alpha)
        float *hg = heads + (order[k] == hb::H_SEG ? HEAD_G_SEG : (order[k] == hb::H_RGB ? HEAD_G_RGB : HEAD_G_ALPHA));
        b.layer_jobs(L, E, level, d_raw, D_RAW, D_RAW, hg, head_db);
        head_db = nullptr;
        b.defer_add(hg + E.kshift * E.ld, G(E.w_off[level]), E.rows * E.ld);
        b.defer_add(heads + HEAD_DB + E.kshift, G(E.b_off[level]), E.rows);
    }
    if (b.err) return b.err;
    e = L.launch(P, b.zero, num_cu, stream, f32);
    if (e) return e;
    b.flush_deferred();
    return b.err;
}

#if SAHS_MODEL != 2
static int fused_def(const float *flat, const float *frame, long P, const float *actbuf, const uint32_t *bits, const float *xwg, float *grad_flat,
                     float *grad_cond, float *ws, int num_cu, hipStream_t stream)
{
    Bwd b{stream, P};
    float *dact = ws, *g3 = dact + P * DEF_PLANES, *dw4 = g3 + P * 4, *db = dw4 + P * 4, *bstream = db + DB_SCRATCH;
    b.zero = db + DB_SCRATCH - 64;
    if (hipMemsetAsync(db, 0, sizeof(float) * DB_SCRATCH, stream) != hipSuccess) return (int)hipGetLastError();
    const bool f32 = !Bwd::x3();
    int e = f32 ? SAHS_SYM(sahs_bwd_chain_f32_pack_launch)(flat, bstream, 0, 1, stream) : SAHS_SYM(sahs_bwd_chain_pack_launch)(flat, bstream, 0, 1, stream);
    if (e) return e;
    e = f32 ? SAHS_SYM(sahs_bwd_chain_f32_def_launch)(bstream, P, xwg, actbuf, bits, dact, g3, dw4, num_cu, stream)
            : SAHS_SYM(sahs_bwd_chain_def_launch)(bstream, P, xwg, actbuf, bits, dact, g3, dw4, num_cu, stream);
    if (e) return e;
    b.flat = flat; b.frame = frame; b.actbuf = actbuf; b.grad_flat = grad_flat; b.grad_cond = grad_cond; b.db = db;
    TnList L;
    for (int id : {hb::H_HF, hb::H_H5, hb::H_H4, hb::H_H3, hb::H_H2, hb::H_H1, hb::H_H0, hb::H_WF, hb::H_W5, hb::H_W4, hb::H_W3, hb::H_W2, hb::H_W1, hb::H_W0}) {
        const bwp::Dense &E = bwp::kFwd.d[id];
        // (a head's dZ: the (P,4) rows of pre-activation gradients the chain kernel left)
        const float *dZ = E.out != bwp::HEAD ? dact + (long)E.out * P : (id == hb::H_HF ? dw4 : g3);
        b.layer_jobs(L, E, 0, dZ, E.out != bwp::HEAD ? E.rows : 4, E.rows, grad_flat + E.w_off[0], grad_flat + E.b_off[0]);
    }
    if (b.err) return b.err;
    e = L.launch(P, b.zero, num_cu, stream, f32);
    if (e) return e;
    b.flush_deferred();
    return b.err;
}

#endif      // SAHS_MODEL != 2

extern "C" int SAHS_SYM(sahs_field_backward_fused_launch)(const float *flat, const float *frame, int level, int part, long P, const float *actbuf,
                                                          const uint32_t *bits, const float *d_raw, const float *xwg_in, float *xwg_out, float *grad_flat,
                                                          float *grad_cond, float *ws, int num_cu, hipStream_t stream)
{
    if (P <= 0) return 0;
    if (P > 4000000L) return -3;      // 32-bit byte offsets inside a plane (256 floats per sample)
#if SAHS_MODEL == 2
    (void)xwg_in; (void)xwg_out;
    if (part != 3) return -2;         // no deformation nets: nothing to split
    return fused_rad(flat, frame, level, P, actbuf, bits, d_raw, nullptr, grad_flat, grad_cond, ws, num_cu, stream);
#else
    if (part == 1) return fused_def(flat, frame, P, actbuf, bits, xwg_in, grad_flat, grad_cond, ws, num_cu, stream);
    if (part == 2) return fused_rad(flat, frame, level, P, actbuf, bits, d_raw, xwg_out, grad_flat, grad_cond, ws, num_cu, stream);
    if (part != 3) return -2;
    // everything: the radiance part's seam gradient (+ xwg_in, the fine pass's share when the deformation was shared) feeds the deformation part
    float *seam = ws + FusedWs::rad(P), *ws_def = seam + P * 8;
    int e = fused_rad(flat, frame, level, P, actbuf, bits + (long)sbits::BD_WORDS * P, d_raw, seam, grad_flat, grad_cond, ws, num_cu, stream);
    if (e) return e;
    if (xwg_in != nullptr) {
        sahs::add_rows8(stream, P * 2, xwg_in, seam);
        if ((e = (int)hipGetLastError())) return e;
    }
    return fused_def(flat, frame, P, actbuf, bits, seam, grad_flat, grad_cond, ws_def, num_cu, stream);
#endif
}
