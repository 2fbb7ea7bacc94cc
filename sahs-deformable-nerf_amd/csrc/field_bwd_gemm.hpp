// field_bwd_gemm.hpp -- host launchers of the backward's model-independent kernels: the dense GEMMs of the per-layer walk and the
// copy / axpy / constant-column helpers of both walks (field_bwd_gemm.hip), the job-table weight-gradient launches of the fused walk
// (field_bwd_tn_jobs.hip).
//
// None of them reads a layout constant, so they are built ONCE, in plain namespace sahs, and every model's field_bwd.hip calls them
// as sahs::...  A kernel can only be launched from the translation unit that defines it: this header declares launchers and the job
// types that travel as kernel arguments, not kernels.  Unless stated otherwise a launcher enqueues on `st` and reports nothing; the
// caller reads hipGetLastError() as it did when the launch was its own.
#pragma once
#include <hip/hip_runtime.h>

namespace sahs {

constexpr int GT = 128, GK = 16;   // GEMM tile (128 x 128) and K-step

// ---- the per-layer walk's GEMMs --------------------------------------------------------------------------------------------
// An operand the LDS-DMA kernels can stream: 16-byte aligned rows.
bool gemm_aligned(const void *p, long ld);
// dX[P x N] (mode 0: =, 1: +=) dY[P x K] * W[K x N] (* mask > 0 ? 1 : slope).  K % GK == 0 and dY aligned: the LDS-DMA kernel, in f32
// products (W: aligned rows) or, x3, on the bf16 pipe (W: the pre-split fragment-ordered pieces of a CopyJob pack); anything else: the
// register-staged f32 kernel.  bits: the sign bits of `mask` that gemm_tn left (or null).
void gemm_nn(hipStream_t st, bool x3, long P, const float *dY, long ldy, int K, const float *W, long ldw, int N, float *dX, long ldx, int mode,
             const float *mask, long ldm, float slope, const float *zero, unsigned char *bits);
// dW[M x N] += dY[P x M]^T * X[P x N];  db != null: db[M] += column sums of dY.  sign_bits != null: the sign bits of X are left there
// when the launch can write them (both operands aligned, N % 8 == 0, N <= 256) -- *bits_written says whether.  Returns a hipError_t.
int gemm_tn(hipStream_t st, bool x3, long P, const float *dY, long ldy, int M, const float *X, long ldx, int N, float *dW, long ldw, float *db,
            const float *zero, unsigned char *sign_bits, bool *bits_written);

// ---- the fused walk's weight gradients: ALL of a part's dW (+ db) = dY^T X in one launch per tile class ----------------------------
// job = one layer's dW (+ db) with dY, X dense [P x width] planes.  The table travels as kernel arguments (no upload, nothing allocated).
struct TnJob { const float *A; const float *B; float *C; float *rowsum; long lda, ldb, ldc; int M, N; };
constexpr int MAX_TN_JOBS = 40;
struct TnBatch { TnJob j[MAX_TN_JOBS]; };
static_assert(sizeof(TnBatch) <= 3072, "kernel-argument budget");
struct TnPlan;

// the job tables of one part -> one launch each: the wide layers (M, N in (128, 256]: whole 256 x 256 blocks per workgroup) and the rest
struct TnList {
    TnBatch b, w; int n = 0, tiles = 0, nw = 0;
    void add(const float *dY, long ldy, int M, const float *X, long ldx, int N, float *dW, long ldw, float *db = nullptr);
    int launch(long P, const float *zero, int num_cu, hipStream_t st, bool f32);
    // units with relative K-step costs -> ranges per unit so that `slots` items of equal cost come out (ranges of >= 1024 samples)
    static bool make_plan(TnPlan &pl, const float *cost, int nunits, long slots, long P);
    int launch_f32(long P, const float *zero, int num_cu, hipStream_t st);
};

// ---- the walk's small launches, batched: job lists travel as kernel arguments (no table upload, nothing allocated) ----
// Everything a walk adds into the SHARED gradient buffers (grad_flat, grad_cond) is an atomicAdd: two walks -- the two levels' radiance parts, the
// two deformation parts -- may run at once on two streams (ops.RenderRaysFn.backward).
// (1) 16-byte aligned copies of the weight sub-matrices the data-gradient GEMMs stream by LDS-DMA: all of a walk's copies in ONE launch
//     in front of it (the walk is run once dry to collect them); (2) the per-frame-constant columns and (3) the bias gradients that went
//     through scratch: their results are read by nothing inside the walk, so they are deferred to one launch each at its end.
struct CopyJob { const float *src; float *dst; long lds_, ldd; int K, N; int pack; };
// pack = 1: dst is not a plain copy but the weight sub-matrix W[K x N] (K a multiple of 16) as the data-gradient GEMM's B operand, split and
// in MFMA fragment order: per (16-row K-step, 128-column block) one 8 KB piece [hi: 4 n-tiles x 64 lanes x 8 bf16 | lo: the same], lane
// (r, h) of n-tile t holding W[16 step + 8h + j][128 block + 32 t + r], j = 0..7 -- so the kernel's B tile is a linear 8 KB copy and a
// fragment is one ds_read_b128, with no conversion work in the GEMM (columns past N are zero).  Pieces in (step, block) order.
struct ConstJob { const float *W; float *dW; const float *db, *c; float *dc; long ld; int rows, cols, col0; };
struct AxpyJob { const float *x; float *y; int n; };
// A full table fails the walk (hipErrorOutOfMemory); no model comes near.  Jobs per flush, read off the walks in field_bwd.hip:
//   per-layer walk, all parts   axpy 12 (6 head rows + the 6 layers with folded constants), const 10 (trunk 2, hyper 4, warp 4) for the
//                               audio model and the NeRFaceModel; axpy 8, const 2 for the NeRFaceModel without deformation nets
//   fused walk, radiance part   axpy 8, const 2 (every model);   deformation part   axpy 4, const 8
constexpr int MAX_COPY_JOBS = 48, MAX_CONST_JOBS = 24, MAX_AXPY_JOBS = 24;
struct CopyBatch { CopyJob j[MAX_COPY_JOBS]; };
struct ConstBatch { ConstJob j[MAX_CONST_JOBS]; };
struct AxpyBatch { AxpyJob j[MAX_AXPY_JOBS]; };

// dst[m*ldd + n] (op)= src[m*lds + n] for n < N   (mode 0 copy, 1 add), on `blocks` workgroups
void copy2d(hipStream_t st, unsigned blocks, long M, int N, const float *src, long lds_, float *dst, long ldd, int mode);
// jobs 0 .. n-1 of the batch; phase 0: the plain copies, 1: the pack jobs (a pack job may read what a plain copy wrote)
void copy2d_batch(hipStream_t st, const CopyBatch &b, int n, int phase);
// per-frame constants: dW[r][col0 + k] += db[r] * c[k];  dc[k] += sum_r W[r][col0 + k] * db[r]
void const_cols_batch(hipStream_t st, const ConstBatch &b, int n);      // (cols <= 256 in every job)
// y[i] += x[i] (atomic), one workgroup per job
void axpy_batch(hipStream_t st, const AxpyBatch &b, int n);
// y[i] += a[i] over n float4s
void add_rows8(hipStream_t st, long n, const float *a, float *y);

}  // namespace sahs
