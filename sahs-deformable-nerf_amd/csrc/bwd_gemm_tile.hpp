// bwd_gemm_tile.hpp -- device-side pieces shared by field_bwd_gemm.hip (the per-layer walk's GEMMs and the small helpers) and
// field_bwd_tn_jobs.hip (the fused walk's job-table weight-gradient kernels): the vector types, lds_barrier, the bf16 operand split
// (split8, mfma3), the LDS positions frag_pos / swz_col, emit_sign_bits, and tn_tile -- one 128 x 128 tile of dW on the bf16 pipe, the
// body of gemm_tn_split_kernel (per-layer walk) and gemm_tn_jobs_kernel (fused).  Everything is __forceinline__ into its kernel.
// The fetch plan (K-major [16 k][128 cols] operand tiles by LDS-DMA, row pairs per instruction, XOR-swizzle by 16 floats on odd rows, zero
// page for what does not exist) is written out in each of its five users, marked "own copy of the fetch plan": as one function it changed
// every user's address arithmetic (LAB_NOTES, "Backward GEMMs: one file per user").
#pragma once
#include <hip/hip_runtime.h>
#include "sahs_common.hpp"
#include "field_bwd_gemm.hpp"

namespace sahs {

typedef __attribute__((address_space(3))) void *lds_void_t;
typedef const __attribute__((address_space(1))) void *gbl_void_t;
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
constexpr int DTILE = GK * GT;                // floats per operand tile of one K-step (8 KB)

// workgroup barrier that orders LDS traffic only: __syncthreads() is a full fence and makes the compiler drain vmcnt too, i.e. wait for every
// outstanding global STORE to be acknowledged -- not needed where the barrier only protects a staging buffer in LDS
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// eight fp32 values (this lane's k = 8h .. 8h+7 of one row/column) -> the bf16x8 MFMA fragments of their hi and lo parts
__device__ __forceinline__ void split8(const float (&x)[8], u32x4_t &hi, u32x4_t &lo)
{
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const uint32_t h = __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2_t{x[2 * p], x[2 * p + 1]}, bf16x2_t));
        hi[p] = h;
        lo[p] = __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2_t{x[2 * p] - __builtin_bit_cast(float, h << 16),
                                                                             x[2 * p + 1] - __builtin_bit_cast(float, h & 0xffff0000u)}, bf16x2_t));
    }
}
__device__ __forceinline__ f32x16_t mfma3(const u32x4_t &ah, const u32x4_t &al, const u32x4_t &bh, const u32x4_t &bl, f32x16_t c)
{
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, ah), __builtin_bit_cast(bf16x8_t, bh), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, ah), __builtin_bit_cast(bf16x8_t, bl), c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, al), __builtin_bit_cast(bf16x8_t, bh), c, 0, 0, 0);
    return c;
}
// position (dwords) of column `col`'s 4 dwords (8 bf16: samples 8 h .. 8 h + 7 of a K-step) inside one [hi] or [lo] fragment block of GT
// columns: [32-column group][h][column of the group][4 dwords] -- the MFMA phase's lane (r32, h) and the split phase's thread (column, h) both
// touch 16 bytes at 16 x lane: conflict-free ds_read_b128 / ds_write_b128.  (Round 4, first form: [column][h][4 dwords] = a 32-byte lane
// stride, two lanes per bank group -- SQ_LDS_BANK_CONFLICT 1.5-1.7 x SQ_ACTIVE_INST_LDS in both weight-gradient kernels.)
__device__ __forceinline__ constexpr int frag_pos(int col, int h) { return ((col >> 5) * 64 + h * 32 + (col & 31)) * 4; }
// float position of column `col` in a K-major tile row whose swizzle bit is `odd`
__device__ __forceinline__ int swz_col(int col, int odd) { return (((col >> 2) ^ (odd << 2)) << 2) + (col & 3); }

// The sign pattern of an activation matrix X as a bit matrix, row r = N/8 bytes, bit (n & 7) of byte n >> 3 set where X[r][n] > 0.  The
// weight-gradient GEMM WRITES it for its B operand X from the tiles it stages anyway (the m-block-0 workgroups); the data-gradient GEMM of the
// same layer, which follows it and whose (leaky-)ReLU mask is that same X, READS it instead of the fp32 matrix -- 1/32 of the bytes of what
// was a third of its HBM traffic.  Here: threads 0..255 of the workgroup, thread (kk, g) packs the 8 columns 8g .. 8g+7 of sample row kk
// of the X tile `Xs` (K-major, swizzled on odd rows) of the K-step that starts at sample k0 into one byte.
__device__ __forceinline__ void emit_sign_bits(const float *Xs, int tid, long k0, long k_hi, int n0, int N, unsigned char *__restrict__ bits)
{
    const int kk = tid >> 4, g = tid & 15;
    const long k = k0 + kk;
    if (k < k_hi && n0 + 8 * g < N) {
        const float *px = Xs + kk * GT + 4 * ((2 * g) ^ ((kk & 1) << 2));     // chunks 2g, 2g+1 stay adjacent under the swizzle
        const f32x4 v0 = *reinterpret_cast<const f32x4 *>(px), v1 = *reinterpret_cast<const f32x4 *>(px + 4);
        unsigned b8 = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) b8 |= (v0[i] > 0.0f ? 1u : 0u) << i | (v1[i] > 0.0f ? 1u : 0u) << (4 + i);
        bits[k * (N >> 3) + (n0 >> 3) + g] = (unsigned char)b8;
    }
}

// ------------------------------------------------------------------------------------------------
// The weight-gradient GEMM on the bf16 pipe, operands split ONCE per workgroup (round 3).  Splitting every fp32 operand value on its way from
// LDS into the MFMA -- in each of the two waves that use it, behind eight scalar LDS reads per fragment -- made a K-step body of 286
// instructions per wave for 12 MFMAs, and that body bounded the kernel: s_memtime stamps (tools/stamp_gemm.py) put 2,250 of a K-step's 2,530
// cycles into it, 120 into the wait for the LDS-DMA and 155 into the barrier.  Here a K-step is two phases:
//   split   thread (operand = tid >> 7, column = tid & 127) reads its column's 16 samples of the fp32 stage (conflict-free: a wave reads 64
//           consecutive columns of one sample row), splits them (48 VALU instructions) and writes the column's hi and lo bf16 fragments
//           [column][16 k] with four ds_write_b128; the bias-gradient column sum rides on the same registers;
//   MFMA    a wave fetches its 2 + 2 (hi, lo) fragment pairs with eight ds_read_b128 (lane (r32, h): 16 bytes at column * 32 + 16 h) and
//           issues the 12 MFMAs.
// Tiles, XCD-aware 1-D grid, sign-bit emission, staged atomic epilogue and arguments as gemm_dma_kernel<true, false>, the f32 form;
// 64 KB ring (depth 4) + 16 KB fragments = 80 KB of LDS: two workgroups per CU.
constexpr int TN_DST = 4, TN_THREADS = 512;
constexpr int TN_RING_FLOATS = TN_DST * 2 * DTILE;
constexpr int TN_FRAG_DWORDS = 2 * 2 * GT * 8;             // [operand][hi | lo][column][8 dwords = 16 bf16]
constexpr int TN_LDS_BYTES = (TN_RING_FLOATS + TN_FRAG_DWORDS) * 4;
static_assert(TN_LDS_BYTES == 81920, "two workgroups per CU: 2 x 80 KB = the 160 KB of a gfx950 CU");

// One 128 x 128 tile of C += A^T B over the samples [k_lo, k_hi): the body shared by the per-layer kernel (one tile-slab per workgroup)
// and the job-table kernel (a workgroup walks many).  Ends on an LDS barrier: the ring and the fragment buffer are free on return.
__device__ __forceinline__ void tn_tile(float *tn_lds, int M, int N, const float *__restrict__ A, long lda, const float *__restrict__ B, long ldb,
                                        float *__restrict__ C, long ldc, long k_lo, long k_hi, float *__restrict__ rowsum, int bx, int by,
                                        const float *__restrict__ zero, unsigned char *__restrict__ bits)
{
    float *ring = tn_lds;                                                    // [TN_DST][2][DTILE]
    uint32_t *frag = reinterpret_cast<uint32_t *>(tn_lds + TN_RING_FLOATS);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 2, wn = wave & 3, h = lane >> 5, r32 = lane & 31, c32 = lane & 31;
    const long m0 = (long)by * GT;
    const int n0 = bx * GT;
    const int T = (int)((k_hi - k_lo + GK - 1) / GK);
    const bool do_sum = rowsum != nullptr && bx == 0;

    // own copy of the fetch plan (head of this file): two DMA instructions per wave and K-step, waves 0..3 move the dY tile, waves 4..7 the
    // X tile, indexed issue (the sign-bit pass relies on the odd-row swizzle)
    const float *src[2]; long step[2]; int krow[2]; bool colok[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int rp = (wave & 3) * 2 + u;
        const float *base = (wave < 4) ? A : B;
        const long ld = (wave < 4) ? lda : ldb;
        const long c0 = (wave < 4) ? m0 : n0;
        const int dim = (wave < 4) ? M : N;
        const int row = 2 * rp + h;
        const int j = c32 ^ ((row & 1) << 2);
        src[u] = base + (k_lo + row) * ld + c0 + 4 * j;
        step[u] = GK * ld;
        krow[u] = row;
        colok[u] = c0 + 4 * j < dim;
    }
    const int dst_off = ((wave < 4) ? 0 : DTILE) + (wave & 3) * 2 * 256;
    auto issue = [&](int t) {
        float *dstb = ring + (t % TN_DST) * 2 * DTILE + dst_off;
        const long k0 = k_lo + (long)t * GK;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const float *g = (colok[u] && k0 + krow[u] < k_hi) ? src[u] + (long)t * step[u] : zero;
#if defined(SAHS_DIAG) && defined(SAHS_TN_NODMA)      // timing-only (results wrong by construction): the K loop without its operand fetch
            asm volatile("" :: "v"(g), "v"(dstb));
#else
            __builtin_amdgcn_global_load_lds((gbl_void_t)g, (lds_void_t)(dstb + u * 256), 16, 0, 0);
#endif
        }
    };
    // split phase: this thread's column of its operand tile, at its two swizzle positions (even / odd sample rows)
    const int sop = tid >> 8, skh = (tid >> 7) & 1, scol = tid & 127;        // samples 8 skh .. 8 skh + 7 of the column
    const int spos0 = scol, spos1 = (((scol >> 2) ^ 4) << 2) + (scol & 3);
    uint32_t *fdst = frag + (sop * 2) * GT * 8 + frag_pos(scol, skh);        // hi block of this column; the lo block is GT * 8 dwords further
    // MFMA phase: fragment rows of this wave's 2 + 2 column blocks
    const uint32_t *fa[2], *fb;                                              // wave (wm, wn): rows 64 wm + 32 i, columns 32 wn
#pragma unroll
    for (int i = 0; i < 2; ++i) fa[i] = frag + (0 * 2) * GT * 8 + frag_pos(64 * wm + 32 * i + r32, h);
    fb = frag + (1 * 2) * GT * 8 + frag_pos(32 * wn + r32, h);
    f32x16_t acx[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) acx[i][e] = 0.0f;
    float cs = 0.0f;

    // vmcnt accounting as in gemm_dma_kernel: the wave's only loads are its 2 LDS-DMA instructions per issue(), completing in issue order;
    // anything older still in flight (the sign-bit stores, a previous tile's atomics) can only make a counted wait stricter
    if (T > 0) issue(0);
    if (T > 1) issue(1);
    if (T > 2) issue(2);
    for (int t = 0; t < T; ++t) {
        if (t + 2 < T) asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");
        else if (t + 1 < T) asm volatile("s_waitcnt vmcnt(2)\n\ts_barrier" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        // (every wave has finished the MFMA phase of step t-1: the fragment buffer and ring stage (t-1) % 4 are free)
        if (t + TN_DST - 1 < T) issue(t + TN_DST - 1);
        const float *stage = ring + (t % TN_DST) * 2 * DTILE;
        {
            const float *col = stage + sop * DTILE + 8 * skh * GT;
            float x[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) x[k] = col[k * GT + ((k & 1) ? spos1 : spos0)];
            u32x4_t hi, lo;
            split8(x, hi, lo);
            *reinterpret_cast<u32x4_t *>(fdst) = hi;
            *reinterpret_cast<u32x4_t *>(fdst + GT * 8) = lo;
            if (do_sum && sop == 0) {
#pragma unroll
                for (int k = 0; k < 8; ++k) cs += x[k];
            }
        }
        if (bits != nullptr && by == 0 && tid < 256) emit_sign_bits(stage + DTILE, tid, k_lo + (long)t * GK, k_hi, n0, N, bits);
        lds_barrier();
        u32x4_t ah[2], al[2], bh, bl;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            ah[i] = *reinterpret_cast<const u32x4_t *>(fa[i]);
            al[i] = *reinterpret_cast<const u32x4_t *>(fa[i] + GT * 8);
        }
        bh = *reinterpret_cast<const u32x4_t *>(fb);
        bl = *reinterpret_cast<const u32x4_t *>(fb + GT * 8);
#pragma unroll
        for (int i = 0; i < 2; ++i) acx[i] = mfma3(ah[i], al[i], bh, bl, acx[i]);
    }
    // epilogue through LDS: one atomic instruction covers 256 contiguous bytes of a dW row.  Accumulator tile i register e is
    // row 32 i + (e & 3) + 8 (e >> 2) + 4 h, column r32 of this wave's 64 x 32 block
    // (own copy of the staged atomic epilogue: shared with gemm_dma_kernel's as one function, the staging writes of both paired otherwise)
    constexpr int SLD = GT + 4;
    float *out = ring;                                   // 64 x 132 floats = 33 KB of the ring, free after the K loop
    __syncthreads();
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        if (wm == half) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) out[(32 * i + (e & 3) + 8 * (e >> 2) + 4 * h) * SLD + 32 * wn + r32] = acx[i][e];
        }
        lds_barrier();
#pragma unroll 4
        for (int e = 0; e < 16; ++e) {
            const int idx = tid + TN_THREADS * e, row = idx >> 7, col = idx & 127;
            const long m = m0 + 64 * half + row;
            const int n = n0 + col;
            if (m < M && n < N && ldc > 0) atomicAdd(C + m * ldc + n, out[row * SLD + col]);
        }
        lds_barrier();
    }
    if (do_sum && sop == 0 && m0 + scol < M) atomicAdd(rowsum + m0 + scol, cs);      // (two partial sums per column: samples 0..7 and 8..15 of every step)
}

}  // namespace sahs
