// field_bwd_tn_jobs.hip -- the fused walk's weight gradients: ALL dW (+ db) = dY^T X of a part in one launch per tile class, from a job
// table (TnList, field_bwd_gemm.hpp).  Four kernels: 128 x 128 tiles and whole 256 x 256 blocks, each on the bf16 pipe with split operands
// (default) and in exact fp32 products.  These run in every training step.  Model-independent, built once; the tile body of the narrow
// bf16 kernel (tn_tile, shared with the per-layer walk's gemm_tn_split_kernel), the bf16 split and the description of the operand fetch that
// all four use are in bwd_gemm_tile.hpp.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "sahs_common.hpp"
#include "field_bwd_gemm.hpp"
#include "bwd_gemm_tile.hpp"
#if SAHS_MODEL != 0
#error "field_bwd_tn_jobs.hip is model-independent: built once, without -DSAHS_MODEL"
#endif
// ONE translation unit with the per-layer walk's kernels (this file is the one build.py compiles): the compiler sets up a kernel's
// workgroup ids and allocates registers around the out-of-line __ockl_get_* calls from ALL kernels of a unit, so compiled apart every
// kernel of both files gets another prologue.  Retiring the per-layer walk deletes that file and this line.
#include "field_bwd_gemm.hip"

namespace sahs {

// ------------------------------------------------------------------------------------------------
// ALL weight-gradient GEMMs of a walk in ONE launch (round 4).  Per launch the per-layer kernel (gemm_tn_split_kernel) pays ring fill, a K
// loop with one workgroup per CU, 64 KB of atomics per workgroup, ramp and tail -- 35-40 us of a 45-200 us launch, 82 times per training
// step.  Here persistent workgroups (two per CU) walk a job table: job = one layer's dW (+ db) = dY^T X with dY, X dense
// [P x width] planes; item = (sample range r, job, 128 x 128 tile), ranges of `range` samples (the same for every job: items cost the same),
// item index = r * tiles_total + tile, so that the tiles of one job and range -- which stream the same dY and X rows -- sit on neighbouring
// workgroups of ONE XCD (virtual id below) at the same time and share that L2's fetches.  A range is ~10 k samples instead of the 512 of
// a slab: 20 x fewer atomic epilogues.  The table (TnJob / TnBatch, field_bwd_gemm.hpp) travels as kernel arguments.
__global__ void __launch_bounds__(TN_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) gemm_tn_jobs_kernel(TnBatch jobs, int njobs, int tiles_total, long P, long range,
                                                                                                             const float *__restrict__ zero)
{
    extern __shared__ __attribute__((aligned(16))) float tn_lds[];
    const int G = gridDim.x;                                                  // a multiple of 8
    const int vid = (blockIdx.x & 7) * (G >> 3) + (blockIdx.x >> 3);          // consecutive virtual ids = consecutive slots of one XCD
    const long nrange = (P + range - 1) / range;
    const long items = nrange * tiles_total;
    for (long it = vid; it < items; it += G) {
        const long r = it / tiles_total;
        int tg = (int)(it - r * tiles_total), j = 0;
        for (; j < njobs - 1; ++j) {
            const int tj = ((jobs.j[j].N + GT - 1) / GT) * ((jobs.j[j].M + GT - 1) / GT);
            if (tg < tj) break;
            tg -= tj;
        }
        const TnJob &J = jobs.j[j];
        const int nx = (J.N + GT - 1) / GT;
        const long k_lo = r * range, k_hi = (k_lo + range < P) ? k_lo + range : P;
        tn_tile(tn_lds, J.M, J.N, J.A, J.lda, J.B, J.ldb, J.C, J.ldc, k_lo, k_hi, J.rowsum, tg % nx, tg / nx, zero, nullptr);
    }
}

// ------------------------------------------------------------------------------------------------
// The wide layers' weight gradients as 256 x 256 BLOCKS (round 4).  With 128 x 128 tiles a 256 x 256 layer is four workgroups that each
// stream 128 columns of dY and 128 of X: every operand byte is fetched twice unless the four happen to run in step on one XCD (measured on
// the training step: 21 GB fetched per step for 15.9 GB of operands, at 5 TB/s -- the launch is HBM-bound, so the re-reads are its time).
// Here ONE workgroup owns the whole 256 x 256 block of a job over a sample range: per 16-sample K-step it brings in 16 x 256 of dY and
// 16 x 256 of X once (32 KB by LDS-DMA, ring of four), splits both into bf16 hi / lo fragments once, and its eight waves (4 along M x 2
// along N, a 64 x 128 sub-block = eight 32 x 32 accumulators each) issue 24 MFMAs per wave and K-step.  160 KB of LDS: one workgroup per
// CU, two waves per SIMD.  The accumulators go out as atomics straight from the registers: one register of a 32 x 32 accumulator is two
// 128-byte row segments, which the memory side takes at full rate (MI355X_MICROARCH.md, global float atomics) -- no staging pass.
// Jobs: M, N <= 256 (columns past M / N come from the zero page); the narrower jobs stay with the 128 x 128 kernel above.
constexpr int TW_DST = 3, TW_UNITS = 4;                                       // ring depth; 128-column operand blocks per K-step (2 of dY + 2 of X)
constexpr int TW_STAGE_FLOATS = TW_UNITS * DTILE;                              // 8192 floats = 32 KB
constexpr int TW_RING_FLOATS = TW_DST * TW_STAGE_FLOATS;
constexpr int TW_FRAG_DWORDS = TW_UNITS * 2 * GT * 8;                          // [block][hi | lo][frag_pos(column, h)]: 32 KB, two of them
constexpr int TW_LDS_BYTES = (TW_RING_FLOATS + 2 * TW_FRAG_DWORDS) * 4;
static_assert(TW_LDS_BYTES == 163840, "one workgroup per CU: all 160 KB of it");

// Software-pipelined: while the MFMAs of K-step t run from fragment buffer t & 1, the same waves split K-step t + 1 from the ring into the
// other fragment buffer (VALU and LDS work beside the matrix pipe instead of in turns with it: in turns the kernel was instruction-bound at
// 2 us per K-step, 3.7 TB/s), ONE barrier per K-step, two K-steps of LDS-DMA in flight behind the one being split.
__device__ __forceinline__ void tn_block256(float *tn_lds, int M, int N, const float *__restrict__ A, long lda, const float *__restrict__ B, long ldb,
                                            float *__restrict__ C, long ldc, long k_lo, long k_hi, float *__restrict__ rowsum,
                                            const float *__restrict__ zero)
{
    float *ring = tn_lds;                                                      // [TW_DST][block 0..3][16 k][128 cols]; blocks 0, 1 = dY, 2, 3 = X
    uint32_t *frag = reinterpret_cast<uint32_t *>(tn_lds + TW_RING_FLOATS);   // [2][TW_FRAG_DWORDS]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1, h = lane >> 5, r32 = lane & 31, c32 = lane & 31;
    const int T = (int)((k_hi - k_lo + GK - 1) / GK);
    // own copy of the fetch plan (bwd_gemm_tile.hpp), indexed issue: 32 one-KB units per K-step (block b, row pair rp); wave w moves
    // units 4 w .. 4 w + 3 = row pairs 4 (w & 1) .. of block w >> 1
    const float *src[4]; long step[4]; int krow[4]; bool colok[4];
    const int blk = wave >> 1;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int rp = (wave & 1) * 4 + u;
        const float *base = (blk < 2) ? A : B;
        const long ld = (blk < 2) ? lda : ldb;
        const int c0 = (blk & 1) * GT;
        const int dim = (blk < 2) ? M : N;
        const int row = 2 * rp + h;
        const int j = c32 ^ ((row & 1) << 2);
        src[u] = base + (k_lo + row) * ld + c0 + 4 * j;
        step[u] = GK * ld;
        krow[u] = row;
        colok[u] = c0 + 4 * j < dim;
    }
    const int dst_off = blk * DTILE + (wave & 1) * 4 * 256;
    auto issue = [&](int t) {
        float *dstb = ring + (t % TW_DST) * TW_STAGE_FLOATS + dst_off;
        const long k0 = k_lo + (long)t * GK;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float *g = (colok[u] && k0 + krow[u] < k_hi) ? src[u] + (long)t * step[u] : zero;
#if defined(SAHS_DIAG) && defined(SAHS_TN_NODMA)      // timing-only (results wrong by construction): the K loop without its operand fetch
            asm volatile("" :: "v"(g), "v"(dstb));
#else
            __builtin_amdgcn_global_load_lds((gbl_void_t)g, (lds_void_t)(dstb + u * 256), 16, 0, 0);
#endif
        }
    };
    // split, two rounds per K-step: round r, thread -> block 2 r + (tid >> 8), samples 8 skh .. 8 skh + 7 of column scol (round 0: the dY blocks)
    const int sb = tid >> 8, skh = (tid >> 7) & 1, scol = tid & 127;
    const int spos0 = scol, spos1 = (((scol >> 2) ^ 4) << 2) + (scol & 3);
    float cs = 0.0f;
    auto split_round = [&](int t, int r) {
        const float *col = ring + (t % TW_DST) * TW_STAGE_FLOATS + (2 * r + sb) * DTILE + 8 * skh * GT;
        float x[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = col[k * GT + ((k & 1) ? spos1 : spos0)];
        u32x4_t hi, lo;
        split8(x, hi, lo);
        uint32_t *fdst = frag + (t & 1) * TW_FRAG_DWORDS + ((2 * r + sb) * 2) * GT * 8 + frag_pos(scol, skh);
        *reinterpret_cast<u32x4_t *>(fdst) = hi;
        *reinterpret_cast<u32x4_t *>(fdst + GT * 8) = lo;
        if (r == 0 && rowsum != nullptr) {
#pragma unroll
            for (int k = 0; k < 8; ++k) cs += x[k];
        }
    };
    // MFMA: wave (wm, wn) owns rows 64 wm .. + 63 (dY block wm >> 1), columns 128 wn .. + 127 (X block wn)
    int fa[2], fb[4];      // dword offsets inside a fragment buffer
#pragma unroll
    for (int i = 0; i < 2; ++i) fa[i] = ((wm >> 1) * 2) * GT * 8 + frag_pos(64 * (wm & 1) + 32 * i + r32, h);
#pragma unroll
    for (int j = 0; j < 4; ++j) fb[j] = ((2 + wn) * 2) * GT * 8 + frag_pos(32 * j + r32, h);
    f32x16_t acx[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acx[i][j][e] = 0.0f;

    // vmcnt accounting as in tn_tile: this wave's loads are its 4 LDS-DMA instructions per issue(), in issue order; anything older still in
    // flight (a previous item's atomics) can only make a counted wait stricter
    if (T > 0) issue(0);
    if (T > 1) issue(1);
    if (T > 2) issue(2);
    if (T > 0) {      // K-step 0 has landed when at most the 8 DMA instructions of steps 1, 2 are outstanding
        if (T > 2) asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");
        else if (T > 1) asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        split_round(0, 0);
        split_round(0, 1);
    }
    for (int t = 0; t < T; ++t) {
        // K-step t + 1 has landed (t + 2 may be in flight); every wave has finished the MFMAs of step t - 1 and the split of step t
        if (t + 2 < T) asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (t + 3 < T) issue(t + 3);                         // into stage t % 3, which the split of step t (last iteration) was the last to read
        const uint32_t *fr = frag + (t & 1) * TW_FRAG_DWORDS;
        u32x4_t ah[2], al[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            ah[i] = *reinterpret_cast<const u32x4_t *>(fr + fa[i]);
            al[i] = *reinterpret_cast<const u32x4_t *>(fr + fa[i] + GT * 8);
        }
        // every fragment of the K-step is requested before the first MFMA (the compiler otherwise reads a column block's pair right in front of
        // its six MFMAs and waits: four exposed LDS round trips per K-step with two waves per SIMD to cover them)
        u32x4_t bh[4], bl[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bh[j] = *reinterpret_cast<const u32x4_t *>(fr + fb[j]);
            bl[j] = *reinterpret_cast<const u32x4_t *>(fr + fb[j] + GT * 8);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int i = 0; i < 2; ++i) acx[i][j] = mfma3(ah[i], al[i], bh[j], bl[j], acx[i][j]);
            if (t + 1 < T && (j & 1) == 0) split_round(t + 1, j >> 1);      // beside the MFMAs: the next K-step's fragments
        }
    }
    // accumulator (i, j) register e: row 64 wm + 32 i + (e & 3) + 8 (e >> 2) + 4 h, column 128 wn + 32 j + r32
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = 128 * wn + 32 * j + r32;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = 64 * wm + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (m < M && n < N) atomicAdd(C + (long)m * ldc + n, acx[i][j][e]);
            }
        }
    if (rowsum != nullptr && sb * GT + scol < M) atomicAdd(rowsum + sb * GT + scol, cs);      // (two partial sums per column: samples 0..7 and 8..15 of every step)
    __syncthreads();      // the ring and the fragment buffers are free (and this item's DMA has long drained) before the next item issues into them
}

__global__ void __launch_bounds__(TN_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) gemm_tn_jobs256_kernel(TnBatch jobs, int njobs, long P, long range,
                                                                                                               const float *__restrict__ zero)
{
    extern __shared__ __attribute__((aligned(16))) float tn_lds[];
    const long nrange = (P + range - 1) / range;
    const long items = nrange * njobs;                                        // item = (range r, job): the jobs of one range side by side
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const long r = it / njobs;
        const TnJob &J = jobs.j[(int)(it - r * njobs)];
        const long k_lo = r * range, k_hi = (k_lo + range < P) ? k_lo + range : P;
        tn_block256(tn_lds, J.M, J.N, J.A, J.lda, J.B, J.ldb, J.C, J.ldc, k_lo, k_hi, J.rowsum, zero);
    }
}

// ------------------------------------------------------------------------------------------------
// The same two job-table launches in exact fp32 products (ops.backward_gemm_precision("fp32"): the reference's arithmetic), on
// v_mfma_f32_16x16x4_f32.  Same operand tiles ([16 k][128 cols] K-major, XOR-swizzled on odd rows) brought in by the same LDS-DMA ring; no
// split phase: the MFMA lanes read their operands straight from the ring (lane (q, c16): sample 4 s4 + q, column 16 i + c16 -- ds_read_b32, conflict-free under
// the swizzle), four samples per MFMA.  Bound: the f32 matrix pipe -- a 256 x 256 block is 128 MFMAs per wave and K-step (4096 cycles)
// against 32 KB of operands -- not HBM.  Ring of four K-steps.
constexpr int TF_DST = 4;
constexpr int TF_LDS_BYTES = TF_DST * 2 * DTILE * 4;                           // 64 KB: two workgroups per CU
constexpr int TFW_DST = 5;                                                     // the wide kernel's ring: all 160 KB of the CU, four K-steps in flight
constexpr int TFW_LDS_BYTES = TFW_DST * TW_STAGE_FLOATS * 4;                   // 160 KB: one workgroup per CU

// One (up to) 128 x 128 tile of C += A^T B over the samples [k_lo, k_hi).  The tile's valid part is TR x TC 16 x 16 accumulators (a head's
// dW is 1 x 8, a 64-wide layer against PE(x) 4 x 4, a trunk layer against PE(w) 8 x 2): the eight waves are laid over it as RW x CW with
// CW = 4, 2, 1 for TC > 4, > 2, <= 2, a wave owning up to 4 x 2 accumulators -- only the valid ones are multiplied (wave-uniform bounds),
// and the work stays spread evenly over the four SIMDs (wave & 3).
__device__ __forceinline__ void tn_tile_f32(float *ring, int M, int N, const float *__restrict__ A, long lda, const float *__restrict__ B, long ldb,
                                            float *__restrict__ C, long ldc, long k_lo, long k_hi, float *__restrict__ rowsum, int bx, int by,
                                            const float *__restrict__ zero)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), h = lane >> 5, c32 = lane & 31, q = lane >> 4, c16 = lane & 15;
    const long m0 = (long)by * GT;
    const int n0 = bx * GT;
    const int T = (int)((k_hi - k_lo + GK - 1) / GK);
    const bool do_sum = rowsum != nullptr && bx == 0;
    const int mt = (int)(M - m0 < GT ? M - m0 : GT), nt = N - n0 < GT ? N - n0 : GT;
    const int TR = (mt + 15) >> 4, TC = (nt + 15) >> 4;
    const int CW = TC > 4 ? 4 : (TC > 2 ? 2 : 1), RW = 8 / CW, RPW = (TR + RW - 1) / RW;      // RPW <= 4
    const int wm = wave / CW, wn = wave % CW;
    const int rt0 = wm * RPW, ct0 = 2 * wn;
    const int ni = __builtin_amdgcn_readfirstlane(TR - rt0 < 0 ? 0 : (TR - rt0 < RPW ? TR - rt0 : RPW));
    const int nj = __builtin_amdgcn_readfirstlane(TC - ct0 < 0 ? 0 : (TC - ct0 < 2 ? TC - ct0 : 2));
    // own copy of the fetch plan (bwd_gemm_tile.hpp), advancing issue: as in tn_tile waves 0..3 move the dY tile, waves 4..7 the X tile, two
    // instructions per wave and K-step
    const float *cur[2]; long step[2]; int krow[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int rp = (wave & 3) * 2 + u;
        const float *base = (wave < 4) ? A : B;
        const long ld = (wave < 4) ? lda : ldb;
        const long c0 = (wave < 4) ? m0 : n0;
        const int dim = (wave < 4) ? M : N;
        const int row = 2 * rp + h;
        const int j = c32 ^ ((row & 1) << 2);
        const bool colok = c0 + 4 * j < dim;
        cur[u] = colok ? base + (k_lo + row) * ld + c0 + 4 * j : zero;
        step[u] = colok ? GK * ld : 0;
        krow[u] = row;
    }
    const int dst_off = ((wave < 4) ? 0 : DTILE) + (wave & 3) * 2 * 256;
    auto issue = [&](int t) {
        float *dstb = ring + (t % TF_DST) * 2 * DTILE + dst_off;
        const long k0 = k_lo + (long)t * GK;
        const bool tail = k0 + GK > k_hi;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const float *g = (tail && k0 + krow[u] >= k_hi) ? zero : cur[u];
#if defined(SAHS_DIAG) && defined(SAHS_TNF_NODMA)      // timing-only (results wrong by construction): the K loop without its operand fetch
            asm volatile("" :: "v"(g), "v"(dstb));
#else
            __builtin_amdgcn_global_load_lds((gbl_void_t)g, (lds_void_t)(dstb + u * 256), 16, 0, 0);
#endif
            cur[u] += step[u];
        }
    };
    int colA[4], colB[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) colA[i] = swz_col((16 * (rt0 + i) + c16) & (GT - 1), q & 1);
#pragma unroll
    for (int j = 0; j < 2; ++j) colB[j] = DTILE + swz_col((16 * (ct0 + j) + c16) & (GT - 1), q & 1);
    f32x4 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float cs = 0.0f;
    // vmcnt accounting as in tn_tile: the wave's only loads are its 2 LDS-DMA instructions per issue(), completing in issue order
    if (T > 0) issue(0);
    if (T > 1) issue(1);
    if (T > 2) issue(2);
    // The K loop, once per shape of the wave block (4, 2 or 1 row tiles by 2 column tiles; NI = 0: any other -- ragged widths -- with a uniform
    // guard per accumulator): the dispatch is outside the loop, so the loop body is MFMAs and operand reads only (with the guards inside, the
    // compiler put a vcc branch between any two of them)
    auto kloop = [&]<int NI, int NJ>() {
        for (int t = 0; t < T; ++t) {
            if (t + 2 < T) asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");
            else if (t + 1 < T) asm volatile("s_waitcnt vmcnt(2)\n\ts_barrier" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
            const float *stage = ring + (t % TF_DST) * 2 * DTILE;
            // K-step t + 3 goes into the stage every wave finished reading before the barrier above -- requested behind the first quarter of
            // this step's MFMAs, not in front of them: its address arithmetic then runs beside the matrix pipe instead of holding it up
            const bool work = NI > 0 || (ni > 0 && nj > 0);
            if (!work && t + TF_DST - 1 < T) issue(t + TF_DST - 1);
            if (work) {
#pragma unroll
                for (int s4 = 0; s4 < GK / 4; ++s4) {
                    if (s4 == 1 && t + TF_DST - 1 < T) issue(t + TF_DST - 1);
                    const float *row = stage + (4 * s4 + q) * GT;
                    if constexpr (NI > 0) {
                        float a[NI], b[NJ];
#pragma unroll
                        for (int i = 0; i < NI; ++i) a[i] = row[colA[i]];
#pragma unroll
                        for (int j = 0; j < NJ; ++j) b[j] = row[colB[j]];
#pragma unroll
                        for (int i = 0; i < NI; ++i)
#pragma unroll
                            for (int j = 0; j < NJ; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
#pragma unroll
                            for (int j = 0; j < 2; ++j)
                                if (i < ni && j < nj) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(row[colA[i]], row[colB[j]], acc[i][j], 0, 0, 0);
                    }
                }
            }
            if (do_sum && tid < GT) {      // (measured: the launch is as long without these sums, 0.650 vs 0.652 ms)
#pragma unroll
                for (int k = 0; k < GK; ++k) cs += stage[k * GT + swz_col(tid, k & 1)];
            }
        }
    };
    if (nj == 2 && ni == 4) kloop.template operator()<4, 2>();
    else if (nj == 2 && ni == 2) kloop.template operator()<2, 2>();
    else if (nj == 2 && ni == 1) kloop.template operator()<1, 2>();
    else kloop.template operator()<0, 0>();
    // accumulator (i, j) register r: row 16 (rt0 + i) + 4 q + r, column 16 (ct0 + j) + c16
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (i < ni && j < nj) {
                const int n = n0 + 16 * (ct0 + j) + c16;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const long m = m0 + 16 * (rt0 + i) + 4 * q + r;
                    if (m < M && n < N && ldc > 0) atomicAdd(C + m * ldc + n, acc[i][j][r]);
                }
            }
        }
    if (do_sum && tid < GT && m0 + tid < M) atomicAdd(rowsum + m0 + tid, cs);
    __syncthreads();      // the ring is free (this item's DMA has drained) before the next item issues into it
}

// The item table of an fp32 job launch.  Unit = one output tile (narrow kernel) or one 256 x 256 job (wide kernel); a unit's samples are
// cut into n ranges in proportion to what a K-step of it costs (a 16 x 128 head tile is 1/8 of the MFMAs of a 128 x 128 tile, a 128 x 256
// layer half of a 256 x 256 one), so that items cost the same and every workgroup gets the same number of them: with equal ranges the
// launch lasts as long as its dearest unit (measured: wide kernel 2.83 ms per 262,144 samples for 2.24 ms of matrix work in its longest item).
struct TnUnit { unsigned short start, n; unsigned char job, bx, by, pad; };
constexpr int MAX_TN_UNITS = 64;
struct TnPlan { TnUnit u[MAX_TN_UNITS]; int nunits, items; };
static_assert(sizeof(TnBatch) + sizeof(TnPlan) <= 3800, "kernel-argument budget");

// (the item lookup below -- item -> its unit and sample range [k_lo, k_hi); a unit's last range can lie past P after the rounding to
// K-steps and is skipped -- is written out in both fp32 kernels: as one function it changed how they load the plan's fields)
__global__ void __launch_bounds__(TN_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) gemm_tn_jobs_f32_kernel(TnBatch jobs, TnPlan plan, long P, const float *__restrict__ zero)
{
    extern __shared__ __attribute__((aligned(16))) float tn_lds[];
    const int G = gridDim.x;
    for (int it = blockIdx.x; it < plan.items; it += G) {
        int u = 0;
        while (u + 1 < plan.nunits && (int)plan.u[u + 1].start <= it) ++u;
        const TnUnit U = plan.u[u];
        const long range = ((P + U.n - 1) / U.n + 15) / 16 * 16;
        const long k_lo = (long)(it - U.start) * range, k_hi = (k_lo + range < P) ? k_lo + range : P;
        if (k_lo >= P) continue;
        const TnJob &J = jobs.j[U.job];
        tn_tile_f32(tn_lds, J.M, J.N, J.A, J.lda, J.B, J.ldb, J.C, J.ldc, k_lo, k_hi, J.rowsum, U.bx, U.by, zero);
    }
}

// One whole 256 x 256 block: wave (wm, wn) of eight owns rows 64 wm .. (dY block wm >> 1), columns 128 wn .. (X block wn): 4 x 8 accumulators
__device__ __forceinline__ void tn_block256_f32(float *ring, int M, int N, const float *__restrict__ A, long lda, const float *__restrict__ B, long ldb,
                                                float *__restrict__ C, long ldc, long k_lo, long k_hi, float *__restrict__ rowsum,
                                                const float *__restrict__ zero)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), wm = wave >> 1, wn = wave & 1, h = lane >> 5, c32 = lane & 31, q = lane >> 4, c16 = lane & 15;
    const int T = (int)((k_hi - k_lo + GK - 1) / GK);
    // own copy of the fetch plan (bwd_gemm_tile.hpp), advancing issue as in tn_tile_f32: 32 one-KB units per K-step (block b, row pair rp)
    // as in tn_block256; wave w moves row pairs 4 (w & 1) .. of block w >> 1
    const float *cur[4]; long step[4]; int krow[4];
    const int blk = wave >> 1;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int rp = (wave & 1) * 4 + u;
        const float *base = (blk < 2) ? A : B;
        const long ld = (blk < 2) ? lda : ldb;
        const int c0 = (blk & 1) * GT;
        const int dim = (blk < 2) ? M : N;
        const int row = 2 * rp + h;
        const int j = c32 ^ ((row & 1) << 2);
        const bool colok = c0 + 4 * j < dim;
        cur[u] = colok ? base + (k_lo + row) * ld + c0 + 4 * j : zero;
        step[u] = colok ? GK * ld : 0;
        krow[u] = row;
    }
    const int dst_off = blk * DTILE + (wave & 1) * 4 * 256;
    auto issue = [&](int t) {
        float *dstb = ring + (t % TFW_DST) * TW_STAGE_FLOATS + dst_off;
        const long k0 = k_lo + (long)t * GK;
        const bool tail = k0 + GK > k_hi;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float *g = (tail && k0 + krow[u] >= k_hi) ? zero : cur[u];
#if defined(SAHS_DIAG) && defined(SAHS_TNF_NODMA)      // timing-only (results wrong by construction): the K loop without its operand fetch
            asm volatile("" :: "v"(g), "v"(dstb));
#else
            __builtin_amdgcn_global_load_lds((gbl_void_t)g, (lds_void_t)(dstb + u * 256), 16, 0, 0);
#endif
            cur[u] += step[u];
        }
    };
    int colA[4], colB[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) colA[i] = (wm >> 1) * DTILE + swz_col(64 * (wm & 1) + 16 * i + c16, q & 1);
#pragma unroll
    for (int j = 0; j < 8; ++j) colB[j] = (2 + wn) * DTILE + swz_col(16 * j + c16, q & 1);
    f32x4 acc[4][8];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float cs = 0.0f;
    const int scol = (tid >> 7) * DTILE, sc = tid & 127;      // bias gradient: thread tid < 256 sums column tid of dY
    // vmcnt accounting: this wave's loads are its 4 LDS-DMA instructions per issue(), in issue order; anything older still in flight (a
    // previous item's atomics) can only make a counted wait stricter
    if (T > 0) issue(0);
    if (T > 1) issue(1);
    if (T > 2) issue(2);
    if (T > 3) issue(3);
    for (int t = 0; t < T; ++t) {
        if (t + 3 < T) asm volatile("s_waitcnt vmcnt(12)\n\ts_barrier" ::: "memory");
        else if (t + 2 < T) asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");
        else if (t + 1 < T) asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        const float *stage = ring + (t % TFW_DST) * TW_STAGE_FLOATS;
        const bool rows_valid = 64 * wm < M;      // (a 128 x 256 layer: waves 4..7 -- the second wave of every SIMD -- own rows of the zero page)
        if (!rows_valid && t + TFW_DST - 1 < T) issue(t + TFW_DST - 1);
        if (rows_valid) {
            // operands of sample group s4 + 1 are requested before the 32 MFMAs of group s4 (two register sets).  Measured MFMA busy 0.71 at
            // 2.35 GHz -- and the same launch time with the compiler's own read placement, with all four groups read up front and every
            // accumulator taking its four MFMAs in a row (the forward's pattern), with the DMA issue in front of the MFMAs, and without the
            // operand fetch (-7 %): LAB_NOTES R4.6
            float a[2][4], b[2][8];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[0][i] = stage[q * GT + colA[i]];
#pragma unroll
            for (int j = 0; j < 8; ++j) b[0][j] = stage[q * GT + colB[j]];
#pragma unroll
            for (int s4 = 0; s4 < GK / 4; ++s4) {
                if (s4 + 1 < GK / 4) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) a[(s4 + 1) & 1][i] = stage[(4 * (s4 + 1) + q) * GT + colA[i]];
#pragma unroll
                    for (int j = 0; j < 8; ++j) b[(s4 + 1) & 1][j] = stage[(4 * (s4 + 1) + q) * GT + colB[j]];
                }
                __builtin_amdgcn_sched_barrier(0);
                if (s4 == 1 && t + TFW_DST - 1 < T) issue(t + TFW_DST - 1);      // (behind the first quarter of the step's MFMAs: see tn_tile_f32)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
#if defined(SAHS_DIAG) && defined(SAHS_TNF_NOMFMA)      // timing-only (results wrong by construction): the K loop without its matrix work
                        acc[i][j][0] += a[s4 & 1][i] * b[s4 & 1][j];
#else
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s4 & 1][i], b[s4 & 1][j], acc[i][j], 0, 0, 0);
#endif
                    }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (rowsum != nullptr && tid < 2 * GT) {
#pragma unroll
            for (int k = 0; k < GK; ++k) cs += stage[scol + k * GT + swz_col(sc, k & 1)];
        }
    }
    // accumulator (i, j) register r: row 64 wm + 16 i + 4 q + r, column 128 wn + 16 j + c16
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int n = 128 * wn + 16 * j + c16;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = 64 * wm + 16 * i + 4 * q + r;
#if defined(SAHS_DIAG) && defined(SAHS_TNF_NOATOMIC)      // timing-only (results wrong by construction): the launch without its atomic epilogue
                if (64 * wm < M && m < M && n < N && acc[i][j][r] == 123.456f) C[(long)m * ldc + n] = 0.0f;
#else
                if (64 * wm < M && m < M && n < N) atomicAdd(C + (long)m * ldc + n, acc[i][j][r]);
#endif
            }
        }
    if (rowsum != nullptr && tid < 2 * GT && tid < M) atomicAdd(rowsum + tid, cs);
    __syncthreads();
}

__global__ void __launch_bounds__(TN_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) gemm_tn_jobs256_f32_kernel(TnBatch jobs, TnPlan plan, long P, const float *__restrict__ zero)
{
    extern __shared__ __attribute__((aligned(16))) float tn_lds[];
    for (int it = blockIdx.x; it < plan.items; it += gridDim.x) {
        int u = 0;
        while (u + 1 < plan.nunits && (int)plan.u[u + 1].start <= it) ++u;
        const TnUnit U = plan.u[u];
        const long range = ((P + U.n - 1) / U.n + 15) / 16 * 16;
        const long k_lo = (long)(it - U.start) * range, k_hi = (k_lo + range < P) ? k_lo + range : P;
        if (k_lo >= P) continue;
        const TnJob &J = jobs.j[U.job];
        tn_block256_f32(tn_lds, J.M, J.N, J.A, J.lda, J.B, J.ldb, J.C, J.ldc, k_lo, k_hi, J.rowsum, zero);
    }
}

// ---- the job tables of one part -> one launch each (TnList, field_bwd_gemm.hpp) ----
void TnList::add(const float *dY, long ldy, int M, const float *X, long ldx, int N, float *dW, long ldw, float *db)
{
    static const bool no_wide = sahs_diag_env("SAHS_BWD_TN_NOWIDE") != nullptr;      // (A/B aid: everything through the 128 x 128 tiles)
    if (!no_wide && M <= 256 && N <= 256 && M >= 128 && N >= 128 && (M > 128 || N > 128)) {
        if (nw < MAX_TN_JOBS) w.j[nw] = TnJob{dY, X, dW, db, ldy, ldx, ldw, M, N};
        ++nw;
        return;
    }
    if (n < MAX_TN_JOBS) b.j[n] = TnJob{dY, X, dW, db, ldy, ldx, ldw, M, N};
    ++n;
    tiles += ((N + GT - 1) / GT) * ((M + GT - 1) / GT);
}
int TnList::launch(long P, const float *zero, int num_cu, hipStream_t st, bool f32)
{
    if (n > MAX_TN_JOBS || nw > MAX_TN_JOBS) return (int)hipErrorOutOfMemory;
    if (f32) return launch_f32(P, zero, num_cu, st);
    static sahs_once::Flags attr_set, attr_set_w;
    hipError_t ae = sahs_once::per_device(attr_set, [&]() {
        return hipFuncSetAttribute(reinterpret_cast<const void *>(gemm_tn_jobs_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, TN_LDS_BYTES);
    });
    if (ae != hipSuccess) return (int)ae;
    ae = sahs_once::per_device(attr_set_w, [&]() {
        return hipFuncSetAttribute(reinterpret_cast<const void *>(gemm_tn_jobs256_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, TW_LDS_BYTES);
    });
    if (ae != hipSuccess) return (int)ae;
    // ranges of >= 1024 samples (a multiple of 16), `rounds` rounds of equal items per workgroup: fewer, longer items mean fewer atomic
    // epilogues (measured on the training step: wide kernel 1.21 / 1.24 / 1.27 / 1.31 ms at 1 / 2 / 3 / 5 rounds; the narrow one is flat)
    static const long rounds_env = sahs_diag_env("SAHS_BWD_TN_ROUNDS") ? atol(sahs_diag_env("SAHS_BWD_TN_ROUNDS")) : 0;      // (tuning aid)
    auto range_for = [&](long workgroups, int units, long rounds) {
        long nsplit = (rounds_env > 0 ? rounds_env : rounds) * workgroups / (units > 0 ? units : 1);
        if (nsplit < 1) nsplit = 1;
        long range = ((P + nsplit - 1) / nsplit + 15) / 16 * 16;
        return range < 1024 ? 1024L : range;
    };
    if (nw > 0) {
        gemm_tn_jobs256_kernel<<<num_cu, TN_THREADS, TW_LDS_BYTES, st>>>(w, nw, P, range_for(num_cu, nw, 1), zero);      // one 128-KB workgroup per CU
        if (hipGetLastError() != hipSuccess) return (int)hipErrorLaunchFailure;
    }
    if (n > 0) {
        const int G = 2 * num_cu / 8 * 8;                     // two 80-KB workgroups per CU
        gemm_tn_jobs_kernel<<<G, TN_THREADS, TN_LDS_BYTES, st>>>(b, n, tiles, P, range_for(G, tiles, 2), zero);
    }
    return (int)hipGetLastError();
}
bool TnList::make_plan(TnPlan &pl, const float *cost, int nunits, long slots, long P)
{
    if (nunits > MAX_TN_UNITS) return false;
    double total = 0.0;
    for (int i = 0; i < nunits; ++i) total += cost[i];
    const long nmax = P / 1024 > 0 ? P / 1024 : 1;
    long n[MAX_TN_UNITS], sum = 0;
    for (int i = 0; i < nunits; ++i) {
        n[i] = (long)(cost[i] / total * (double)slots + 0.5);
        n[i] = n[i] < 1 ? 1 : (n[i] > nmax ? nmax : n[i]);
        sum += n[i];
    }
    while (sum > slots) {      // never one item more than the slots: it would be a whole extra round of the launch (measured: 1.9 -> 3.5 ms)
        int big = 0;
        for (int i = 1; i < nunits; ++i)
            if (n[i] > n[big]) big = i;
        if (n[big] <= 1) break;
        --n[big]; --sum;
    }
    int start = 0;
    for (int i = 0; i < nunits; ++i) {
        if (start + n[i] > 65535) return false;
        pl.u[i].start = (unsigned short)start;
        pl.u[i].n = (unsigned short)n[i];
        start += (int)n[i];
    }
    pl.nunits = nunits;
    pl.items = start;
    return true;
}
int TnList::launch_f32(long P, const float *zero, int num_cu, hipStream_t st)
{
    static sahs_once::Flags attr_set, attr_set_w;
    hipError_t ae = sahs_once::per_device(attr_set, [&]() {
        return hipFuncSetAttribute(reinterpret_cast<const void *>(gemm_tn_jobs_f32_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, TF_LDS_BYTES);
    });
    if (ae != hipSuccess) return (int)ae;
    ae = sahs_once::per_device(attr_set_w, [&]() {
        return hipFuncSetAttribute(reinterpret_cast<const void *>(gemm_tn_jobs256_f32_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, TFW_LDS_BYTES);
    });
    if (ae != hipSuccess) return (int)ae;
    static const float c0w = sahs_diag_env("SAHS_TNF_C0W") ? (float)atof(sahs_diag_env("SAHS_TNF_C0W")) : 0.27f;      // (tuning aids: a K-step's fixed part in the two
    static const float c0n = sahs_diag_env("SAHS_TNF_C0N") ? (float)atof(sahs_diag_env("SAHS_TNF_C0N")) : 0.4f;      //  cost models, items per workgroup of the narrow launch)
    static const long rounds_n = sahs_diag_env("SAHS_TNF_ROUNDS") ? atol(sahs_diag_env("SAHS_TNF_ROUNDS")) : 3;
    if (nw > 0) {      // one 128-KB workgroup per CU, one item each
        TnPlan pl;
        float cost[MAX_TN_UNITS];
        for (int i = 0; i < nw && i < MAX_TN_UNITS; ++i) {
            cost[i] = c0w + (w.j[i].M > 128 ? 2.0f : 1.0f);      // (rows past M are the zero page: the waves that own them skip their MFMAs; 0.27: a K-step's fixed part)
            pl.u[i].job = (unsigned char)i; pl.u[i].bx = pl.u[i].by = pl.u[i].pad = 0;
        }
        if (!make_plan(pl, cost, nw, num_cu, P)) return (int)hipErrorOutOfMemory;
        gemm_tn_jobs256_f32_kernel<<<num_cu, TN_THREADS, TFW_LDS_BYTES, st>>>(w, pl, P, zero);
        if (hipGetLastError() != hipSuccess) return (int)hipErrorLaunchFailure;
    }
    if (n > 0) {       // two 64-KB workgroups per CU, three items each (measured on the training step: 0.91 / 0.69 / 0.64 / 0.64 ms per launch at 1 / 2 / 3 / 4)
        const int G = 2 * num_cu;
        TnPlan pl;
        float cost[MAX_TN_UNITS];
        int nu = 0;
        for (int i = 0; i < n; ++i) {
            const int nx = (b.j[i].N + GT - 1) / GT, ny = (b.j[i].M + GT - 1) / GT;
            for (int by = 0; by < ny; ++by)
                for (int bx = 0; bx < nx; ++bx, ++nu) {
                    if (nu >= MAX_TN_UNITS) return (int)hipErrorOutOfMemory;
                    const int mt = b.j[i].M - by * GT < GT ? b.j[i].M - by * GT : GT, nt = b.j[i].N - bx * GT < GT ? b.j[i].N - bx * GT : GT;
                    // a K-step: its fixed part (barrier, DMA issue, first LDS round trip; fitted on the training step, tools/sweep_tnf.sh: 0.54 / 0.54 /
                    // 0.55 / 0.56 / 0.57 ms per launch at 0.4 / 0.7 / 1.0 / 1.3 / 1.8) + the tile's valid accumulators
                    cost[nu] = c0n + (float)(((mt + 15) / 16) * ((nt + 15) / 16)) / 64.0f;
                    pl.u[nu].job = (unsigned char)i; pl.u[nu].bx = (unsigned char)bx; pl.u[nu].by = (unsigned char)by; pl.u[nu].pad = 0;
                }
        }
        if (!make_plan(pl, cost, nu, rounds_n * G, P)) return (int)hipErrorOutOfMemory;
        gemm_tn_jobs_f32_kernel<<<G, TN_THREADS, TF_LDS_BYTES, st>>>(b, pl, P, zero);
    }
    return (int)hipGetLastError();
}

}  // namespace sahs
