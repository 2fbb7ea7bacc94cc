// field_bwd_gemm.hip -- the per-layer walk's kernels that depend on no model layout, built once (field_bwd_gemm.hpp has their launchers):
// three generations of dense fp32-in GEMM (register-staged gemm_f32_kernel, LDS-DMA gemm_dma_kernel, split-once weight gradient
// gemm_tn_split_kernel), and the copy / axpy / constant-column helpers of both walks.  For every dense layer
// dW += dY^T X (+ db = column sums of dY, fused),   dX = (dY W) * act'(X);  which layers there are is the business of field_bwd.hip.
// Since the fused walk reached every model the GEMMs here serve as the tests' A/B reference and behind ops.fused_backward(False); the fused
// walk's job-table weight-gradient kernels are in field_bwd_tn_jobs.hip, what the two files share in bwd_gemm_tile.hpp.  This file is not
// compiled on its own: field_bwd_tn_jobs.hip includes it (one translation unit, see there).
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "sahs_common.hpp"
#include "field_bwd_gemm.hpp"
#include "bwd_gemm_tile.hpp"
#if SAHS_MODEL != 0
#error "field_bwd_gemm.hip is model-independent: built once, without -DSAHS_MODEL"
#endif

namespace sahs {

// ------------------------------------------------------------------------------------------------
// C[M x N] (op)= A'[M x K] B[K x N], fp32, v_mfma_f32_16x16x4_f32.  TA: A'(m,k) = A[k*lda + m], else A[m*lda + k];
// B(k,n) = B[k*ldb + n].  64x64 tile per 256-thread workgroup, K in steps of 16 through LDS; blockIdx.z splits K.
// mode 0: C = acc; 1: C += acc; 2: atomicAdd(C, acc).  mask != null: acc *= (mask[m*ldm + n] > 0 ? 1 : slope).
// ------------------------------------------------------------------------------------------------
constexpr int GLD = 132;   // 128x128 tile (GT), K-step 16 (GK); LDS row stride 132 floats

// Global -> register staging of one K-step of both operands (8 floats per thread per operand), so that the loads of step
// k+1 are in flight while step k is multiplied (the LDS tiles are double buffered).
struct Stage { float a[8], b[8]; };

template <bool TA>
__device__ __forceinline__ void stage_load(Stage &st, int tid, long m0, int n0, long k0, long k_hi, int M, int N, const float *__restrict__ A,
                                           long lda, const float *__restrict__ B, long ldb, bool va, bool vb)
{
    // A' tile element (kk, mm): thread covers 8 consecutive elements along the contiguous global direction
    if (TA) {   // A'(m,k) = A[k*lda + m]: contiguous in m.  16 k-rows x 128 m: thread -> row kk = tid/16, mm = (tid%16)*8
        const int kk = tid >> 4, mm = (tid & 15) * 8;
        const long k = k0 + kk, m = m0 + mm;
        if (va && k < k_hi && m + 7 < M) {
            const f32x4 v0 = *reinterpret_cast<const f32x4 *>(A + k * lda + m), v1 = *reinterpret_cast<const f32x4 *>(A + k * lda + m + 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) { st.a[i] = v0[i]; st.a[4 + i] = v1[i]; }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) st.a[i] = (k < k_hi && m + i < M) ? A[k * lda + m + i] : 0.0f;
        }
    } else {    // A'(m,k) = A[m*lda + k]: contiguous in k.  128 m-rows x 16 k: thread -> mm = tid/2, kk = (tid%2)*8
        const int mm = tid >> 1, kk = (tid & 1) * 8;
        const long m = m0 + mm, k = k0 + kk;
        if (va && m < M && k + 7 < k_hi) {
            const f32x4 v0 = *reinterpret_cast<const f32x4 *>(A + m * lda + k), v1 = *reinterpret_cast<const f32x4 *>(A + m * lda + k + 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) { st.a[i] = v0[i]; st.a[4 + i] = v1[i]; }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) st.a[i] = (m < M && k + i < k_hi) ? A[m * lda + k + i] : 0.0f;
        }
    }
    {           // B(k,n) = B[k*ldb + n]: contiguous in n.  16 k-rows x 128 n
        const int kk = tid >> 4, nn = (tid & 15) * 8;
        const long k = k0 + kk;
        const int n = n0 + nn;
        if (vb && k < k_hi && n + 7 < N) {
            const f32x4 v0 = *reinterpret_cast<const f32x4 *>(B + k * ldb + n), v1 = *reinterpret_cast<const f32x4 *>(B + k * ldb + n + 4);
#pragma unroll
            for (int i = 0; i < 4; ++i) { st.b[i] = v0[i]; st.b[4 + i] = v1[i]; }
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) st.b[i] = (k < k_hi && n + i < N) ? B[k * ldb + n + i] : 0.0f;
        }
    }
}

template <bool TA>
__device__ __forceinline__ void stage_store(const Stage &st, int tid, float (*As)[GLD], float (*Bs)[GLD])
{
    if (TA) {
        const int kk = tid >> 4, mm = (tid & 15) * 8;
#pragma unroll
        for (int i = 0; i < 8; ++i) As[kk][mm + i] = st.a[i];
    } else {
        const int mm = tid >> 1, kk = (tid & 1) * 8;
#pragma unroll
        for (int i = 0; i < 8; ++i) As[kk + i][mm] = st.a[i];
    }
    const int kk = tid >> 4, nn = (tid & 15) * 8;
#pragma unroll
    for (int i = 0; i < 8; ++i) Bs[kk][nn + i] = st.b[i];
}

// TA && rowsum != null: the n-block-0 workgroups also accumulate rowsum[m] += sum_k A'(m,k) (the bias gradient of the layer whose
// weight gradient this GEMM is) from the A tiles they stage anyway.
// nbn > 0 (1-D grid): XCD-aware mapping -- the nbn column blocks of one row block run on the same XCD (consecutive slots of
// workgroup ids congruent mod 8), so the second one finds the shared A tile in that XCD's L2.
template <bool TA>
__global__ void __launch_bounds__(256) gemm_f32_kernel(int M, int N, int K, const float *__restrict__ A, long lda,
                                                       const float *__restrict__ B, long ldb, float *__restrict__ C, long ldc, int mode,
                                                       const float *__restrict__ mask, long ldm, float slope, int kslab,
                                                       float *__restrict__ rowsum, int nbn)
{
    __shared__ float As[2][GK][GLD], Bs[2][GK][GLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, c16 = lane & 15;
    const int wm = wave >> 1, wn = wave & 1;              // each wave: 64 x 64 = 4 x 4 MFMA tiles
    int bx = blockIdx.x, by = blockIdx.y;
    if (nbn > 0) {
        const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
        bx = slot % nbn;
        by = (slot / nbn) * 8 + xcd;
        if ((long)by * GT >= M) return;
    }
    const long m0 = (long)by * GT;
    const int n0 = bx * GT;
    const long k_lo = (long)blockIdx.z * kslab;
    const bool do_sum = TA && rowsum != nullptr && bx == 0;
    float cs[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    const long k_hi = (k_lo + kslab < K) ? k_lo + kslab : K;
    // 16-byte vector loads only when every row start is 16-byte aligned
    const bool va = ((reinterpret_cast<uintptr_t>(A) & 15) == 0) && (lda % 4 == 0);
    const bool vb = ((reinterpret_cast<uintptr_t>(B) & 15) == 0) && (ldb % 4 == 0);
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    Stage st;
    stage_load<TA>(st, tid, m0, n0, k_lo, k_hi, M, N, A, lda, B, ldb, va, vb);
    stage_store<TA>(st, tid, As[0], Bs[0]);
    if (do_sum)
#pragma unroll
        for (int i = 0; i < 8; ++i) cs[i] += st.a[i];
    __syncthreads();
    int cur = 0;
    for (long k0 = k_lo; k0 < k_hi; k0 += GK) {
        const bool more = k0 + GK < k_hi;
        if (more) {
            stage_load<TA>(st, tid, m0, n0, k0 + GK, k_hi, M, N, A, lda, B, ldb, va, vb);
            if (do_sum)
#pragma unroll
                for (int i = 0; i < 8; ++i) cs[i] += st.a[i];
        }
#pragma unroll
        for (int s = 0; s < GK / 4; ++s) {
            float a[4], b[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = As[cur][4 * s + q][64 * wm + 16 * i + c16];
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = Bs[cur][4 * s + q][64 * wn + 16 * j + c16];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (more) stage_store<TA>(st, tid, As[cur ^ 1], Bs[cur ^ 1]);
        __syncthreads();
        cur ^= 1;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long m = m0 + 64 * wm + 16 * i + 4 * q + r;
                const int n = n0 + 64 * wn + 16 * j + c16;
                if (m < M && n < N) {
                    float v = acc[i][j][r];
                    if (mask != nullptr) v *= (mask[m * ldm + n] > 0.0f) ? 1.0f : slope;
                    float *dst = C + m * ldc + n;
                    if (mode == 0) *dst = v;
                    else if (mode == 1) *dst += v;
                    else atomicAdd(dst, v);
                }
            }
    if (do_sum) {   // the K loop ended on a barrier: the LDS tiles are free.  Thread (kk, mm) holds the sums of its 8 m over k = kk mod 16.
        const int kk = tid >> 4, mm = (tid & 15) * 8;
#pragma unroll
        for (int i = 0; i < 8; ++i) As[0][kk][mm + i] = cs[i];
        __syncthreads();
        if (tid < GT && m0 + tid < M) {
            float t = 0.0f;
#pragma unroll
            for (int k = 0; k < GK; ++k) t += As[0][k][tid];
            atomicAdd(rowsum + m0 + tid, t);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// The same two GEMMs with the operand tiles moved global -> LDS by LDS-DMA (global_load_lds, 16 B per lane, no VGPR
// staging, no ds_write), three K-steps deep: while step t is multiplied, steps t+1 and t+2 are in flight.  One raw
// s_barrier per K-step; the wait before it is a counted vmcnt (4 = the wave's DMA instructions of the one newer step).
// Needs 16-byte aligned operand rows (A, B, lda, ldb multiples of 4 floats) -- the host routes everything else to
// gemm_f32_kernel above.  Out-of-range rows/columns are fetched from a 16-byte zero page.
//   TA : A'(m,k) = A[k*lda + m]  tile [16 k][128 m]          B(k,n) = B[k*ldb + n]  tile [16 k][128 n]
//   !TA: A'(m,k) = A[m*lda + k]  tile [128 m][16 k] (one ds_read_b128 = 4 k of one row; the MFMA k index is
//        permuted -- lane q takes k = 4q + r at MFMA r -- identically for both operands, so the sum is unchanged)
// K-major tiles are XOR-swizzled by 16 floats on alternate rows (TA: k&1, !TA: (k>>2)&1 -- either way q&1 on the MFMA
// side), so the four q groups of a ds_read_b32 hit two disjoint bank sets (the fetch plan: head of bwd_gemm_tile.hpp).
// ------------------------------------------------------------------------------------------------
// X3 (data gradient only): the products on the bf16 matrix pipe at near-fp32 accuracy (the operand split of field_bf16x3.hip): every fp32
// value of A is split on its way from LDS to the MFMA into x = hi + lo (hi = bf16(x), lo = bf16(x - hi): 16-17 significant bits together),
// B arrives pre-split, and a product is three v_mfma_f32_32x32x16_bf16 with fp32 accumulation, a b ~= a_hi b_hi + a_hi b_lo + a_lo b_hi
// (the dropped a_lo b_lo term is ~2^-18 of the product).  One 16-feature K-step of the LDS ring is exactly one MFMA k-depth; a wave's
// 64 x 64 block is 2 x 2 tiles of 32 x 32, 12 MFMAs per K-step (384 matrix-pipe cycles against the 2048 of the 64 f32 MFMAs it replaces),
// so the GEMM turns from matrix-bound into HBM-bound.  Same tiles, ring, epilogues and arguments as the f32 form (X3 = false), which stays
// selectable (SAHS_BWD_GEMM=f32) as the exact A/B reference.
// ring depth: 3 for the data-gradient GEMM (48 KB of LDS, three workgroups per CU, 16-step K loops), 4 for the weight-gradient GEMM (64 KB,
// two workgroups per CU by its registers anyway, K loops of 32..512 steps: three K-steps = 48 KB per workgroup in flight -- the
// kernel is HBM-bound and at depth 3 it reached 3.7 TB/s with 64 KB per CU in flight)
template <bool TA> constexpr int ring_depth() { return TA ? 4 : 3; }

// (waves per SIMD: 3 is asked of every form; the f32 weight-gradient form <true, false> gets 2, by its 64 KB of LDS, and the compiler says so.
// Asking 2 of it is not the same kernel: the accumulators leave the AGPRs, 2829 -> 2653 instructions -- so the 3 and the warning stay)
template <bool TA, bool X3>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) gemm_dma_kernel(int M, int N, int K, const float *__restrict__ A, long lda,
                                                       const float *__restrict__ B, long ldb, float *__restrict__ C, long ldc, int mode,
                                                       const float *__restrict__ mask, long ldm, float slope, int kslab,
                                                       float *__restrict__ rowsum, int nbn, const float *__restrict__ zero,
                                                       unsigned char *__restrict__ bits)
{
    // the split-bf16 weight gradient is gemm_tn_split_kernel (below): it splits each operand value once per workgroup, not once per wave
    static_assert(!(TA && X3), "gemm_dma_kernel<true, true> does not exist: gemm_tn sends the split-bf16 weight gradient to gemm_tn_split_kernel");
    // bits (optional): the sign bits of an activation matrix (format: emit_sign_bits, bwd_gemm_tile.hpp).  The weight-gradient GEMM (TA) WRITES
    // them for its B operand X; the data-gradient GEMM of the same layer, whose (leaky-)ReLU mask is that same X, READS them instead of the fp32 matrix.
    constexpr int DST = ring_depth<TA>();
    __shared__ __attribute__((aligned(16))) float smem[DST][2][DTILE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, c16 = lane & 15;
    const int wm = wave >> 1, wn = wave & 1;
    int bx = blockIdx.x, by = blockIdx.y;
    long bz = blockIdx.z;
    if (nbn > 0) {
        const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
        bx = slot % nbn;
        by = (slot / nbn) * 8 + xcd;
        if ((long)by * GT >= M) return;
    } else if (nbn < 0) {
        // weight-gradient GEMM, 1-D grid: the nx x ny output tiles of ONE sample slab read the same dY and X rows -- they run on the same
        // XCD (workgroup ids congruent mod 8, consecutive slots), so that XCD's L2 fetches the slab from HBM once instead of once per tile
        const int nx = -nbn, ny = (M + GT - 1) / GT, tiles = nx * ny;
        const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
        const int tile = slot % tiles;
        bz = (long)(slot / tiles) * 8 + xcd;
        bx = tile % nx;
        by = tile / nx;
        if (bz * kslab >= K) return;
    }
    const long m0 = (long)by * GT;
    const int n0 = bx * GT;
    const long k_lo = bz * kslab;
    const long k_hi = (k_lo + kslab < K) ? k_lo + kslab : K;
    const int T = (int)((k_hi - k_lo + GK - 1) / GK);
    const bool do_sum = TA && rowsum != nullptr && bx == 0;

    // ---- this wave's four DMA instructions per K-step: waves 0,1 move the A tile, waves 2,3 the B tile ----
    // (own copy of the fetch plan, bwd_gemm_tile.hpp, indexed issue; beside its K-major arm it has two operand forms that are not K-major)
    const int h = lane >> 5, c32 = lane & 31;
    const float *src[4]; long step[4]; int krow[4]; bool colok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int rp = (wave & 1) * 4 + u;                 // 0..7: which 1-KB eighth of the tile
        if (X3 && wave >= 2) {                               // B = pre-split, fragment-ordered weight pieces: a linear 8 KB copy per K-step
            src[u] = B + ((k_lo / GK) * (long)nbn + bx) * (GK * GT) + (rp * 64 + lane) * 4;
            step[u] = (long)nbn * (GK * GT);
            krow[u] = 0;
            colok[u] = true;
        } else if (wave < 2 && !TA) {                        // A, row-major [128 m][16 k]: 4 chunks per row
            const int chunk = rp * 64 + lane, m = chunk >> 2, kc = chunk & 3;
            src[u] = A + (m0 + m) * lda + k_lo + 4 * kc;
            step[u] = GK;
            krow[u] = 4 * kc;                                // valid while k0 + krow < k_hi
            colok[u] = m0 + m < M;
        } else {                                             // K-major [16 k][128 cols], 32 chunks per row, two rows per instruction
            const float *base = (wave < 2) ? A : B;
            const long ld = (wave < 2) ? lda : ldb;
            const long c0 = (wave < 2) ? m0 : n0;
            const int dim = (wave < 2) ? M : N;
            const int row = 2 * rp + h;
            const int sw = TA ? (row & 1) : ((row >> 2) & 1);
            const int j = c32 ^ (sw << 2);
            src[u] = base + (k_lo + row) * ld + c0 + 4 * j;
            step[u] = GK * ld;
            krow[u] = row;
            colok[u] = c0 + 4 * j < dim;
        }
    }
    const int dst_off = ((wave < 2) ? 0 : DTILE) + (wave & 1) * 4 * 256;   // + u*256 floats, + lane*4 by the hardware
    auto issue = [&](int t) {
        float *dstb = &smem[t % DST][0][0] + dst_off;
        const long k0 = k_lo + (long)t * GK;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float *g = (colok[u] && k0 + krow[u] < k_hi) ? src[u] + (long)t * step[u] : zero;
            __builtin_amdgcn_global_load_lds((gbl_void_t)g, (lds_void_t)(dstb + u * 256), 16, 0, 0);
        }
    };

    // ---- MFMA-side LDS offsets ----
    int colA[4], colB[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = 64 * wm + 16 * i + c16, n = 64 * wn + 16 * i + c16;
        colA[i] = TA ? ((((m >> 2) ^ ((q & 1) << 2)) << 2) + (m & 3)) : (m * GK + 4 * q);
        colB[i] = (((n >> 2) ^ ((q & 1) << 2)) << 2) + (n & 3);
    }
    // X3: lane (r32, h) of a 32x32x16 MFMA supplies k = 8h .. 8h+7 of row r32 of a 32-wide tile: 32 contiguous bytes of row m of the row-major A
    const int r32 = lane & 31;
    int x3a[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) x3a[t] = (64 * wm + 32 * t + r32) * GK + 8 * h;
    f32x4 acc[4][4];
    f32x16_t acx[2][2];
    if constexpr (X3) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acx[i][j][e] = 0.0f;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    float cs = 0.0f;

    // vmcnt accounting of the K loop (audited on the ISA, tools/check_isa.py; the build fails if this kernel gets scratch): the only
    // vector-memory instructions a wave executes between kernel entry and the end of the loop are its 4 LDS-DMA instructions per
    // issue(); they complete in issue order, so "vmcnt(4)" at step t means step t has landed while step t+1 may still be in flight --
    // and any further VMEM instruction the compiler might ever add there could only make that wait stricter, never weaker.
    // (depth DST: steps t+1 .. t+DST-2 may be in flight at step t's wait -- 4 DMA instructions each -- and step t+DST-1 is issued after it)
    // data-gradient GEMM: this lane's 16 mask bytes of the epilogue (row (tid >> 5) + 8 e, columns n0 + 4 (tid & 31) ..) are requested
    // here, ahead of the K loop -- they are older than every LDS-DMA, so the counted waits below stay correct (stricter) -- and have long
    // landed when the epilogue packs them; fetched after the loop they cost every workgroup an exposed memory round trip
    unsigned char pre_raw[16];
    if constexpr (!TA) {
        const bool pre_bits = mode != 2 && mask != nullptr && bits != nullptr;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const long m = m0 + (tid >> 5) + 8 * e;
            const int en = n0 + 4 * (tid & 31);
            pre_raw[e] = pre_bits ? bits[(m < M && en < N) ? m * (N >> 3) + (en >> 3) : 0] : (unsigned char)0;
        }
    }
    if (T > 0) issue(0);      // an empty K slab (k_lo >= K) issues nothing and falls through to a zero contribution
    if (T > 1) issue(1);
    if (DST > 3 && T > 2) issue(2);
    for (int t = 0; t < T; ++t) {
        if (DST > 3 && t + 2 < T) asm volatile("s_waitcnt vmcnt(8)\n\ts_barrier" ::: "memory");
        else if (t + 1 < T) asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        if (t + DST - 1 < T) issue(t + DST - 1);          // into the buffer every wave finished reading before the barrier above
        const float *As = &smem[t % DST][0][0], *Bs = &smem[t % DST][1][0];
        if constexpr (TA) {
            // (own copy of emit_sign_bits, bwd_gemm_tile.hpp: calling it costs this kernel's <true, false> form one s_nop of its schedule)
            if (bits != nullptr && by == 0) {      // thread (kk, g): the 8 columns 8g .. 8g+7 of sample row kk of the X tile -> one byte
                const int kk = tid >> 4, g = tid & 15;
                const long k = k_lo + (long)t * GK + kk;
                if (k < k_hi && n0 + 8 * g < N) {
                    const float *px = Bs + kk * GT + 4 * ((2 * g) ^ ((kk & 1) << 2));     // chunks 2g, 2g+1 stay adjacent under the swizzle
                    const f32x4 v0 = *reinterpret_cast<const f32x4 *>(px), v1 = *reinterpret_cast<const f32x4 *>(px + 4);
                    unsigned b8 = 0;
#pragma unroll
                    for (int i = 0; i < 4; ++i) b8 |= (v0[i] > 0.0f ? 1u : 0u) << i | (v1[i] > 0.0f ? 1u : 0u) << (4 + i);
                    bits[k * (N >> 3) + (n0 >> 3) + g] = (unsigned char)b8;
                }
            }
        }
        if constexpr (X3) {
            u32x4_t ah[2], al[2], bh[2], bl[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                float x[8];
                const f32x4 v0 = *reinterpret_cast<const f32x4 *>(As + x3a[i]), v1 = *reinterpret_cast<const f32x4 *>(As + x3a[i] + 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) { x[j] = v0[j]; x[4 + j] = v1[j]; }
                split8(x, ah[i], al[i]);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {      // weights arrive split and in fragment order (CopyJob pack): n-tile 2 wn + i, hi then lo
                bh[i] = *reinterpret_cast<const u32x4_t *>(Bs + ((2 * wn + i) * 64 + lane) * 4);
                bl[i] = *reinterpret_cast<const u32x4_t *>(Bs + GK * GT / 2 + ((2 * wn + i) * 64 + lane) * 4);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acx[i][j] = mfma3(ah[i], al[i], bh[j], bl[j], acx[i][j]);
        } else if constexpr (TA) {
#pragma unroll
            for (int s4 = 0; s4 < GK / 4; ++s4) {
                float a[4], b[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) a[i] = As[(4 * s4 + q) * GT + colA[i]];
#pragma unroll
                for (int j = 0; j < 4; ++j) b[j] = Bs[(4 * s4 + q) * GT + colB[j]];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
            }
            if (do_sum && tid < GT) {
#pragma unroll
                for (int k = 0; k < GK; ++k) cs += As[k * GT + ((((tid >> 2) ^ ((k & 1) << 2)) << 2) + (tid & 3))];
            }
        } else {
            f32x4 av[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) av[i] = *reinterpret_cast<const f32x4 *>(As + colA[i]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float b[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) b[j] = Bs[(4 * q + r) * GT + colB[j]];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i][r], b[j], acc[i][j], 0, 0, 0);
            }
        }
    }
    // one accessor for both accumulator layouts: value of row `row` (0..63 of this wave's block, as enumerated below) x column
    // f32 form: tile (i, j) register r  -> row 16 i + 4 q + r,                       column 16 j + c16
    // X3 form : tile (i, j) register e  -> row 32 i + (e & 3) + 8 (e >> 2) + 4 h,    column 32 j + r32
    constexpr int NI = X3 ? 2 : 4, NR = X3 ? 16 : 4;
    auto row_of = [&](int i, int e) { return X3 ? 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h : 16 * i + 4 * q + e; };
    auto col_of = [&](int j) { return X3 ? 32 * j + r32 : 16 * j + c16; };
    auto val_of = [&](int i, int j, int e) -> float { if constexpr (X3) return acx[i][j][e]; else return acc[i][j][e]; };
    constexpr int SLD = GT + 4;                 // staging rows of the two LDS epilogues: 64 x 132 floats = 33 KB of the ring, free after the K loop
    if constexpr (!TA) {
    if (mode != 2 && ((reinterpret_cast<uintptr_t>(C) | (mask ? reinterpret_cast<uintptr_t>(mask) : 0)) & 15) == 0 && ldc % 4 == 0 &&
        (mask == nullptr || ldm % 4 == 0)) {
        // Data-gradient epilogue through LDS: the accumulator layout gives 64-byte row segments per store instruction (64 mask loads
        // + 64 stores per lane); staged, every thread moves whole float4s of 512-byte rows (8 stores per lane per half).
        // Everything the stores need from memory -- the mask (as sign bits or as the fp32 activation) and, for mode 1, the old value -- is
        // fetched by ONE batch of loads per half through clamped addresses (no per-lane branches), ahead of the staging barrier; the
        // stores then follow each other with no wait between them.  (Round 3, from the cycle stamps of tools/stamp_gemm.py: with a load
        // inside each store's guard the compiler put `s_waitcnt vmcnt(0)` -- which on gfx9 also waits for every earlier STORE -- in front of
        // all 16 stores of a lane: a serial chain of 16 memory round trips, 60 % of this kernel's wave time.)
        float *stage = &smem[0][0][0];
        const bool by_bits = mask != nullptr && bits != nullptr, by_mask = mask != nullptr && bits == nullptr, whole4 = (N & 3) == 0;
        const int erow = tid >> 5, en = n0 + 4 * (tid & 31);
        unsigned nibs[2] = {0u, 0u};                        // this lane's 16 mask nibbles (row erow + 8 e, columns en .. en+3), 4 bits each
        if (by_bits) {
#pragma unroll
            for (int e = 0; e < 16; ++e) nibs[e >> 3] |= (((unsigned)pre_raw[e] >> (en & 4)) & 15u) << (4 * (e & 7));
        }
        lds_barrier();
#pragma unroll
        for (int half = 0; half < 2; ++half) {
#pragma unroll
            for (int grp = 0; grp < 2; ++grp) {             // the rarer fp32-mask / accumulate forms fetch in two batches of four per half
                f32x4 mk[4], od[4];
                if (whole4 && by_mask) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const long m = m0 + 64 * half + erow + 8 * (4 * grp + e);
                        mk[e] = *reinterpret_cast<const f32x4 *>(mask + ((m < M && en < N) ? m * ldm + en : 0));
                    }
                }
                if (whole4 && mode == 1) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const long m = m0 + 64 * half + erow + 8 * (4 * grp + e);
                        od[e] = *reinterpret_cast<const f32x4 *>(C + ((m < M && en < N) ? m * ldc + en : 0));
                    }
                }
                if (grp == 0) {
                    if (wm == half) {
#pragma unroll
                        for (int i = 0; i < NI; ++i)
#pragma unroll
                            for (int j = 0; j < NI; ++j)
#pragma unroll
                                for (int r = 0; r < NR; ++r) stage[row_of(i, r) * SLD + 64 * wn + col_of(j)] = val_of(i, j, r);
                    }
                    lds_barrier();
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int row = erow + 8 * (4 * grp + e);
                    const long m = m0 + 64 * half + row;
                    const unsigned nb = nibs[half] >> (4 * (4 * grp + e));
                    f32x4 v = *reinterpret_cast<const f32x4 *>(stage + row * SLD + 4 * (tid & 31));
                    if (whole4) {
                        if (by_bits) {
#pragma unroll
                            for (int k = 0; k < 4; ++k) v[k] *= ((nb >> k) & 1u) ? 1.0f : slope;
                        } else if (by_mask) {
#pragma unroll
                            for (int k = 0; k < 4; ++k) v[k] *= (mk[e][k] > 0.0f) ? 1.0f : slope;
                        }
                        if (mode == 1) { v[0] += od[e][0]; v[1] += od[e][1]; v[2] += od[e][2]; v[3] += od[e][3]; }
                        if (m < M && en < N) *reinterpret_cast<f32x4 *>(C + m * ldc + en) = v;
                    } else if (m < M && en < N) {            // ragged N (the encodings' gradients): element-wise, rare and small
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            if (en + k < N) {
                                float x = v[k];
                                if (by_bits) x *= ((nb >> k) & 1u) ? 1.0f : slope;
                                else if (by_mask) x *= (mask[m * ldm + en + k] > 0.0f) ? 1.0f : slope;
                                float *dst = C + m * ldc + en + k;
                                *dst = (mode == 1) ? *dst + x : x;
                            }
                        }
                    }
                }
            }
            lds_barrier();
        }
        return;
    }
    }
    if constexpr (TA) {
    if (mode == 2) {
        // Weight-gradient epilogue through LDS as well: one atomic instruction then covers 256 contiguous bytes of a dW row
        // instead of four 64-byte segments of four rows.  (own copy of the staged atomic epilogue: see tn_tile)
        float *stage = &smem[0][0][0];
        __syncthreads();
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            if (wm == half) {
#pragma unroll
                for (int i = 0; i < NI; ++i)
#pragma unroll
                    for (int j = 0; j < NI; ++j)
#pragma unroll
                        for (int r = 0; r < NR; ++r) stage[row_of(i, r) * SLD + 64 * wn + col_of(j)] = val_of(i, j, r);
            }
            __syncthreads();
#pragma unroll 4
            for (int e = 0; e < 32; ++e) {
                const int idx = tid + 256 * e, row = idx >> 7, col = idx & 127;
                const long m = m0 + 64 * half + row;
                const int n = n0 + col;
                if (m < M && n < N && ldc > 0) atomicAdd(C + m * ldc + n, stage[row * SLD + col]);
            }
            __syncthreads();
        }
        if (do_sum && tid < GT && m0 + tid < M) atomicAdd(rowsum + m0 + tid, cs);
        return;
    }
    }
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j)
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const long m = m0 + 64 * wm + row_of(i, r);
                const int n = n0 + 64 * wn + col_of(j);
                if (m < M && n < N) {
                    float v = val_of(i, j, r);
                    if (mask != nullptr) v *= (mask[m * ldm + n] > 0.0f) ? 1.0f : slope;
                    float *dst = C + m * ldc + n;
                    if (mode == 0) *dst = v;
                    else if (mode == 1) *dst += v;
                    else atomicAdd(dst, v);
                }
            }
    if (do_sum && tid < GT && m0 + tid < M) atomicAdd(rowsum + m0 + tid, cs);
}

// ------------------------------------------------------------------------------------------------
// The weight-gradient GEMM on the bf16 pipe, operands split ONCE per workgroup (round 3): one 128 x 128 tile over one sample slab per
// workgroup, the tile body tn_tile of bwd_gemm_tile.hpp (which the fused walk's gemm_tn_jobs_kernel shares).
__global__ void __launch_bounds__(TN_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) gemm_tn_split_kernel(int M, int N, int K, const float *__restrict__ A, long lda,
                                                       const float *__restrict__ B, long ldb, float *__restrict__ C, long ldc, int kslab,
                                                       float *__restrict__ rowsum, int nx, const float *__restrict__ zero,
                                                       unsigned char *__restrict__ bits)
{
    extern __shared__ __attribute__((aligned(16))) float tn_lds[];
    // 1-D grid: the nx x ny output tiles of ONE sample slab read the same dY and X rows -- they run on the same XCD (workgroup ids congruent
    // mod 8, consecutive slots), so that XCD's L2 fetches the slab from HBM once instead of once per tile
    const int ny = (M + GT - 1) / GT, tiles = nx * ny;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, tile = slot % tiles;
    const long bz = (long)(slot / tiles) * 8 + xcd;
    if (bz * kslab >= K) return;
    const long k_lo = bz * kslab;
    const long k_hi = (k_lo + kslab < K) ? k_lo + kslab : K;
    tn_tile(tn_lds, M, N, A, lda, B, ldb, C, ldc, k_lo, k_hi, rowsum, tile % nx, tile / nx, zero, bits);
}

// dst[m*ldd + n] (op)= src[m*lds + n] for n < N   (mode 0 copy, 1 add)
__global__ void copy2d_kernel(long M, int N, const float *__restrict__ src, long lds_, float *__restrict__ dst, long ldd, int mode)
{
    const long total = M * N;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long m = e / N; const int n = (int)(e % N);
        const float v = src[m * lds_ + n];
        if (mode) dst[m * ldd + n] += v; else dst[m * ldd + n] = v;
    }
}

__global__ void __launch_bounds__(256) copy2d_batch_kernel(CopyBatch b, int phase)      // phase 0: the plain copies, 1: the pack jobs
{                                                                                        // (a pack job may read what a plain copy wrote)
    const CopyJob &j = b.j[blockIdx.y];
    if ((j.pack != 0) != (phase != 0)) return;
    if (j.pack) {
        const int nblk = (j.N + GT - 1) / GT;
        const long total = (long)(j.K / 2) * nblk * GT;        // one thread per (row pair, padded column)
        uint32_t *dst = reinterpret_cast<uint32_t *>(j.dst);
        for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
            const int n = (int)(e % (nblk * GT));
            const int k = 2 * (int)(e / (nblk * GT));
            const float x0 = n < j.N ? j.src[(long)k * j.lds_ + n] : 0.0f, x1 = n < j.N ? j.src[(long)(k + 1) * j.lds_ + n] : 0.0f;
            const uint32_t hi = __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2_t{x0, x1}, bf16x2_t));
            const uint32_t lo = __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2_t{x0 - __builtin_bit_cast(float, hi << 16),
                                                                                                 x1 - __builtin_bit_cast(float, hi & 0xffff0000u)}, bf16x2_t));
            const int step = k >> 4, kk = k & 15, h = kk >> 3, jp = (kk & 7) >> 1, cb = n >> 7, t = (n & 127) >> 5, r = n & 31;
            uint32_t *piece = dst + ((long)step * nblk + cb) * (GK * GT);       // 2048 dwords = 8 KB
            const int at = (t * 64 + h * 32 + r) * 4 + jp;                      // dword within the hi (or lo) half
            piece[at] = hi;
            piece[GK * GT / 2 + at] = lo;
        }
        return;
    }
    const long total = (long)j.K * j.N;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const long m = e / j.N; const int n = (int)(e % j.N);
        j.dst[m * j.ldd + n] = j.src[m * j.lds_ + n];
    }
}

// per-frame constants: dW[r][col0 + k] += db[r] * c[k];  dc[k] += sum_r W[r][col0 + k] * db[r].
// one workgroup per job: thread (g, k) walks rows g, g + ngroups, ... of column k -- the reads of W and the atomics into dW are contiguous
// along k (a block per column made them 256 strided accesses each), dc[k] is reduced over the row groups through LDS
__global__ void __launch_bounds__(256) const_cols_batch_kernel(ConstBatch b)
{
    const ConstJob &j = b.j[blockIdx.x];
    __shared__ float part[256];
    const int cols = j.cols, ngroups = 256 / cols, g = threadIdx.x / cols, k = threadIdx.x - g * cols;
    float s = 0.0f;
    if (g < ngroups) {
        const float ck = j.c[k];
        for (int r = g; r < j.rows; r += ngroups) {
            const float gr = j.db[r];
            s += j.W[(long)r * j.ld + j.col0 + k] * gr;
            atomicAdd(j.dW + (long)r * j.ld + j.col0 + k, gr * ck);
        }
    }
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x < cols) {
        float t = 0.0f;
        for (int q = 0; q < ngroups; ++q) t += part[q * cols + threadIdx.x];
        atomicAdd(j.dc + threadIdx.x, t);      // several jobs share a dc (d driving, d pose)
    }
}

__global__ void __launch_bounds__(256) axpy_batch_kernel(AxpyBatch b)
{
    const AxpyJob &j = b.j[blockIdx.y];
    for (int i = threadIdx.x; i < j.n; i += blockDim.x) atomicAdd(j.y + i, j.x[i]);
}

__global__ void add_rows8_kernel(long n, const float *__restrict__ a, float *__restrict__ y)      // y[i] += a[i] over (P,8) rows, as float4s
{
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        f32x4 v = reinterpret_cast<f32x4 *>(y)[i];
        const f32x4 u = reinterpret_cast<const f32x4 *>(a)[i];
        v[0] += u[0]; v[1] += u[1]; v[2] += u[2]; v[3] += u[3];
        reinterpret_cast<f32x4 *>(y)[i] = v;
    }
}

// ---- launchers of the per-layer walk's GEMMs and of the small kernels (field_bwd_gemm.hpp) ----
bool gemm_aligned(const void *p, long ld)
{
    static const bool nodma = sahs_diag_env("SAHS_BWD_NODMA") != nullptr;     // diagnostic: route every GEMM to the register-staged kernel
    return !nodma && (reinterpret_cast<uintptr_t>(p) & 15) == 0 && ld % 4 == 0;
}

void gemm_nn(hipStream_t st, bool x3, long P, const float *dY, long ldy, int K, const float *W, long ldw, int N, float *dX, long ldx, int mode,
             const float *mask, long ldm, float slope, const float *zero, unsigned char *bits)
{
    const int nbn = (N + GT - 1) / GT;
    const long nbm = (P + GT - 1) / GT;
    dim3 g((unsigned)(((nbm + 7) / 8) * 8 * nbn), 1, 1);
    if (K % GK == 0 && gemm_aligned(dY, ldy)) {
        if (x3) gemm_dma_kernel<false, true><<<g, 256, 0, st>>>((int)P, N, K, dY, ldy, W, ldw, dX, ldx, mode, mask, ldm, slope, K, nullptr, nbn, zero, bits);
        else gemm_dma_kernel<false, false><<<g, 256, 0, st>>>((int)P, N, K, dY, ldy, W, ldw, dX, ldx, mode, mask, ldm, slope, K, nullptr, nbn, zero, bits);
    } else {
        gemm_f32_kernel<false><<<g, 256, 0, st>>>((int)P, N, K, dY, ldy, W, ldw, dX, ldx, mode, mask, ldm, slope, K, nullptr, nbn);
    }
}

// The sample dimension is cut into slabs of >= 512 samples, ~2 workgroups per CU per launch: a workgroup's fixed cost (ring fill,
// 64 atomics per lane) wants many K-steps per slab -- measured on the 2048-ray step: 1536 workgroups / 256-sample slabs 35.6 ms,
// 512 / 512 33.0 ms, 256 / 1024 34.5 ms; writing partial tiles and reducing them in a second pass instead of the atomics
// changed nothing at any setting (the atomics are not the cost).
int gemm_tn(hipStream_t st, bool x3, long P, const float *dY, long ldy, int M, const float *X, long ldx, int N, float *dW, long ldw, float *db,
            const float *zero, unsigned char *sign_bits, bool *bits_written)
{
    *bits_written = false;
    const int tiles = ((N + GT - 1) / GT) * ((M + GT - 1) / GT);
    static const long wg_target = sahs_diag_env("SAHS_BWD_TN_WGS") ? atol(sahs_diag_env("SAHS_BWD_TN_WGS")) : 512;      // (tuning aid)
    long kslab = (P * tiles / wg_target + 15) / 16 * 16;
    static const long min_slab = sahs_diag_env("SAHS_BWD_TN_MINSLAB") ? atol(sahs_diag_env("SAHS_BWD_TN_MINSLAB")) : 512;      // (tuning aid)
    kslab = kslab < min_slab ? min_slab : (kslab > 8192 ? 8192 : kslab);
    dim3 g((N + GT - 1) / GT, (M + GT - 1) / GT, (unsigned)((P + kslab - 1) / kslab));
    if (gemm_aligned(dY, ldy) && gemm_aligned(X, ldx)) {
        const int nx = (N + GT - 1) / GT, slabs = (int)((P + kslab - 1) / kslab);
        const dim3 g1((unsigned)((slabs + 7) / 8 * 8 * tiles), 1, 1);        // XCD-aware 1-D grid (kernel: nbn < 0)
        unsigned char *mb = (sign_bits != nullptr && N % 8 == 0 && N <= 256) ? sign_bits : nullptr;
        static const bool dbg_noatomic = sahs_diag_env("SAHS_BWD_DBG_NOATOMIC") != nullptr;      // timing experiment: results wrong
        if (dbg_noatomic) ldw = 0;
        if (x3) {
            static sahs_once::Flags attr_set;       // the large-LDS attribute is per device
            const hipError_t ae = sahs_once::per_device(attr_set, [&]() {
                return hipFuncSetAttribute(reinterpret_cast<const void *>(gemm_tn_split_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, TN_LDS_BYTES);
            });
            if (ae != hipSuccess) return (int)ae;
            gemm_tn_split_kernel<<<g1, TN_THREADS, TN_LDS_BYTES, st>>>(M, N, (int)P, dY, ldy, X, ldx, dW, ldw, (int)kslab, db, nx, zero, mb);
        } else gemm_dma_kernel<true, false><<<g1, 256, 0, st>>>(M, N, (int)P, dY, ldy, X, ldx, dW, ldw, 2, nullptr, 0, 0.0f, (int)kslab, db, -nx, zero, mb);
        *bits_written = mb != nullptr;
    } else {
        gemm_f32_kernel<true><<<g, 256, 0, st>>>(M, N, (int)P, dY, ldy, X, ldx, dW, ldw, 2, nullptr, 0, 0.0f, (int)kslab, db, 0);
    }
    return (int)hipGetLastError();
}

void copy2d(hipStream_t st, unsigned blocks, long M, int N, const float *src, long lds_, float *dst, long ldd, int mode)
{
    copy2d_kernel<<<blocks, 256, 0, st>>>(M, N, src, lds_, dst, ldd, mode);
}
void copy2d_batch(hipStream_t st, const CopyBatch &b, int n, int phase) { copy2d_batch_kernel<<<dim3(16, n), 256, 0, st>>>(b, phase); }
void const_cols_batch(hipStream_t st, const ConstBatch &b, int n) { const_cols_batch_kernel<<<n, 256, 0, st>>>(b); }
void axpy_batch(hipStream_t st, const AxpyBatch &b, int n) { axpy_batch_kernel<<<dim3(1, n), 256, 0, st>>>(b); }
void add_rows8(hipStream_t st, long n, const float *a, float *y) { add_rows8_kernel<<<2048, 256, 0, st>>>(n, a, y); }

}  // namespace sahs
