// field_bwd_gemm.hip -- the backward's kernels that depend on no model layout, built once (field_bwd_gemm.hpp has their launchers):
// three generations of dense fp32-in GEMM for the per-layer walk (register-staged, LDS-DMA, split-once weight gradient), the four job-table
// weight-gradient kernels of the fused walk with their plan code, and the copy / axpy / constant-column helpers.  For every dense layer
// dW += dY^T X (+ db = column sums of dY, fused),   dX = (dY W) * act'(X);  which layers there are is the business of field_bwd.hip.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include "sahs_common.hpp"
#include "field_bwd_gemm.hpp"
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
// side), so the four q groups of a ds_read_b32 hit two disjoint bank sets.
// ------------------------------------------------------------------------------------------------
// X3: the products on the bf16 matrix pipe at near-fp32 accuracy (the operand split of field_bf16x3.hip): every fp32 operand value is
// split on its way from LDS to the MFMA into x = hi + lo (hi = bf16(x), lo = bf16(x - hi): 16-17 significant bits together) and a product
// is three v_mfma_f32_32x32x16_bf16 with fp32 accumulation, a b ~= a_hi b_hi + a_hi b_lo + a_lo b_hi (the dropped a_lo b_lo term is ~2^-18
// of the product).  One 16-sample (TA) / 16-feature (!TA) K-step of the LDS ring is exactly one MFMA k-depth; a wave's 64 x 64 block is
// 2 x 2 tiles of 32 x 32, 12 MFMAs per K-step (384 matrix-pipe cycles against the 2048 of the 64 f32 MFMAs it replaces), so these GEMMs
// turn from matrix-bound into HBM-bound; the ~100 VALU instructions of the splits per K-step ride in the slack.  Same tiles, ring,
// epilogues and arguments as the f32 form (X3 = false), which stays selectable (SAHS_BWD_GEMM=f32) as the exact A/B reference.
typedef __attribute__((address_space(3))) void *lds_void_t;
typedef const __attribute__((address_space(1))) void *gbl_void_t;
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
// ring depth: 3 for the data-gradient GEMM (48 KB of LDS, three workgroups per CU, 16-step K loops), 4 for the weight-gradient GEMM (64 KB,
// two workgroups per CU by its registers anyway, K loops of 32..512 steps: three K-steps = 48 KB per workgroup in flight -- the
// kernel is HBM-bound and at depth 3 it reached 3.7 TB/s with 64 KB per CU in flight)
template <bool TA> constexpr int ring_depth() { return TA ? 4 : 3; }
constexpr int DTILE = GK * GT;                // floats per operand tile (8 KB)

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

template <bool TA, bool X3>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu((TA && X3) ? 2 : 3, 3))) gemm_dma_kernel(int M, int N, int K, const float *__restrict__ A, long lda,
                                                       const float *__restrict__ B, long ldb, float *__restrict__ C, long ldc, int mode,
                                                       const float *__restrict__ mask, long ldm, float slope, int kslab,
                                                       float *__restrict__ rowsum, int nbn, const float *__restrict__ zero,
                                                       unsigned char *__restrict__ bits)
{
    // bits (optional): the sign pattern of an activation matrix as a bit matrix, row r = N/8 bytes, bit (n & 7) of byte n >> 3 set where
    // X[r][n] > 0.  The weight-gradient GEMM (TA) WRITES it for its B operand X from the tiles it stages anyway (the m-block-0 workgroups);
    // the data-gradient GEMM of the same layer, which follows it and whose (leaky-)ReLU mask is that same X, READS it instead of the fp32
    // matrix -- 1/32 of the bytes of what was a third of its HBM traffic.
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
    const int h = lane >> 5, c32 = lane & 31;
    const float *src[4]; long step[4]; int krow[4]; bool colok[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int rp = (wave & 1) * 4 + u;                 // 0..7: which 1-KB eighth of the tile
        if (X3 && !TA && wave >= 2) {                        // B = pre-split, fragment-ordered weight pieces: a linear 8 KB copy per K-step
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
    // X3: lane (r32, h) of a 32x32x16 MFMA supplies k = 8h .. 8h+7 of row/column r32 of a 32-wide tile.  K-major tiles are swizzled on
    // alternate rows (TA: k & 1, !TA: (k >> 2) & 1), so a lane's eight k sit in two column positions: x3c[t][0] where the swizzle bit is
    // clear, x3c[t][1] where it is set.  (Row-major A of !TA: the eight k are 32 contiguous bytes of row m.)
    const int r32 = lane & 31;
    int x3a[2][2], x3b[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int m = 64 * wm + 32 * t + r32, n = 64 * wn + 32 * t + r32;
        x3a[t][0] = TA ? (((m >> 2) << 2) + (m & 3)) : (m * GK + 8 * h);
        x3a[t][1] = TA ? ((((m >> 2) ^ 4) << 2) + (m & 3)) : 0;
        x3b[t][0] = ((n >> 2) << 2) + (n & 3);
        x3b[t][1] = (((n >> 2) ^ 4) << 2) + (n & 3);
    }
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
    const bool pre_bits = !TA && mode != 2 && mask != nullptr && bits != nullptr;
    if constexpr (!TA) {
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
        if (TA && bits != nullptr && by == 0) {      // thread (kk, g): the 8 columns 8g .. 8g+7 of sample row kk of the X tile -> one byte
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
        if constexpr (X3) {
            u32x4_t ah[2], al[2], bh[2], bl[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                float x[8];
                if (TA) {
#pragma unroll
                    for (int j = 0; j < 8; ++j) x[j] = As[(8 * h + j) * GT + x3a[i][j & 1]];
                } else {
                    const f32x4 v0 = *reinterpret_cast<const f32x4 *>(As + x3a[i][0]), v1 = *reinterpret_cast<const f32x4 *>(As + x3a[i][0] + 4);
#pragma unroll
                    for (int j = 0; j < 4; ++j) { x[j] = v0[j]; x[4 + j] = v1[j]; }
                }
                split8(x, ah[i], al[i]);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                if constexpr (TA) {
                    float x[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) x[j] = Bs[(8 * h + j) * GT + x3b[i][j & 1]];
                    split8(x, bh[i], bl[i]);
                } else {      // weights arrive split and in fragment order (CopyJob pack): n-tile 2 wn + i, hi then lo
                    bh[i] = *reinterpret_cast<const u32x4_t *>(Bs + ((2 * wn + i) * 64 + lane) * 4);
                    bl[i] = *reinterpret_cast<const u32x4_t *>(Bs + GK * GT / 2 + ((2 * wn + i) * 64 + lane) * 4);
                }
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acx[i][j] = mfma3(ah[i], al[i], bh[j], bl[j], acx[i][j]);
            if (TA && do_sum && tid < GT) {
#pragma unroll
                for (int k = 0; k < GK; ++k) cs += As[k * GT + ((((tid >> 2) ^ ((k & 1) << 2)) << 2) + (tid & 3))];
            }
        } else if (TA) {
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
    if (!TA && mode != 2 && ((reinterpret_cast<uintptr_t>(C) | (mask ? reinterpret_cast<uintptr_t>(mask) : 0)) & 15) == 0 && ldc % 4 == 0 &&
        (mask == nullptr || ldm % 4 == 0)) {
        // Data-gradient epilogue through LDS: the accumulator layout gives 64-byte row segments per store instruction (64 mask loads
        // + 64 stores per lane); staged, every thread moves whole float4s of 512-byte rows (8 stores per lane per half).
        // Everything the stores need from memory -- the mask (as sign bits or as the fp32 activation) and, for mode 1, the old value -- is
        // fetched by ONE batch of loads per half through clamped addresses (no per-lane branches), ahead of the staging barrier; the
        // stores then follow each other with no wait between them.  (Round 3, from the cycle stamps of tools/stamp_gemm.py: with a load
        // inside each store's guard the compiler put `s_waitcnt vmcnt(0)` -- which on gfx9 also waits for every earlier STORE -- in front of
        // all 16 stores of a lane: a serial chain of 16 memory round trips, 60 % of this kernel's wave time.)
        constexpr int SLD = GT + 4;
        float *stage = &smem[0][0][0];                      // 64 x 132 floats = 33 KB of the 48 KB ring, free after the K loop
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
    if (TA && mode == 2) {
        // Weight-gradient epilogue through LDS as well: one atomic instruction then covers 256 contiguous bytes of a dW row
        // instead of four 64-byte segments of four rows.
        constexpr int SLD = GT + 4;
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
// The weight-gradient GEMM on the bf16 pipe, operands split ONCE per workgroup (round 3).  gemm_dma_kernel<true, true> splits every fp32
// operand value on its way from LDS into the MFMA -- in each of the two waves that use it, behind eight scalar LDS reads per fragment --
// and its K-step body (286 instructions per wave for 12 MFMAs) is what bounds it: s_memtime stamps (tools/stamp_gemm.py) put 2,250 of a
// K-step's 2,530 cycles into the body, 120 into the wait for the LDS-DMA and 155 into the barrier.  Here a K-step is two phases:
//   split   thread (operand = tid >> 7, column = tid & 127) reads its column's 16 samples of the fp32 stage (conflict-free: a wave reads 64
//           consecutive columns of one sample row), splits them (48 VALU instructions) and writes the column's hi and lo bf16 fragments
//           [column][16 k] with four ds_write_b128; the bias-gradient column sum rides on the same registers;
//   MFMA    a wave fetches its 2 + 2 (hi, lo) fragment pairs with eight ds_read_b128 (lane (r32, h): 16 bytes at column * 32 + 16 h) and
//           issues the 12 MFMAs.
// Same tiles, LDS-DMA ring (depth 4), XCD-aware 1-D grid, sign-bit emission, staged atomic epilogue and arguments as the kernel it replaces
// for X3; 64 KB ring + 16 KB fragments = 80 KB of LDS: two workgroups per CU.
constexpr int TN_DST = 4, TN_THREADS = 512;
constexpr int TN_RING_FLOATS = TN_DST * 2 * DTILE;
constexpr int TN_FRAG_DWORDS = 2 * 2 * GT * 8;             // [operand][hi | lo][column][8 dwords = 16 bf16]
constexpr int TN_LDS_BYTES = (TN_RING_FLOATS + TN_FRAG_DWORDS) * 4;
static_assert(TN_LDS_BYTES == 81920, "two workgroups per CU: 2 x 80 KB = the 160 KB of a gfx950 CU");

// One 128 x 128 tile of C += A^T B over the samples [k_lo, k_hi): the body shared by the per-layer kernel (one tile-slab per workgroup)
// and the job-table kernel (a workgroup walks many).  Ends on an LDS barrier: the ring and the fragment buffer are free on return.
// position (dwords) of column `col`'s 4 dwords (8 bf16: samples 8 h .. 8 h + 7 of a K-step) inside one [hi] or [lo] fragment block of GT
// columns: [32-column group][h][column of the group][4 dwords] -- the MFMA phase's lane (r32, h) and the split phase's thread (column, h) both
// touch 16 bytes at 16 x lane: conflict-free ds_read_b128 / ds_write_b128.  (Round 4, first form: [column][h][4 dwords] = a 32-byte lane
// stride, two lanes per bank group -- SQ_LDS_BANK_CONFLICT 1.5-1.7 x SQ_ACTIVE_INST_LDS in both weight-gradient kernels.)
__device__ __forceinline__ constexpr int frag_pos(int col, int h) { return ((col >> 5) * 64 + h * 32 + (col & 31)) * 4; }

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

    // this wave's two DMA instructions per K-step: waves 0..3 move the dY tile, waves 4..7 the X tile; K-major [16 k][128 cols], 32 chunks
    // per row, two rows per instruction, XOR-swizzled by 16 floats on odd rows (kept from gemm_dma_kernel: the sign-bit pass relies on it)
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
        if (bits != nullptr && by == 0 && tid < 256) {      // thread (kk, g): the 8 columns 8g .. 8g+7 of sample row kk of the X tile -> one byte
            const int kk = tid >> 4, g = tid & 15;
            const long k = k_lo + (long)t * GK + kk;
            if (k < k_hi && n0 + 8 * g < N) {
                const float *px = stage + DTILE + kk * GT + 4 * ((2 * g) ^ ((kk & 1) << 2));     // chunks 2g, 2g+1 stay adjacent under the swizzle
                const f32x4 v0 = *reinterpret_cast<const f32x4 *>(px), v1 = *reinterpret_cast<const f32x4 *>(px + 4);
                unsigned b8 = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) b8 |= (v0[i] > 0.0f ? 1u : 0u) << i | (v1[i] > 0.0f ? 1u : 0u) << (4 + i);
                bits[k * (N >> 3) + (n0 >> 3) + g] = (unsigned char)b8;
            }
        }
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

// ------------------------------------------------------------------------------------------------
// ALL weight-gradient GEMMs of a walk in ONE launch (round 4).  Per launch the kernel above pays ring fill, a K loop with one workgroup
// per CU, 64 KB of atomics per workgroup, ramp and tail -- 35-40 us of a 45-200 us launch, 82 times per training step (DESIGN.md section
// 7).  Here persistent workgroups (two per CU) walk a job table: job = one layer's dW (+ db) = dY^T X with dY, X dense [P x width]
// planes; item = (sample range r, job, 128 x 128 tile), ranges of `range` samples (the same for every job: items cost the same), item
// index = r * tiles_total + tile, so that the tiles of one job and range -- which stream the same dY and X rows -- sit on neighbouring
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
    // DMA: 32 one-KB units per K-step (block b, row pair rp); wave w moves units 4 w .. 4 w + 3 = row pairs 4 (w & 1) .. of block w >> 1.
    // K-major [16 k][128 cols], XOR-swizzled by 16 floats on odd rows as in tn_tile.
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
// split phase: the MFMA lanes read their operands straight from the ring (lane (q, c16): sample 4 s4 + q, column 16 i + c16 -- ds_read_b32,
// conflict-free under the swizzle), four samples per MFMA.  Bound: the f32 matrix pipe -- a 256 x 256 block is 128 MFMAs per wave and K-step
// (4096 cycles) against 32 KB of operands -- not HBM.  Ring of four K-steps.
constexpr int TF_DST = 4;
constexpr int TF_LDS_BYTES = TF_DST * 2 * DTILE * 4;                           // 64 KB: two workgroups per CU
constexpr int TFW_DST = 5;                                                     // the wide kernel's ring: all 160 KB of the CU, four K-steps in flight
constexpr int TFW_LDS_BYTES = TFW_DST * TW_STAGE_FLOATS * 4;                   // 160 KB: one workgroup per CU
__device__ __forceinline__ int swz_col(int col, int odd) { return (((col >> 2) ^ (odd << 2)) << 2) + (col & 3); }

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
    // DMA as in tn_tile: waves 0..3 move the dY tile, waves 4..7 the X tile, two instructions per wave and K-step
    // (K-steps are issued in order: the lane's source pointers simply advance; columns past the operand's width read the zero page and stay
    // there; rows past k_hi exist in the last K-step of a ragged range only -- a uniform test)
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
    // DMA as in tn_block256: 32 one-KB units per K-step (block b, row pair rp); wave w moves row pairs 4 (w & 1) .. of block w >> 1
    // (pointers advance per K-step as in tn_tile_f32)
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

// per-frame constants: dW[r][col0 + k] += db[r] * c[k];  dc[k] += sum_r W[r][col0 + k] * db[r].  One workgroup per column k.
__global__ void __launch_bounds__(256) const_cols_backward_kernel(int rows, int cols, const float *__restrict__ W, float *__restrict__ dW, long ld,
                                                                  int col0, const float *__restrict__ db, const float *__restrict__ c,
                                                                  float *__restrict__ dc)
{
    const int k = blockIdx.x;
    const float ck = c[k];
    float s = 0.0f;
    for (int r = threadIdx.x; r < rows; r += blockDim.x) {
        const float g = db[r];
        s += W[(long)r * ld + col0 + k] * g;
        atomicAdd(dW + (long)r * ld + col0 + k, g * ck);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    __shared__ float red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(dc + k, (red[0] + red[1]) + (red[2] + red[3]));
}

__global__ void axpy_kernel(int n, const float *__restrict__ x, float *__restrict__ y)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) atomicAdd(y + i, x[i]);
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
void const_cols(hipStream_t st, int rows, int cols, const float *W, float *dW, long ld, int col0, const float *db, const float *c, float *dc)
{
    const_cols_backward_kernel<<<cols, 256, 0, st>>>(rows, cols, W, dW, ld, col0, db, c, dc);
}
void const_cols_batch(hipStream_t st, const ConstBatch &b, int n) { const_cols_batch_kernel<<<n, 256, 0, st>>>(b); }
void axpy(hipStream_t st, unsigned blocks, int n, const float *x, float *y) { axpy_kernel<<<blocks, 256, 0, st>>>(n, x, y); }
void axpy_batch(hipStream_t st, const AxpyBatch &b, int n) { axpy_batch_kernel<<<dim3(1, n), 256, 0, st>>>(b); }
void add_rows8(hipStream_t st, long n, const float *a, float *y) { add_rows8_kernel<<<2048, 256, 0, st>>>(n, a, y); }

}  // namespace sahs
