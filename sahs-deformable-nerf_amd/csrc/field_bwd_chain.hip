// field_bwd_chain.hip -- the data-gradient chain of the field backward, sample-major, on the bf16 matrix pipe with split operands.
//
// Autograd of the reference's per-sample networks (modules.py:254-295 NeRFMLP, :371-390 WarpFieldMLP, :444-462 HyperSheetMLP, as driven by
// train_stage_rays_auto.py:437-499) needs, for every dense layer, the gradient of its pre-activation, dZ_l = (W_{l+1}^T dZ_{l+1}) * act'(z_l).
// Rounds 1-3 ran that as one GEMM launch per layer over all samples (field_bwd.hip: nn()), every dZ going through HBM twice.  Here ONE
// launch walks a whole net backwards for 32 samples per wave, exactly as the split-operand forward of field_bf16x3.hip walks it forwards
// (bf16x3_pipe.hpp: dense_x -- the 32x32 accumulator tile of one layer becomes the hi/lo B fragments of the next in registers), with
//   * transposed weight streams (A = W^T in MFMA fragment order, split into bf16 hi + lo by pack_bwd_stream_kernel once per walk),
//   * the (leaky-)ReLU derivative taken from the sign bits the saving forward wrote (sahs_layout.hpp: sbits; 1 bit per value instead of the
//     saved fp32 activation), applied as v_bfe_i32 + v_bfi_b32 on the value's way into the conversion,
//   * every dZ tile stored once, fp32, into the plane of its layer (the act:: layout: dZ of a layer sits where its activation sits in
//     the saved-activation buffer) -- the operands of the weight-gradient launch that follows (field_bwd_tn_jobs.hip: gemm_tn_jobs_kernel).
// Same arithmetic as the per-layer split-operand GEMMs it replaces (hi*hi + hi*lo + lo*hi, fp32 accumulation), a different summation
// order.  Built once per model (sahs_model.hpp): the layer programs below follow each model's trunk (8 layers for the AudioFaceModel, 4 for
// the NeRFaceModels, skip layer 3 in all) and the NeRFaceModel without deformation nets (SAHS_MODEL 2) has no deformation chain and no
// encodings' gradient -- nothing upstream of its raw sample point has parameters.
#include <hip/hip_runtime.h>
#include <utility>
#include "sahs_common.hpp"
#include "sahs_launchers.hpp"
#include "sahs_layout.hpp"
#include "bwd_program.hpp"
#include "bf16_pipe.hpp"
#include "bf16x3_pipe.hpp"

namespace SAHS_NS {
namespace bwc {
using namespace hx3;

// ---- the backward layer program: bwd_program.hpp's, in 32-row tiles and 32-gradient k-blocks (halfwords of hi + lo), chunked as dense_x
// streams it.  The enums name its layers in the order of bwp::make_rad / make_def = the order of the stream = the order in which the
// kernels below walk it (the trunk from fc_feat back: T<i>IN = the encodings' rows of a layer that reads [PE(x') | PE(w)], T<i> = its
// hidden rows) ------------------------------------------------------------------------------------------------------------------------
#if SAHS_MODEL == 0
enum RadLayer { R_RGBH, R_D3, R_D2, R_D1, R_GRIDF, R_SEGH, R_S3, R_S2, R_S1, R_FEATIN, R_FEAT, R_T7, R_T6, R_T5, R_T4, R_T3IN, R_T3, R_T2, R_T1, R_T0IN, R_COUNT };
#elif SAHS_MODEL == 1
enum RadLayer { R_RGBH, R_D3, R_D2, R_D1, R_GRIDF, R_SEGH, R_S3, R_S2, R_S1, R_FEATIN, R_FEAT, R_T3IN, R_T3, R_T2, R_T1, R_T0IN, R_COUNT };
#else
enum RadLayer { R_RGBH, R_D3, R_D2, R_D1, R_GRIDF, R_SEGH, R_S3, R_S2, R_S1, R_FEATIN, R_FEAT, R_T3, R_T2, R_T1, R_COUNT };
#endif
enum DefLayer { D_HF, D_H5, D_H4, D_H3, D_H2, D_H1, D_WF, D_W5, D_W4, D_W3, D_W2, D_W1, D_COUNT };
static_assert(!USE_DEFORM || DIN_LD == 96 || DIN_LD == 128, "the encodings' rows are one 32-row tile short of or exactly the layer's 4 tiles");
#if SAHS_MODEL != 2
constexpr bwp::Prog<D_COUNT> kDef = bwp::make_def<32, D_COUNT>(pick_GX);
__device__ const bwp::Prog<D_COUNT> dDef = kDef;
static_assert(kDef.n == D_COUNT, "DefLayer names every layer of the program");
constexpr long DEF_HW = kDef.stream;         // halfwords of the deformation stream
#else
constexpr long DEF_HW = 0;                   // (no deformation nets)
#endif
constexpr bwp::Prog<R_COUNT> kRad = bwp::make_rad<32, R_COUNT>(pick_GX);
__device__ const bwp::Prog<R_COUNT> dRad = kRad;
static_assert(kRad.n == R_COUNT, "RadLayer names every layer of the program");
constexpr long RAD_HW = kRad.stream;         // halfwords of a level's radiance stream
static_assert(RAD_HW % 8 == 0 && DEF_HW % 8 == 0, "16-byte granules");

// ---- transposed, split stream of one part: [layer][tile32][k-step][hi 64 x 8 | lo 64 x 8]; lane 32 h + i of k-step (block b, step st)
// holds A[32 t + i][32 b + 16 st + 8 (j >> 2) + 4 h + (j & 3)], j = 0..7 (the B-operand order of bf16x3_pipe.hpp) -----------------------
template <int N>
__device__ __forceinline__ void pack_one(const bwp::Prog<N> &Pg, const float *__restrict__ flat, unsigned short *__restrict__ out, int level, long e)
{
    const long hw = e * 16;                                // one thread: the hi AND lo fragment granule of one lane (2 x 8 halfwords)
    const bwp::BLayer &L = bwp::layer_at(Pg, hw);
    const long w = hw - L.stream_off;
    const int per_tile = L.KB * 2048;
    const int t = (int)(w / per_tile);
    const int rem = (int)(w - (long)t * per_tile);
    const int f = rem >> 10, lane = (rem & 1023) >> 4;     // fragment pair f = 2 b + st; 16 halfwords (hi 8 + lo 8) per lane and pair
    const int b = f >> 1, st = f & 1, i = lane & 31, h = lane >> 5;
    const bwp::Spot at = bwp::spot<32>(L, level, 32 * t + i, b);
    unsigned short vh[8], vl[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const long src = bwp::element(at, 16 * st + 8 * (j >> 2) + 4 * h + (j & 3));
        const float x = src >= 0 ? flat[src] : 0.0f;
        const __bf16 hi = (__bf16)x;
        vh[j] = __builtin_bit_cast(unsigned short, hi);
        vl[j] = __builtin_bit_cast(unsigned short, (__bf16)(x - (float)hi));
    }
    unsigned short *dst = out + L.stream_off + (long)t * per_tile + (long)f * 1024 + lane * 8;
    uint4 q;
    q.x = vh[0] | ((unsigned)vh[1] << 16); q.y = vh[2] | ((unsigned)vh[3] << 16);
    q.z = vh[4] | ((unsigned)vh[5] << 16); q.w = vh[6] | ((unsigned)vh[7] << 16);
    *reinterpret_cast<uint4 *>(dst) = q;
    q.x = vl[0] | ((unsigned)vl[1] << 16); q.y = vl[2] | ((unsigned)vl[3] << 16);
    q.z = vl[4] | ((unsigned)vl[5] << 16); q.w = vl[6] | ((unsigned)vl[7] << 16);
    *reinterpret_cast<uint4 *>(dst + 512) = q;
}
__global__ void __launch_bounds__(256) pack_bwd_stream_kernel(const float *__restrict__ flat, unsigned short *__restrict__ out, int level, int part)
{
    const long total = (part == 1 ? DEF_HW : RAD_HW) / 16;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
#if SAHS_MODEL != 2
        if (part == 1) pack_one(dDef, flat, out, 0, e);
        else
#endif
            pack_one(dRad, flat, out, level, e);
    }
}

// ---- the backward epilogue: derivative mask from the forward's sign bits, dZ stored once --------------------------------------------
// This lane (sample, h) of 32-row tile TILE holds, as value U = 4 g + i, feature 32 TILE + 8 g + 4 h + i: bit 8 TILE + 4 (g >> 1) + i of
// sign word q = h (g even) or q = 2 + h (g odd) -- sahs_layout.hpp: sbits.  MASKED = false: no activation behind this gradient (d feat, the
// encodings' gradient).  Tiles >= NVALID are padding (not stored).  dst = (uniform plane base, this lane's byte offset of its row + 4 h).
// Where a finished group of four values goes: NOT straight to memory -- the accumulator layout would make every store instruction write 32
// bytes into each of 32 rows (quarter cache lines; measured: the chain kernel then runs at 2.4 TB/s of stores, compute and stores adding up) --
// but through a per-wave 32 x 32 staging tile in LDS: the lane writes its four values (ds_write_b128), and once the tile's fourth group is in,
// the wave reads the tile back row-major and stores it as WHOLE 128-byte lines: lane l -> rows (l >> 3) + 8 i, i = 0..3, 16 bytes (l & 7).
struct StageCtx {
    uint32_t wr, rd;          // LDS byte addresses: this lane's row (+16 h) for writing; row l >> 3, piece l & 7 for reading back
    uint32_t pc;              // 16 (l & 7): the piece's byte offset inside a 128-byte tile row
    uint32_t prow[4];         // the sample index of read-back row i (clamped to P - 1 like the lane's own sample)
    uint32_t np;              // P
};
constexpr int STAGE_ROW_BYTES = 144;                                      // 32 floats + 4 of padding: 16-byte aligned rows, spread over the banks
constexpr int STAGE_WAVE_BYTES = 32 * STAGE_ROW_BYTES;

template <bool MASKED, int NVALID, int WIDTH>
struct BwdEp {
#if defined(SAHS_DIAG) && (defined(SAHS_BWC_NOSTORE) || defined(SAHS_BWC_NOGSTORE))
    static constexpr bool stores(int) { return false; }
#else
    static constexpr bool stores(int tile) { return tile < NVALID; }      // (the counted wait of bf16x3_pipe.hpp: at least one store per group)
#endif
    float slope;
    uint32_t mh[2], m2[2];
    float *base;              // the layer's dZ plane (uniform)
    StageCtx sc;
    template <int TILE, int U> __device__ __forceinline__ float value(float v, float m) const
    {
        if constexpr (!MASKED) {
            return v;
        } else {
            constexpr int g = U >> 2, i = U & 3, bit = 8 * TILE + 4 * (g >> 1) + i;
            const uint32_t w = (g & 1) ? m2[bit >> 5] : mh[bit >> 5];
            const uint32_t t = (uint32_t)((int32_t)(w << (31 - (bit & 31))) >> 31);      // v_bfe_i32: all ones where the activation was > 0
            if (slope == 0.0f) return __builtin_bit_cast(float, t & __builtin_bit_cast(uint32_t, v));
            return __builtin_bit_cast(float, (t & __builtin_bit_cast(uint32_t, v)) | (~t & __builtin_bit_cast(uint32_t, m)));      // v_bfi_b32
        }
    }
    template <int TILE, int G> __device__ __forceinline__ void done4(const float (&r)[4], uint32_t (&)[2]) const
    {
#if defined(SAHS_DIAG) && defined(SAHS_BWC_NOSTORE)      // timing-only: results wrong by construction
        asm volatile("" :: "v"(r[0]), "v"(r[1]), "v"(r[2]), "v"(r[3]));
#else
        if constexpr (TILE < NVALID) {
            *(lds_f4_t)(uintptr_t)(sc.wr + 32 * G) = f32x4{r[0], r[1], r[2], r[3]};
            if constexpr (G == 3) {
                f32x4 v[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = *(lds_f4_t)(uintptr_t)(sc.rd + i * 8 * STAGE_ROW_BYTES);
#if defined(SAHS_DIAG) && defined(SAHS_X3_NOREADBACK)      // timing-only (results wrong by construction): the stores without waiting for the read-back
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = f32x4{r[0], r[1], r[2], r[3]};
#endif
#if defined(SAHS_DIAG) && defined(SAHS_BWC_NOGSTORE)      // timing-only: the staging round trip without the global stores
#pragma unroll
                for (int i = 0; i < 4; ++i) asm volatile("" :: "v"(v[i]));
#elif defined(SAHS_DIAG) && defined(SAHS_BWC_TILEMAJOR)      // timing-only: the same bytes as 4 KB contiguous runs per wave and tile (the weight-gradient launch would read garbage)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    *reinterpret_cast<f32x4 *>(reinterpret_cast<char *>(base) + (size_t)TILE * (sc.np * 128u) + (sc.prow[i] * 128u + sc.pc)) = v[i];
#elif defined(SAHS_DIAG) && defined(SAHS_BWC_PLAINSTORE)      // A/B: default cache policy instead of non-temporal
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    *reinterpret_cast<f32x4 *>(reinterpret_cast<char *>(base) + (sc.prow[i] * (uint32_t)(WIDTH * 4) + sc.pc + 128u * TILE)) = v[i];
#else
                // non-temporal: 4.4 GB of dZ per launch stream THROUGH the L2 that holds the 3 MB weight stream every workgroup re-reads
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    __builtin_nontemporal_store(v[i], reinterpret_cast<f32x4 *>(reinterpret_cast<char *>(base) + (sc.prow[i] * (uint32_t)(WIDTH * 4) + sc.pc + 128u * TILE)));
#endif
            }
        }
#endif
    }
};
struct NoEp {      // (the pending-tile policy of a layer that has none)
    static constexpr bool stores(int) { return false; }
    float slope;
    template <int TILE, int U> __device__ __forceinline__ float value(float v, float) const { return v; }
    template <int TILE, int G> __device__ __forceinline__ void done4(const float (&)[4], uint32_t (&)[2]) const {}
};

// the last tile of a chain's last layer: nothing follows that would convert it under its MFMAs
template <int PTILE, class PEP>
__device__ __forceinline__ void flush_x(St &st, const PEP pep)
{
    Blk dummy;
    pack_ticks<0, PACK_TICKS, PTILE>(st.acc[1], dummy, pep, st.ps);
    fence();
}

constexpr int BWC_ZERO_BYTES = 2048;                                       // the "bias" of every backward layer: zeros
constexpr int BWC_STAGE_BYTE_OFF = LDS_BIAS_BYTE_OFF + BWC_ZERO_BYTES;     // staging tiles behind the zero bias page
// this lane's part in staging its wave's tiles (StageCtx): the wave's 32 samples are consecutive, p0 = 128 tile + 32 wave
__device__ __forceinline__ StageCtx make_stage(const char *lds, int wave, int lane, long tile, long P)
{
    StageCtx sc;
    const uint32_t base = lds_addr_of(lds) + BWC_STAGE_BYTE_OFF + (uint32_t)wave * STAGE_WAVE_BYTES;
    sc.wr = base + (uint32_t)(lane & 31) * STAGE_ROW_BYTES + 16u * (lane >> 5);
    sc.rd = base + (uint32_t)(lane >> 3) * STAGE_ROW_BYTES + 16u * (lane & 7);
    sc.pc = 16u * (lane & 7);
    const long p0 = tile * X_PTS_PER_WG + wave * X_PTS_PER_WAVE + (lane >> 3);
#pragma unroll
    for (int i = 0; i < 4; ++i) sc.prow[i] = (uint32_t)(p0 + 8 * i < P ? p0 + 8 * i : P - 1);
    sc.np = (uint32_t)P;
    return sc;
}

constexpr int BWC_LDS_BYTES = BWC_STAGE_BYTE_OFF + (X_THREADS / WAVE) * STAGE_WAVE_BYTES;
static_assert(BWC_LDS_BYTES <= 160 * 1024, "LDS budget");

// a (P,4)/(P,16) gradient row as the one 32-feature block of a head layer: k-step 0 = columns 4 h .. 4 h + 3 and 8 + 4 h .. 8 + 4 h + 3
__device__ __forceinline__ void head_block(const f32x4 a, const f32x4 b, Blk &o)
{
    const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
#pragma unroll
    for (int jp = 0; jp < 4; ++jp) {
        uint32_t hi, lo;
        split_pair(v[2 * jp], v[2 * jp + 1], hi, lo);
        o.s[0][jp] = hi; o.l[0][jp] = lo;
    }
    o.s[1] = u32x4{0u, 0u, 0u, 0u};
    o.l[1] = u32x4{0u, 0u, 0u, 0u};
}

__device__ __forceinline__ void zero_block(Blk &o)
{
    o.s[0] = o.s[1] = o.l[0] = o.l[1] = u32x4{0u, 0u, 0u, 0u};
}

#define CHR(id) (kRad.layer[id].chunk)
#define CHD(id) (kDef.layer[id].chunk)

// Radiance nets of one level, backwards.  d_raw (P,16); bits: the radiance sign planes (sbits::BR_*); dact: plane c of the act:: table at
// dact + c * P (written: C, S, FEAT, T planes); dgridf (P,32); din_a, din_b (P,96): the encodings' gradient through the skip layer and
// through layer 0 (summed by encode_backward).
__global__ void __launch_bounds__(X_THREADS, 1)
field_backward_chain_rad_kernel(const unsigned short *__restrict__ stream, long P, const float *__restrict__ d_raw, const uint32_t *__restrict__ bits,
                                float *__restrict__ dact, float *__restrict__ dgridf, float *__restrict__ din_a, float *__restrict__ din_b)
{
    extern __shared__ __attribute__((aligned(16))) char lds_x[];
    Ctx cx;
    cx.stream = stream;
    cx.lds = lds_x;
    cx.buf = 0;
    cx.lane = threadIdx.x & 63;
    cx.h = cx.lane >> 5;
    cx.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = cx.h, col = cx.lane & 31;
    {
        float *zl = reinterpret_cast<float *>(lds_x + LDS_BIAS_BYTE_OFF);
        for (int i = threadIdx.x; i < BWC_ZERO_BYTES / 4; i += X_THREADS) zl[i] = 0.0f;
        cx.wrap_at = (uint32_t)RAD_HW;
        cx.wrap_to = 0u;
        cx.off = 0u;
        cx.prepare(CHR(R_RGBH), 0);
#pragma unroll
        for (int pc = 0; pc < (CHR(R_RGBH) + PIECE_HW - 1) / PIECE_HW; ++pc) cx.issue_piece(pc);
        __syncthreads();
    }
    const long ntiles = (P + X_PTS_PER_WG - 1) / X_PTS_PER_WG;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        cx.refresh_bias_base();
        asm volatile("" : "+s"(cx.off));      // (chunk addresses are loop-invariant: keep them from being hoisted and spilled)
        long Pq = P;
        asm volatile("" : "+s"(Pq));          // (and the ~30 plane bases c * P)
        St st;
        const long p_raw = tile * X_PTS_PER_WG + cx.wave * X_PTS_PER_WAVE + col;
        const long p = p_raw < P ? p_raw : P - 1;      // lanes past the end redo the last sample: identical values to identical addresses
        const uint32_t pl = (uint32_t)p;
        const StageCtx sc = make_stage(lds_x, cx.wave, cx.lane, tile, P);
        // policies: sign words of plane (word offset b, NW words per q) + the dZ plane at act:: column c
        auto ep128 = [&](int b, int c) {
            BwdEp<true, 4, 128> e;
            e.slope = 0.01f;
            const uint32_t *a = bits + (long)b * Pq + ((long)pl * 4 + h);
#if defined(SAHS_DIAG) && defined(SAHS_BWC_NOMASK)       // timing-only
            e.mh[0] = pl; e.m2[0] = pl + h; (void)a;
#else
            e.mh[0] = a[0]; e.m2[0] = a[2];
#endif
            e.mh[1] = 0u; e.m2[1] = 0u;
            e.base = dact + (long)c * Pq;
            e.sc = sc;
            return e;
        };
        auto ep256 = [&](int b, int c) {
            BwdEp<true, 8, 256> e;
            e.slope = 0.01f;
            const uint32_t *a = bits + (long)b * Pq + ((long)pl * 4 + h) * 2;
#if defined(SAHS_DIAG) && defined(SAHS_BWC_NOMASK)
            e.mh[0] = pl; e.mh[1] = pl ^ 5u; e.m2[0] = pl + h; e.m2[1] = pl * 3u; (void)a;
#else
            e.mh[0] = a[0]; e.mh[1] = a[1]; e.m2[0] = a[4]; e.m2[1] = a[5];
#endif
            e.base = dact + (long)c * Pq;
            e.sc = sc;
            return e;
        };
        Blk draw[2];
        {
            const f32x4 *r = reinterpret_cast<const f32x4 *>(d_raw + p * D_RAW);
            head_block(r[h], r[2 + h], draw[0]);
            zero_block(draw[1]);
        }
        Blk dC0[4], dS0[4];
        {   // colour branch: d_raw -> dC3 -> dC2 -> dC1 -> dC0 (-> d grid features)
            Blk cA[4];
            auto e3 = ep128(sbits::BR_C + 12, act::C + 384);
            auto e2 = ep128(sbits::BR_C + 8, act::C + 256);
            dense_x<2, 0, 0, 4, CHR(R_D3), false>(cx, st, draw, nullptr, nullptr, cA, 0, e3, NoEp{1.0f});
            auto e1 = ep128(sbits::BR_C + 4, act::C + 128);
            dense_x<4, 0, 0, 4, CHR(R_D2), true, 3>(cx, st, cA, nullptr, nullptr, dC0, 0, e2, e3);
            auto e0 = ep128(sbits::BR_C + 0, act::C + 0);
            dense_x<4, 0, 0, 4, CHR(R_D1), true, 3>(cx, st, dC0, nullptr, nullptr, cA, 0, e1, e2);
            dense_x<4, 0, 0, 4, CHR(R_GRIDF), true, 3>(cx, st, cA, nullptr, nullptr, dC0, 0, e0, e1);
            BwdEp<false, 1, 32> eg;
            eg.slope = 1.0f; eg.base = dgridf; eg.sc = sc;
            Blk dummy[2];
            dense_x<4, 0, 0, 2, CHR(R_SEGH), true, 3>(cx, st, dC0, nullptr, nullptr, dummy, 0, eg, e0);
        }
        BwdEp<true, 4, 128> es0;
        {   // seg branch: d_raw -> dS3 -> dS2 -> dS1 -> dS0
            Blk sA[4];
            auto e3 = ep128(sbits::BR_S + 12, act::S + 384);
            auto e2 = ep128(sbits::BR_S + 8, act::S + 256);
            dense_x<2, 0, 0, 4, CHR(R_S3), false>(cx, st, draw, nullptr, nullptr, sA, 0, e3, NoEp{1.0f});
            auto e1 = ep128(sbits::BR_S + 4, act::S + 128);
            dense_x<4, 0, 0, 4, CHR(R_S2), true, 3>(cx, st, sA, nullptr, nullptr, dS0, 0, e2, e3);
            es0 = ep128(sbits::BR_S + 0, act::S + 0);
            dense_x<4, 0, 0, 4, CHR(R_S1), true, 3>(cx, st, dS0, nullptr, nullptr, sA, 0, e1, e2);
            dense_x<4, 0, 0, 4, CHR(R_FEATIN), true, 3>(cx, st, sA, nullptr, nullptr, dS0, 0, es0, e1);
        }
        Blk F[8], G[8];
        {   // d feat (no activation behind it), then the trunk
            BwdEp<false, 8, 256> ef;
            ef.slope = 1.0f; ef.base = dact + (long)act::FEAT * Pq; ef.sc = sc;
#if SAHS_MODEL == 0
            auto e7 = ep256(sbits::BR_T + 8 * 7, act::T + 7 * 256);
            dense_x<4, 4, 1, 8, CHR(R_FEAT), true, 3>(cx, st, dS0, dC0, draw, F, 0, ef, es0);
            auto e6 = ep256(sbits::BR_T + 8 * 6, act::T + 6 * 256);
            dense_x<8, 0, 0, 8, CHR(R_T7), true, 7>(cx, st, F, nullptr, nullptr, G, 0, e7, ef);
            auto e5 = ep256(sbits::BR_T + 8 * 5, act::T + 5 * 256);
            dense_x<8, 0, 0, 8, CHR(R_T6), true, 7>(cx, st, G, nullptr, nullptr, F, 0, e6, e7);
            auto e4 = ep256(sbits::BR_T + 8 * 4, act::T + 4 * 256);
            dense_x<8, 0, 0, 8, CHR(R_T5), true, 7>(cx, st, F, nullptr, nullptr, G, 0, e5, e6);
            auto e3 = ep256(sbits::BR_T + 8 * 3, act::T + 3 * 256);
            dense_x<8, 0, 0, 8, CHR(R_T4), true, 7>(cx, st, G, nullptr, nullptr, F, 0, e4, e5);
            auto e2 = ep256(sbits::BR_T + 8 * 2, act::T + 2 * 256);
            dense_x<8, 0, 0, 8, CHR(R_T3IN), true, 7>(cx, st, F, nullptr, nullptr, G, 0, e3, e4);      // G = dT3 (last tile pending)
            BwdEp<false, 3, 96> ea;
            ea.slope = 1.0f; ea.base = din_a; ea.sc = sc;
            {
                Blk dummy[4];
                dense_x<8, 0, 0, 4, CHR(R_T3), true, 7>(cx, st, G, nullptr, nullptr, dummy, 0, ea, e3);  // d [PE(x') | PE(w)] through the skip layer
            }
            auto e1 = ep256(sbits::BR_T + 8 * 1, act::T + 1 * 256);
            dense_x<8, 0, 0, 8, CHR(R_T2), false>(cx, st, G, nullptr, nullptr, F, 0, e2, NoEp{1.0f});
            auto e0 = ep256(sbits::BR_T + 0, act::T + 0);
            dense_x<8, 0, 0, 8, CHR(R_T1), true, 7>(cx, st, F, nullptr, nullptr, G, 0, e1, e2);
            dense_x<8, 0, 0, 8, CHR(R_T0IN), true, 7>(cx, st, G, nullptr, nullptr, F, 0, e0, e1);      // F = dT0
            BwdEp<false, 3, 96> eb;
            eb.slope = 1.0f; eb.base = din_b; eb.sc = sc;
            {
                Blk dummy[4];
                dense_x<8, 0, 0, 4, CHR(R_RGBH), true, 7>(cx, st, F, nullptr, nullptr, dummy, 0, eb, e0);
            }
#elif SAHS_MODEL == 1
            // 4-layer trunk, skip layer 3 = the last: d feat -> dT3 (-> d [PE(x') | PE(w)], 128 rows = four whole tiles) -> dT2 -> dT1 -> dT0
            auto e3 = ep256(sbits::BR_T + 8 * 3, act::T + 3 * 256);
            dense_x<4, 4, 1, 8, CHR(R_FEAT), true, 3>(cx, st, dS0, dC0, draw, F, 0, ef, es0);
            dense_x<8, 0, 0, 8, CHR(R_T3IN), true, 7>(cx, st, F, nullptr, nullptr, G, 0, e3, ef);      // G = dT3 (last tile pending)
            BwdEp<false, DIN_LD / 32, DIN_LD> ea;
            ea.slope = 1.0f; ea.base = din_a; ea.sc = sc;
            {
                Blk dummy[4];
                dense_x<8, 0, 0, 4, CHR(R_T3), true, 7>(cx, st, G, nullptr, nullptr, dummy, 0, ea, e3);  // d [PE(x') | PE(w)] through the skip layer
                flush_x<3>(st, ea);      // (its last tile holds PE(w) rows: stored here, nothing after it converts it)
            }
            auto e2 = ep256(sbits::BR_T + 8 * 2, act::T + 2 * 256);
            auto e1 = ep256(sbits::BR_T + 8 * 1, act::T + 1 * 256);
            dense_x<8, 0, 0, 8, CHR(R_T2), false>(cx, st, G, nullptr, nullptr, F, 0, e2, NoEp{1.0f});
            auto e0 = ep256(sbits::BR_T + 0, act::T + 0);
            dense_x<8, 0, 0, 8, CHR(R_T1), true, 7>(cx, st, F, nullptr, nullptr, G, 0, e1, e2);
            dense_x<8, 0, 0, 8, CHR(R_T0IN), true, 7>(cx, st, G, nullptr, nullptr, F, 0, e0, e1);      // F = dT0
            BwdEp<false, DIN_LD / 32, DIN_LD> eb;
            eb.slope = 1.0f; eb.base = din_b; eb.sc = sc;
            {
                Blk dummy[4];
                dense_x<8, 0, 0, 4, CHR(R_RGBH), true, 7>(cx, st, F, nullptr, nullptr, dummy, 0, eb, e0);
                flush_x<3>(st, eb);
            }
#else
            // no deformation nets: nothing upstream of the raw sample point has parameters, so the chain stops at dT0 (the encodings' rows
            // of layers 0 and 3 only enter the weight gradients)
            (void)din_a; (void)din_b;
            auto e3 = ep256(sbits::BR_T + 8 * 3, act::T + 3 * 256);
            dense_x<4, 4, 1, 8, CHR(R_FEAT), true, 3>(cx, st, dS0, dC0, draw, F, 0, ef, es0);
            auto e2 = ep256(sbits::BR_T + 8 * 2, act::T + 2 * 256);
            dense_x<8, 0, 0, 8, CHR(R_T3), true, 7>(cx, st, F, nullptr, nullptr, G, 0, e3, ef);
            auto e1 = ep256(sbits::BR_T + 8 * 1, act::T + 1 * 256);
            dense_x<8, 0, 0, 8, CHR(R_T2), true, 7>(cx, st, G, nullptr, nullptr, F, 0, e2, e3);
            auto e0 = ep256(sbits::BR_T + 0, act::T + 0);
            dense_x<8, 0, 0, 8, CHR(R_T1), true, 7>(cx, st, F, nullptr, nullptr, G, 0, e1, e2);
            dense_x<8, 0, 0, 8, CHR(R_RGBH), true, 7>(cx, st, G, nullptr, nullptr, F, 0, e0, e1);      // F = dT0 (last tile pending)
            flush_x<7>(st, e0);
#endif
        }
    }
}

#if SAHS_MODEL != 2
// Deformation nets, backwards.  xwg (P,8): the seam gradient [dx'0 dx'1 dx'2 . dw0 dw1 . .]; actbuf: the saved activations (DX plane:
// tanh'); bits: the deformation sign planes (sbits::BD_*); dact: dZ planes WH, HH; g3, dw4 (P,4): the heads' pre-activation gradients
// [dx' (1 - dx^2) | 0], [dw | 0 0] -- the dY operands of the two final layers' weight-gradient jobs.
__global__ void __launch_bounds__(X_THREADS, 1)
field_backward_chain_def_kernel(const unsigned short *__restrict__ stream, long P, const float *__restrict__ xwg, const float *__restrict__ actbuf,
                                const uint32_t *__restrict__ bits, float *__restrict__ dact, float *__restrict__ g3, float *__restrict__ dw4)
{
    extern __shared__ __attribute__((aligned(16))) char lds_x[];
    Ctx cx;
    cx.stream = stream;
    cx.lds = lds_x;
    cx.buf = 0;
    cx.lane = threadIdx.x & 63;
    cx.h = cx.lane >> 5;
    cx.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = cx.h, col = cx.lane & 31;
    {
        float *zl = reinterpret_cast<float *>(lds_x + LDS_BIAS_BYTE_OFF);
        for (int i = threadIdx.x; i < BWC_ZERO_BYTES / 4; i += X_THREADS) zl[i] = 0.0f;
        cx.wrap_at = (uint32_t)DEF_HW;
        cx.wrap_to = 0u;
        cx.off = 0u;
        cx.prepare(CHD(D_HF), 0);
#pragma unroll
        for (int pc = 0; pc < (CHD(D_HF) + PIECE_HW - 1) / PIECE_HW; ++pc) cx.issue_piece(pc);
        __syncthreads();
    }
    const long ntiles = (P + X_PTS_PER_WG - 1) / X_PTS_PER_WG;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        cx.refresh_bias_base();
        asm volatile("" : "+s"(cx.off));
        long Pq = P;
        asm volatile("" : "+s"(Pq));
        St st;
        const long p_raw = tile * X_PTS_PER_WG + cx.wave * X_PTS_PER_WAVE + col;
        const long p = p_raw < P ? p_raw : P - 1;
        const uint32_t pl = (uint32_t)p;
        const StageCtx sc = make_stage(lds_x, cx.wave, cx.lane, tile, P);
        auto fill = [&](auto &e, int b, int c) {       // one sign word per q for the 128- and the 64-wide nets alike
            e.slope = 0.0f;
            const uint32_t *a = bits + (long)b * Pq + ((long)pl * 4 + h);
            e.mh[0] = a[0]; e.m2[0] = a[2]; e.mh[1] = 0u; e.m2[1] = 0u;
            e.base = dact + (long)c * Pq;
            e.sc = sc;
        };
        auto epw = [&](int b, int c) { BwdEp<true, 4, 128> e; fill(e, b, c); return e; };
        Blk hd_w[2], hd_x[2];
        {
            const f32x4 *r = reinterpret_cast<const f32x4 *>(xwg + p * 8);
            const f32x4 gx = r[0], gw = r[1];
            const float *dxp = actbuf + (long)act::DX * Pq + p * 16;
            const float d0 = dxp[0], d1 = dxp[1], d2 = dxp[2];
            const f32x4 t3 = f32x4{gx[0] * (1.0f - d0 * d0), gx[1] * (1.0f - d1 * d1), gx[2] * (1.0f - d2 * d2), 0.0f};     // x' = x + tanh(.) (models.py:304-305)
            const f32x4 tw = f32x4{gw[0], AMB_DIM > 1 ? gw[1] : 0.0f, 0.0f, 0.0f};
            const f32x4 z4 = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            head_block(h == 0 ? t3 : z4, z4, hd_x[0]);
            head_block(h == 0 ? tw : z4, z4, hd_w[0]);
            zero_block(hd_x[1]);
            zero_block(hd_w[1]);
            if (h == 0) {
                *reinterpret_cast<f32x4 *>(g3 + p * 4) = t3;
                *reinterpret_cast<f32x4 *>(dw4 + p * 4) = tw;
            }
        }
        {   // hyper sheet: dw -> dG5 -> ... -> dG0 (the 64-wide layers: two 32-row tiles)
            Blk A[2], B[2];
            auto mk = [&](int i) { BwdEp<true, 2, 64> e; fill(e, sbits::BD_HH + 4 * i, act::HH + 64 * i); return e; };
            auto e5 = mk(5);
            auto e4 = mk(4);
            dense_x<2, 0, 0, 2, CHD(D_H5), false>(cx, st, hd_w, nullptr, nullptr, A, 0, e5, NoEp{1.0f});
            auto e3 = mk(3);
            dense_x<2, 0, 0, 2, CHD(D_H4), true, 1>(cx, st, A, nullptr, nullptr, B, 0, e4, e5);
            auto e2 = mk(2);
            dense_x<2, 0, 0, 2, CHD(D_H3), true, 1>(cx, st, B, nullptr, nullptr, A, 0, e3, e4);
            auto e1 = mk(1);
            dense_x<2, 0, 0, 2, CHD(D_H2), true, 1>(cx, st, A, nullptr, nullptr, B, 0, e2, e3);
            auto e0 = mk(0);
            dense_x<2, 0, 0, 2, CHD(D_H1), true, 1>(cx, st, B, nullptr, nullptr, A, 0, e1, e2);
            dense_x<2, 0, 0, 2, CHD(D_WF), true, 1>(cx, st, A, nullptr, nullptr, B, 0, e0, e1);
            flush_x<1>(st, e0);
        }
        {   // warp field: dx' (1 - dx^2) -> dH5 -> ... -> dH0
            Blk A[4], B[4];
            auto e5 = epw(sbits::BD_WH + 4 * 5, act::WH + 128 * 5);
            auto e4 = epw(sbits::BD_WH + 4 * 4, act::WH + 128 * 4);
            dense_x<2, 0, 0, 4, CHD(D_W5), false>(cx, st, hd_x, nullptr, nullptr, A, 0, e5, NoEp{1.0f});
            auto e3 = epw(sbits::BD_WH + 4 * 3, act::WH + 128 * 3);
            dense_x<4, 0, 0, 4, CHD(D_W4), true, 3>(cx, st, A, nullptr, nullptr, B, 0, e4, e5);
            auto e2 = epw(sbits::BD_WH + 4 * 2, act::WH + 128 * 2);
            dense_x<4, 0, 0, 4, CHD(D_W3), true, 3>(cx, st, B, nullptr, nullptr, A, 0, e3, e4);
            auto e1 = epw(sbits::BD_WH + 4 * 1, act::WH + 128 * 1);
            dense_x<4, 0, 0, 4, CHD(D_W2), true, 3>(cx, st, A, nullptr, nullptr, B, 0, e2, e3);
            auto e0 = epw(sbits::BD_WH + 0, act::WH + 0);
            dense_x<4, 0, 0, 4, CHD(D_W1), true, 3>(cx, st, B, nullptr, nullptr, A, 0, e1, e2);
            dense_x<4, 0, 0, 4, CHD(D_HF), true, 3>(cx, st, A, nullptr, nullptr, B, 0, e0, e1);
            flush_x<3>(st, e0);
        }
    }
}
#endif      // SAHS_MODEL != 2

}  // namespace bwc
}  // namespace SAHS_NS

using namespace SAHS_NS;
using namespace SAHS_NS::bwc;

// halfwords of the transposed stream of `part` (1 deformation nets, 2 radiance nets of one level; 0 for a part the model does not have)
extern "C" long SAHS_SYM(sahs_bwd_chain_stream_hw)(int part) { return part == 1 ? DEF_HW : RAD_HW; }

extern "C" int SAHS_SYM(sahs_bwd_chain_pack_launch)(const float *flat, void *stream_out, int level, int part, hipStream_t stream)
{
    const long total = (part == 1 ? DEF_HW : RAD_HW) / 16;
    if (total <= 0) return (int)hipErrorInvalidValue;
    pack_bwd_stream_kernel<<<(unsigned)((total + 255) / 256), 256, 0, stream>>>(flat, reinterpret_cast<unsigned short *>(stream_out), level, part);
    return (int)hipGetLastError();
}

template <auto Kernel, class... A>
static int launch_chain(long P, int num_cu, hipStream_t stream, A... args)
{
    if (P <= 0) return 0;
    return sahs_launch_persistent<Kernel>((P + X_PTS_PER_WG - 1) / X_PTS_PER_WG, num_cu, X_THREADS, BWC_LDS_BYTES, stream, args...);
}

extern "C" int SAHS_SYM(sahs_bwd_chain_rad_launch)(const void *bstream, long P, const float *d_raw, const uint32_t *bits, float *dact, float *dgridf,
                                         float *din_a, float *din_b, int num_cu, hipStream_t stream)
{
    return launch_chain<field_backward_chain_rad_kernel>(P, num_cu, stream, reinterpret_cast<const unsigned short *>(bstream), P, d_raw, bits, dact,
                        dgridf, din_a, din_b);
}

#if SAHS_MODEL != 2
extern "C" int SAHS_SYM(sahs_bwd_chain_def_launch)(const void *bstream, long P, const float *xwg, const float *actbuf, const uint32_t *bits, float *dact,
                                         float *g3, float *dw4, int num_cu, hipStream_t stream)
{
    return launch_chain<field_backward_chain_def_kernel>(P, num_cu, stream, reinterpret_cast<const unsigned short *>(bstream), P, xwg, actbuf, bits,
                        dact, g3, dw4);
}
#endif
