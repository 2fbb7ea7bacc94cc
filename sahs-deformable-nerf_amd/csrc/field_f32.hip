// field_f32.hip -- the per-sample field (deformation MLPs + feature grid + radiance MLP), exact fp32.
//
// Replaces, for one level, the reference's run_network -> AudioFaceModel.forward chain
// (train_utils.py:9-50, models.py:514-528, modules.py:371-390 / 444-462 / 254-295, grid lookup
// models.py:346-365) including the point construction pts = ro + rd*z (train_utils.py:115,168).
// Input is the ray table and the per-ray depths; output is raw (N,S,16) = [rgb3, seg12, sigma].
// Nothing else touches HBM: the (P,18) point rows, the three positional encodings, the
// replicated conditioning vectors and every hidden activation of the reference (~50-100 KB per
// sample) never exist.
//
// Design (gfx950):
//  * one wave owns 16 sample points for the whole network.  v_mfma_f32_16x16x4_f32 computes
//    D[16 out-features x 16 points] += A[16 x 4] * B[4 x 16]; the D tile of layer l (lane (q,j):
//    features 4q..4q+3 of point j in its 4 registers) is exactly the B operand layout of layer
//    l+1 (lane (q,j) supplies k = feature 16b+4q+r at step r), so activations stay in VGPRs and
//    never visit LDS.  f32 MFMA is a k-ordered fmaf chain: results are exact fp32.
//  * weights are pre-packed in A-fragment order (pack.hip) and streamed L2 -> LDS in <=64 KB
//    chunks (<=32 KB in the activation-saving instances) with global_load_lds (no VGPR staging), double buffered, one barrier per chunk; all 8
//    waves of the workgroup (2 per SIMD: MFMA of one overlaps VALU/LDS of the other) consume the
//    same chunk, so each weight byte is fetched once per 128 points.
//  * persistent workgroups (one per CU) walk 128-point tiles; the weight stream simply wraps.
// Roofline: MFMA-bound (1.86 MFLOP per sample against ~100 B of HBM traffic).
#include <hip/hip_runtime.h>
#include "sahs_common.hpp"
#include "sahs_launchers.hpp"
#include "sahs_layout.hpp"
#include "f32_pipe.hpp"

namespace SAHS_NS {


// ---- positional encoding in B layout ----------------------------------------------------------
// feature f of positional_encoding(v[0:d], L, include_input=True): [v | sin(2^0 v) | cos(2^0 v) | ...]
// (nerf_helpers.py:322-349); f >= d+2dL is zero padding.
//
// sin/cos(2^k x) to ~1e-7 absolute, without a general-purpose range reduction: the octave scaling is a power
// of two, so the angle is reduced in REVOLUTIONS.  u = x/(2 pi) is formed once per coordinate as an unevaluated
// sum p + lo (error-free product with a two-term 1/(2 pi), ~48 bits); 2^k p and 2^k lo are exact, 2^k p - rint(2^k p)
// is exact, so the fraction f of a revolution carries only lo's error (<= 2^-48 * 2^k |u|).  Then the quadrant is
// peeled off and sin/cos(2 pi g), |g| <= 1/8, are the classic minimax polynomials on [-pi/4, pi/4] (1 ulp).
// The reference evaluates sin(fl(2^k x)) with SLEEF/libm (1 ulp): both are within rounding of the true value.
struct RevArg { float p, lo; };
__device__ __forceinline__ RevArg rev_arg(float x)
{
    const float C_HI = 0.15915494f;                 // fl(1/(2 pi))
    const float C_LO = 6.4206382e-09f;              // 1/(2 pi) - C_HI
    RevArg r;
    r.p = x * C_HI;
    r.lo = fmaf(x, C_LO, fmaf(x, C_HI, -r.p));
    return r;
}
// sin(2^k x + fn*pi/2) given rev_arg(x) and scale = 2^k
__device__ __forceinline__ float sin_octave(RevArg u, float scale, int fn)
{
    const float P = u.p * scale, Lo = u.lo * scale;                 // exact
    const float f = (P - rintf(P)) + Lo;                            // fraction of a revolution, [-1/2, 1/2]
    const float qf = rintf(4.0f * f);
    const float th = fmaf(qf, -0.25f, f) * 6.2831855f;              // |th| <= pi/4
    const float z = th * th;
    const float sp = fmaf(th * z, fmaf(fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f), th);
    const float cp = fmaf(z * z, fmaf(fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f), fmaf(z, -0.5f, 1.0f));
    const int m = ((int)qf + fn) & 3;                               // sin(th + m pi/2)
    const float v = (m & 1) ? cp : sp;
    return (m & 2) ? -v : v;
}

template <int D, int L, int NB, int INC = 1>   // INC: include_input (the raw coordinates come first)
__device__ __forceinline__ void pe_blocks(const float *v, int q, f32x4 *out)
{
    constexpr int D0 = INC ? D : 0;
    constexpr int W = D0 + 2 * D * L;
    // plain scalars, selected with ternaries: an array of structs indexed by the lane-dependent axis ends up in scratch
    const float v0 = v[0], v1 = v[D > 1 ? 1 : 0], v2 = v[D > 2 ? 2 : 0];
    const RevArg u0 = rev_arg(v0), u1 = rev_arg(v1), u2 = rev_arg(v2);
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int f = 16 * b + 4 * q + r;
            float val = 0.0f;
            if (f < D0) {
                val = (f == 0) ? v0 : ((f == 1) ? v1 : v2);
            } else if (f < W) {
                const int g = f - D0;
                const int k = g / (2 * D), rem = g % (2 * D);
                const int fn = rem / D, ax = rem % D;
                RevArg a;
                a.p = (ax == 0) ? u0.p : ((ax == 1) ? u1.p : u2.p);
                a.lo = (ax == 0) ? u0.lo : ((ax == 1) ? u1.lo : u2.lo);
                val = sin_octave(a, (float)(1 << k), fn);
            }
            out[b][r] = val;
        }
}

// ---- trilinear feature-grid lookup (models.py:346-365; ATen grid_sampler_3d, align_corners=True,
// zeros padding; x indexes W, y H, z D).  grid is channel-last [D][H][W][32]; this lane fetches
// channels 16b+4q..+3 (b = 0,1) = its B-layout share.
__device__ __forceinline__ void grid_blocks(const float *__restrict__ grid, float x, float y, float z, int q, f32x4 *out)
{
    const float R1 = (float)(G_RES - 1);
    const float ix = ((x + 1.0f) / 2.0f) * R1, iy = ((y + 1.0f) / 2.0f) * R1, iz = ((z + 1.0f) / 2.0f) * R1;
    const float fx = floorf(ix), fy = floorf(iy), fz = floorf(iz);
    const float x1 = fx + 1.0f, y1 = fy + 1.0f, z1 = fz + 1.0f;
    const float wx[2] = {x1 - ix, ix - fx}, wy[2] = {y1 - iy, iy - fy}, wz[2] = {z1 - iz, iz - fz};
    const bool ok = fx >= -1.0f && fx <= (float)G_RES && fy >= -1.0f && fy <= (float)G_RES && fz >= -1.0f && fz <= (float)G_RES;
    const int xi = ok ? (int)fx : -2, yi = ok ? (int)fy : -2, zi = ok ? (int)fz : -2;
    out[0] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    out[1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int n = 0; n < 8; ++n) {
        const int cx = xi + (n & 1), cy = yi + ((n >> 1) & 1), cz = zi + (n >> 2);
        const bool inb = cx >= 0 && cx < G_RES && cy >= 0 && cy < G_RES && cz >= 0 && cz < G_RES;
        const float wt = (wx[n & 1] * wy[(n >> 1) & 1]) * wz[n >> 2];
        const long vox = inb ? (((long)cz * G_RES + cy) * G_RES + cx) : 0;
        const f32x4 *g = reinterpret_cast<const f32x4 *>(grid + vox * D_GRID) + q;
        const f32x4 g0 = g[0], g1 = g[4];
        // branch-free (weight 0 for a corner outside the grid; x + 0 == x): guarded corners become eight dependent fetch round trips
        const float we = inb ? wt : 0.0f;
#pragma unroll
        for (int r = 0; r < 4; ++r) { out[0][r] = out[0][r] + g0[r] * we; out[1][r] = out[1][r] + g1[r] * we; }
    }
}

// the radiance trunk's input blocks [PE(x') | PE(w)] from a lane's stash {x'0 x'1 x'2 w0 w1}: they feed T0 and, re-injected, the skip layer T3A
__device__ __forceinline__ void trunk_encodings(const float *stash, int q, f32x4 *enc)
{
    const float xw[3] = {stash[0], stash[1], stash[2]}, amb[2] = {stash[3], stash[4]};
    pe_blocks<3, L_XYZ, KB_XYZ>(xw, q, enc);
#if SAHS_MODEL != 2
    pe_blocks<AMB_DIM, L_AMB, KB_AMB, AMB_INC>(amb, q, enc + KB_XYZ);
#else
    (void)amb;
#endif
}

// floats in one chunk of layer id under a chunk cap of `cap` floats (kProg.layer[].G is the 32 KB chunking: pack.hip's table)
constexpr int chunk_floats(int id, int cap) { return pick_G(kProg.layer[id].KB, kProg.layer[id].NT, cap) * kProg.layer[id].KB * 256; }
#define CHF(id) chunk_floats(id, CAP)   /* ... of the kernel instance it is used in */
// The chunk cap of an instance.  Without saved activations: 64 KB buffers, which halve the chunk boundaries of the 256-wide layers (a
// boundary = MFMA drain + barrier + one LDS round trip with nothing of the next chunk readable), and with them the pinned fragment
// pipeline of f32_pipe.hpp (a_ahead, a_pinned) -- which is what the 2 % per launch come from; the cap's own share measured 0.4 ms per
// W512 frame, 11-134 cycles per boundary (LAB_NOTES.md).  The saving instances keep 32 KB and the compiler's order: at 64 KB the
// whole-network one spills, and their counted closing waits (f32_pipe.hpp: stores_behind_last_piece) are derived for today's chunks.
constexpr int field_chunk_cap(bool save) { return save ? CHUNK_FLOATS_MAX : CHUNK_FLOATS_WIDE; }
// Whether an instance reads its tiles' biases ahead (f32_pipe.hpp: BIAS_AHEAD): the pinned ones, i.e. those without saved activations; the
// saving instances keep the step as it was.  SAHS_F32_BIAS_AHEAD / SAHS_F32_ENC_ONCE6: pricing builds (tools/ablate.py), one part at a time.
#if defined(SAHS_DIAG) && defined(SAHS_F32_BIAS_AHEAD)
constexpr bool field_bias_ahead(bool save) { return !save && (SAHS_F32_BIAS_AHEAD) != 0; }
#else
constexpr bool field_bias_ahead(bool save) { return !save; }
#endif
#if defined(SAHS_DIAG) && defined(SAHS_F32_ENC_ONCE6)
constexpr bool field_enc_once6() { return (SAHS_F32_ENC_ONCE6) != 0; }
#else
constexpr bool field_enc_once6() { return true; }
#endif

// SAVE: also store every layer's activations (sahs::act layout, 19 KB/sample) for field_bwd.hip
// MODE: which part of the per-sample network a launch evaluates.  The deformation nets (warp field, hyper sheet) are shared by the
// coarse and the fine level, and the fine pass's depths are sort(cat(coarse depths, new depths)) (train_utils.py:166): the reference
// evaluates the deformation of the coarse samples a second time in its fine pass.  Here the coarse launch (FIELD_ALL) also writes every
// sample's deformed point x' and ambient coordinate w to `xw`, a FIELD_DEFORM launch computes them for the new depths only, and the
// fine launch (FIELD_RADIANCE) reads them through the merge permutation `src` and runs only the radiance net: the same arithmetic on
// the same operands, hence bit-identical results, for 6 % fewer matrix instructions per frame.
//   xw: (rays, xw_row, 8) floats [x'0 x'1 x'2 w0 w1 . . .]; a launch over (N, S) depths owns columns xw_col0 .. xw_col0 + S - 1
//   src: (N, S) int32, FIELD_RADIANCE only: column of xw holding sample s of the ray
//
// The inference render also splits the radiance evaluation at fc_alpha (sparse branches).  The composite gives a sample whose sigma + noise
// is <= 0 the weight exactly 0 (and replaces the last sample's channels by the background prior), so its colour and seg logits are never
// used.  The dense modes (FIELD_ALL, FIELD_DEFORM, FIELD_RADIANCE) evaluate every layer of their part for every sample; the fused sparse
// modes run the branches L_D0B..L_SEG for the LIVE samples only, in the same launch:
//   FIELD_ALL_FUSED = FIELD_ALL with sparse branches, FIELD_RADIANCE_FUSED = FIELD_RADIANCE with sparse branches
//  * the ring.  Every persistent workgroup keeps a private FIFO ring of records (feat, x' and the sample index of a live sample) in the
//    workspace.  A tile runs the network up to L_ALPHA, stores the FINAL tile as it stands there (rows 0..14 the fc_rgb / fc_seg biases,
//    row 15 sigma) as the samples' raw rows and appends its live samples to the ring (slots from per-wave live counts through LDS: no
//    global atomic).  When the ring held a tile's worth (128) at the START of the tile, the iteration goes on through L_D0B..L_SEG over
//    the 128 oldest records instead of wrapping at L_D0B, and overwrites those samples' raw rows.  All of those records were stored during
//    earlier tiles of the same workgroup (same CU, workgroup barriers in between), so the loads are disjoint from this tile's stores.
//    Columns of an MFMA tile are independent, so a live sample's row has the bits of the dense evaluation whatever slot it lands in.
//  * the drain.  After its last tile the workgroup empties the ring in branch-only iterations (the last one partial: lanes past the count
//    redo the last record and store nothing).
//  * the tile rotation: which tile an iteration takes (fused_tile below), so that a workgroup's share of live samples evens out.
// The mode numbers are part of the instances' mangled names (build.py: NO_SCRATCH, tools/compare_isa.py); 3..5 were the trunk-launch +
// branch-launch form this one replaced (LAB_NOTES.md).
enum { FIELD_ALL = 0, FIELD_DEFORM = 1, FIELD_RADIANCE = 2, FIELD_ALL_FUSED = 6, FIELD_RADIANCE_FUSED = 7 };
// Ring slots per workgroup of the fused instances.  The branch decision is taken from the count carried INTO a tile (>= 128), so that count
// is at most 255 when a tile starts, a tile adds at most 128, and 383 slots can never overflow; a workgroup of T tiles appends at most
// 128 T records in all.  Workgroup g's ring starts at the sum of its predecessors' slots.
constexpr int SPARSE_RING = 512;
static_assert(SPARSE_RING >= 255 + 128 && SPARSE_RING % 128 == 0, "a ring holds the carried count plus one tile");
__host__ __device__ constexpr long sparse_ring_slots(long tiles) { return tiles * F32_PTS_PER_WG < SPARSE_RING ? tiles * F32_PTS_PER_WG : SPARSE_RING; }
// slots in front of workgroup g's ring (g == grid: all of them) when `grid` workgroups share ntiles tiles (every workgroup one tile of each
// full row of `grid` tiles, workgroups g < ntiles % grid one more).  With grid = min(ntiles, CUs) the total never goes down as ntiles goes up
// (one more tile is 128 slots more, or one workgroup's step from slots(t) to slots(t + 1) >= slots(t)), so a workspace sized for the
// larger pass of a render holds the rings of the smaller one
__host__ __device__ constexpr long sparse_ring_base(long ntiles, long grid, long g)
{
    const long tlo = ntiles / grid, rem = ntiles % grid;
    return g * sparse_ring_slots(tlo) + (g < rem ? g : rem) * (sparse_ring_slots(tlo + 1) - sparse_ring_slots(tlo));
}
constexpr int LDS_RING_FLOATS = 16;      // fused instances: the waves' live counts of a tile, behind the stash
constexpr bool field_mode_fused(int mode) { return mode == 6 || mode == 7; }      // (FIELD_ALL_FUSED, FIELD_RADIANCE_FUSED)
// dynamic LDS of an instance: two chunk buffers of its cap, biases, stash (+ ring words)
constexpr int field_lds_floats(bool save, int mode) { return (save ? LdsMap<field_chunk_cap(true)>::TOTAL_FLOATS : LdsMap<field_chunk_cap(false)>::TOTAL_FLOATS) + (field_mode_fused(mode) ? LDS_RING_FLOATS : 0); }
static_assert(field_lds_floats(false, 7) * 4 <= 160 * 1024 && field_lds_floats(true, 0) * 4 <= 160 * 1024, "LDS budget of the largest instance of each cap");
// The record workspace of the fused instances (the kernel's argument block; the launcher fills it from one allocation).  Records sit in
// groups of 16 slots (one wave of a branch pass); a group's feat is laid out [k-block 16][lane 64][4] like a weight fragment, so a branch
// pass loads it with whole 1-KB wave transactions.
struct SparseArgs {
    const float *noise;      // the composite's noise of these samples (N, S), or null: part of what decides which samples are live
    unsigned int *count;     // head words: [0] += the pass's live count (zeroed by the caller), [1] = 1 once a sparse pass ran
    f32x4 *hdr;              // [cap] {x'0, x'1, x'2, sample index (int bits)}
    f32x4 *feat;             // [cap / 16][16][64]
    unsigned int cap;        // slots (a multiple of 128, at least the rings of the launch: sparse_ring_base(ntiles, grid, grid))
    int has_bg;              // a background prior replaces the last sample's channels
};
constexpr long SPARSE_HEAD_BYTES = 256, SPARSE_RECORD_BYTES = 16 + 16 * 16 * 4;
template <bool SAVE, int MODE>
__global__ void __launch_bounds__(F32_THREADS, 2)
field_forward_f32_kernel(const float *__restrict__ packed, const float *__restrict__ frame, int level, long P, int S,
                         const float *__restrict__ rays, int ray_stride, const float *__restrict__ zvals,
                         float *__restrict__ raw, float *__restrict__ dbg, float *__restrict__ actbuf,
                         float *__restrict__ xw, int xw_row, int xw_col0, const int *__restrict__ src, uint32_t *__restrict__ bits, SparseArgs sp)
{
#if SAHS_MODEL == 2
    static_assert(MODE == FIELD_ALL || MODE == FIELD_ALL_FUSED, "this model has no deformation nets to split off");
#endif
    constexpr bool FUSED = MODE == FIELD_ALL_FUSED || MODE == FIELD_RADIANCE_FUSED;      // sparse branches: trunk, ring append and branch pass in one launch
    constexpr bool XW_IN = MODE == FIELD_RADIANCE || MODE == FIELD_RADIANCE_FUSED;       // x', w come from xw through src
    static_assert(!(SAVE && FUSED), "the sparse branches are an inference path");
    constexpr int CAP = field_chunk_cap(SAVE);
    typedef LdsMap<CAP> Lds;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    CtxT<CAP, field_bias_ahead(SAVE)> cx;
    cx.stream = packed + PACK_STREAM_OFF + (long)level * STREAM_FLOATS;
    cx.lds = lds;
    cx.buf = 1;                       // so that the first chunk lands in buffer 0
    cx.lane = threadIdx.x & 63;
    cx.q = cx.lane >> 4;
    cx.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr const Layer *Ly = kProg.layer;
    constexpr int L_START = XW_IN ? L_T0 : L_FIRST;      // first layer of this launch's walk through the stream
    cx.wrap_to = (uint32_t)Ly[L_START].stream_off;
    cx.wrap_at = (MODE == FIELD_DEFORM) ? (uint32_t)Ly[L_T0].stream_off : (FUSED ? (uint32_t)Ly[L_D0B].stream_off : (uint32_t)STREAM_FLOATS);      // (FUSED: chosen per tile)
    cx.off = cx.wrap_to;
    const float *grid = packed + PACK_GRID_OFF;

    {   // per-level biases (static + folded conditioning) -> LDS, first weight chunk -> buffer 0
        const float *bsrc = frame + FRAME_BIAS_OFF + level * BIAS_FLOATS;
        for (int i = threadIdx.x; i < BIAS_FLOATS; i += F32_THREADS) lds[Lds::BIAS_OFF + i] = bsrc[i];
        cx.begin_chunk(CHF(L_START));
#pragma unroll
        for (int pc = 0; pc < (CHF(L_START) + PIECE_FLOATS - 1) / PIECE_FLOATS; ++pc) cx.issue_piece(pc);
        cx.end_chunk();
    }

    const long ntiles = (P + F32_PTS_PER_WG - 1) / F32_PTS_PER_WG;
    // FIELD_RADIANCE_FUSED: the x', w row of the workgroup's NEXT tile is fetched while this one multiplies (its src entry at the start of
    // the tile, the dependent xw row behind T2), so a tile no longer starts with two dependent trips to HBM while the matrix pipe idles.
    // The addresses use the same P - 1 clamp; a workgroup with no next tile issues nothing.
    constexpr bool XW_AHEAD = MODE == FIELD_RADIANCE_FUSED;
    f32x4 nx_a = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float nx_w1 = 0.0f;
    int nx_src = 0;
    // (FUSED) the workgroup's ring: uniform values, the same in every wave (they come from kernel arguments and from LDS words read behind a
    // workgroup barrier), so every barrier below sits under workgroup-uniform control flow
    uint32_t r_cnt = 0u, r_head = 0u, r_total = 0u, r_cap = 0u, r_base = 0u;
    uint32_t r_it = 0u, r_tiles = 0u;      // iterations so far, this workgroup's tiles (32-bit: a 64-bit signed compare is a vector instruction, and what hangs on it leaves the scalar registers)
    if constexpr (FUSED) {
        r_tiles = (uint32_t)__builtin_amdgcn_readfirstlane((int)(ntiles / gridDim.x + ((long)blockIdx.x < ntiles % gridDim.x ? 1 : 0)));
        r_cap = (uint32_t)sparse_ring_slots(r_tiles);
        r_base = (uint32_t)__builtin_amdgcn_readfirstlane((int)sparse_ring_base(ntiles, gridDim.x, blockIdx.x));
    }
    // (FUSED) which tile an iteration takes.  A workgroup's time depends on how many of ITS samples are live, and neighbouring rays are
    // alike: with the fixed stride workgroup g would take the same image columns in every row of tiles.  So in the k-th full row of
    // gridDim.x tiles workgroup g takes tile (g + 61 k) mod gridDim.x of that row -- a rotation, so every tile is still taken exactly once
    // and the tiles running at one time are neighbours in memory as before -- and the leftover row keeps the fixed stride (workgroup g has
    // a tile there iff g < ntiles % gridDim.x: what r_tiles and r_base count on).
    const uint32_t r_rows = FUSED ? (uint32_t)__builtin_amdgcn_readfirstlane((int)(ntiles / gridDim.x)) : 0u;
    auto fused_tile = [&](uint32_t k) -> long {
        const uint32_t col = k < r_rows ? (blockIdx.x + 61u * k) % gridDim.x : blockIdx.x;
        return (long)k * gridDim.x + col;
    };
    for (long tile_it = blockIdx.x; FUSED || tile_it < ntiles; tile_it += gridDim.x, ++r_it) {
        const long tile = FUSED ? fused_tile(r_it) : tile_it;
        // (FUSED) has_tile: the iteration runs a trunk tile; do_branch: it ends in a branch pass over the ring's oldest records.  Past the
        // last tile the iterations are branch passes only, until the ring is empty.
        bool has_tile = true, do_branch = false;
        uint32_t b_valid = 0u;      // records of this iteration's branch pass
        if constexpr (FUSED) {
            has_tile = r_it < r_tiles;
            do_branch = has_tile ? r_cnt >= (uint32_t)F32_PTS_PER_WG : r_cnt > 0u;
            if (!has_tile && !do_branch) break;
            b_valid = r_cnt < (uint32_t)F32_PTS_PER_WG ? r_cnt : (uint32_t)F32_PTS_PER_WG;
            if (has_tile) {      // known before L_ALPHA prefetches what follows it: on through the branches, or back to the first layer
                cx.wrap_at = do_branch ? (uint32_t)STREAM_FLOATS : (uint32_t)Ly[L_D0B].stream_off;
            } else {             // drain: the chunk in LDS is the first layer's; start the stream again at L_D0B (once per drain pass, at most 4 per launch)
                cx.off = (uint32_t)Ly[L_D0B].stream_off;
                cx.wrap_at = (uint32_t)STREAM_FLOATS;
                cx.begin_chunk(CHF(L_D0B));
#pragma unroll
                for (int pc = 0; pc < (CHF(L_D0B) + PIECE_FLOATS - 1) / PIECE_FLOATS; ++pc) cx.issue_piece(pc);
                cx.end_chunk();
            }
        }
        cx.refresh();
        // (a tile of the 4-layer-trunk models that stops behind fc_alpha has no rolled layer loop, so the stream offset of every chunk is the same constant
        // in every tile and LICM precomputes all ~100 LDS-DMA source addresses outside the persistent loop -- a kilobyte of scratch per
        // lane -- unless the offset is opaque per tile; likewise the encodings' per-lane octave selectors and the lane quarter.  At the 64 KB
        // cap the dense instances of those models need the same: without it NeRFaceModel's <false,0> and <false,2> sit at 256 registers and spill)
        int q_tile = cx.q;
        if constexpr (FUSED || (!SAVE && TR_LAYERS == 4)) { asm volatile("" : "+s"(cx.off)); asm volatile("" : "+v"(q_tile)); }
        const int q = q_tile;
        const long p_raw = tile * F32_PTS_PER_WG + cx.wave * F32_PTS_PER_WAVE + (cx.lane & 15);
        const long p = p_raw < P ? p_raw : P - 1;
        // x' (3) and w (2) are parked in LDS between their uses; the ray direction is re-read where needed: values that stay
        // live across the 256-wide layers get spilled to scratch, and a scratch reload drains the LDS-DMA prefetch (vmcnt).
        float *stash = lds + Lds::STASH_OFF + (cx.wave * F32_PTS_PER_WAVE + (cx.lane & 15)) * STASH_FLOATS;
        const bool dump = MODE == FIELD_ALL && dbg != nullptr && q == 0 && p_raw < P;   // lanes holding feature 0 of tile 0
        float *dsl = dbg + p * DBG_STRIDE;
        // saved activations are one dense [P x width] array per layer (array at column c of the act:: table starts at c * P):
        // this lane's slot in its sample's row of array (c, w)
        const bool sv_on = SAVE && p_raw < P;
        // (the plane bases actbuf + c * P are loop-invariant: unless P is opaque per tile the compiler hoists all ~40 of them out of the
        // persistent loop and spills them -- 176 bytes of scratch whose reloads drain the LDS-DMA prefetch)
        long Psv = P;
        if constexpr (SAVE) asm volatile("" : "+s"(Psv));
#define SVP(c, w) (actbuf + (long)(c) * Psv + p * (long)(w) + 4 * q)
#define SV(c, w) SVP(c, w)      // (a layer's tile stores are unconditional: lanes past the end redo sample P - 1 and store the same values again -- f32_pipe.hpp: kStores)
        // sign-bit planes (sbits): this lane's NW = w / 128 (at least 1) words of plane b; a whole-network save holds [deformation | radiance] planes
        const bool sb_on = sv_on && bits != nullptr;
        uint32_t *const bits_r = bits + (MODE == FIELD_ALL ? (long)sbits::BD_WORDS * Psv : 0L);
        const uint32_t sb_lane = (uint32_t)(p * 4 + q);      // (a uniform plane base + a 32-bit lane offset: one live register, not a pointer pair)
#define SBD(b, w) (sb_on ? bits + (long)(b) * Psv + sb_lane * (uint32_t)((w) >= 128 ? (w) / 128 : 1) : nullptr)
#define SBR(b, w) (sb_on ? bits_r + (long)(b) * Psv + sb_lane * (uint32_t)((w) >= 128 ? (w) / 128 : 1) : nullptr)
        float x[3] = {0.0f, 0.0f, 0.0f};
        long smp = p;            // the sample of this lane's point: its ray is smp / S, its raw row smp
        if constexpr (!XW_IN) {
            if (!FUSED || has_tile) {
            const float *rp = rays + (p / S) * ray_stride;
            const float z = zvals[p];
#pragma unroll
            for (int i = 0; i < 3; ++i) x[i] = rp[i] + rp[3 + i] * z;          // train_utils.py:115
            }
        } else if constexpr (XW_AHEAD) {
            if (q == 0 && has_tile) {
                if (r_it == 0u) {      // the workgroup's first tile: nothing was fetched ahead
                    const float *row = xw + ((p / S) * (long)xw_row + src[p]) * 8;
                    nx_a = *reinterpret_cast<const f32x4 *>(row);
                    nx_w1 = row[4];
                }
                stash[0] = nx_a[0]; stash[1] = nx_a[1]; stash[2] = nx_a[2]; stash[3] = nx_a[3]; stash[4] = nx_w1;
            }
        } else if (q == 0) {     // (XW_IN) x', w of this sample were computed by the coarse or the deformation launch: fetch through the merge permutation
            const float *row = xw + ((p / S) * (long)xw_row + src[p]) * 8;
            const f32x4 a = *reinterpret_cast<const f32x4 *>(row);
            stash[0] = a[0]; stash[1] = a[1]; stash[2] = a[2]; stash[3] = a[3]; stash[4] = row[4];
            if (sv_on) { float *d = SVP(act::XW, 16); d[0] = a[0]; d[1] = a[1]; d[2] = a[2]; }   // the grid backward reads x'
        }
        // (XW_AHEAD) this lane's sample of the workgroup's next tile
        const bool has_next = XW_AHEAD && r_it + 1u < r_tiles;
        const long pn_raw = fused_tile(r_it + 1u) * F32_PTS_PER_WG + cx.wave * F32_PTS_PER_WAVE + (cx.lane & 15);
        const long p_next = pn_raw < P ? pn_raw : P - 1;
        if constexpr (XW_AHEAD) {
            if (has_next && q == 0) nx_src = src[p_next];
        }
        // (FUSED) the header of this lane's record of the branch pass, fetched most of a trunk ahead: its sample index is what the raw row and
        // the ray direction are addressed with.  Lanes past the count take the last record (and store nothing).  The youngest of the 128
        // records may be of the previous tile, stored by another wave, so the load sits behind the first chunk barrier of this iteration: a
        // drain pass has had the one of its stream restart, a tile issues it behind T0.
        f32x4 b_hdr = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        uint32_t b_slot = 0u;
        if constexpr (FUSED) {
            if (do_branch) {
                const uint32_t j = (uint32_t)(cx.wave * F32_PTS_PER_WAVE + (cx.lane & 15));
                b_slot = r_base + r_head + (j < b_valid ? j : b_valid - 1u);      // (r_head is a multiple of 128, as r_cap is: a pass never straddles the ring's end)
                if (!has_tile) b_hdr = sp.hdr[b_slot];
            }
        }
        if constexpr (!XW_IN) {
        if (!FUSED || has_tile) {
#if SAHS_MODEL == 2
        // no deformation nets (use_warp False, use_ambient False): the template is queried at the raw point (models.py:316-327)
        if (q == 0) {
            stash[0] = x[0]; stash[1] = x[1]; stash[2] = x[2]; stash[3] = 0.0f; stash[4] = 0.0f;
            if (sv_on) { float *d = SVP(act::XW, 16); d[0] = x[0]; d[1] = x[1]; d[2] = x[2]; }   // the grid backward reads it
        }
#else
        f32x4 pe_x[KB_XYZ];
        {
            pe_blocks<3, L_XYZ, KB_XYZ>(x, q, pe_x);
            if (sv_on) {
#pragma unroll
                for (int b = 0; b < KB_XYZ; ++b) *reinterpret_cast<f32x4 *>(SVP(act::E, 16 * KB_XYZ) + 16 * b) = pe_x[b];
            }
        }
        // ---- warp field: dx = tanh(MLP) (modules.py:371-390) ----
        {
            f32x4 h[8], hn[8];
            dense_sv<SAVE, KB_XYZ, 0, 8, CHF(L_W1)>(cx, pe_x, nullptr, h, Ly[L_W0].bias_off, false, 0.0f, SV(act::WH, 128), SBD(sbits::BD_WH + 4 * (0), 128));
            // W1..W3; the chunk after each is W2, W3, W4B.  One rolled loop where those have the same size (AudioFaceModel at the 32 KB cap; at 64 KB a
            // 128 x 128 layer is one 64 KB chunk, W4B's stays 32 KB, and W3 is spelled out)
            constexpr int W_ROLLED = (CHF(L_W4B) == CHF(L_W2)) ? 3 : 2;
#pragma unroll 1
            for (int l = 0; l < W_ROLLED; ++l) {
                dense_sv<SAVE, 8, 0, 8, CHF(L_W2)>(cx, h, nullptr, hn, Ly[L_W1].bias_off + 128 * l, false, 0.0f, SV(act::WH + 128 * (l + 1), 128), SBD(sbits::BD_WH + 4 * ((l + 1)), 128));
#pragma unroll
                for (int i = 0; i < 8; ++i) h[i] = hn[i];
            }
            if (W_ROLLED == 2) {
                dense_sv<SAVE, 8, 0, 8, CHF(L_W4B)>(cx, h, nullptr, hn, Ly[L_W3].bias_off, false, 0.0f, SV(act::WH + 128 * 3, 128), SBD(sbits::BD_WH + 4 * (3), 128));
#pragma unroll
                for (int i = 0; i < 8; ++i) h[i] = hn[i];
            }
            dense<KB_XYZ, 0, 8, CHF(L_W4A)>(cx, pe_x, nullptr, hn, Ly[L_W4B].bias_off, false, 1.0f);
            dense_sv<SAVE, 8, 0, 8, CHF(L_W5)>(cx, h, nullptr, hn, 0, true, 0.0f, SV(act::WH + 4 * 128, 128), SBD(sbits::BD_WH + 4 * (4), 128));
            dense_sv<SAVE, 8, 0, 8, CHF(L_WF)>(cx, hn, nullptr, h, Ly[L_W5].bias_off, false, 0.0f, SV(act::WH + 5 * 128, 128), SBD(sbits::BD_WH + 4 * (5), 128));
            f32x4 o[1];
            dense<8, 0, 1, CHF(L_H0)>(cx, h, nullptr, o, Ly[L_WF].bias_off, false, 1.0f);
            if (q == 0) {
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const float dxv = tanhf(o[0][i]);
                    stash[i] = x[i] + dxv;                                            // models.py:305 (rows 0..2 live in lane quarter 0)
                    if (sv_on) { SVP(act::DX, 16)[i] = dxv; SVP(act::XW, 16)[i] = x[i] + dxv; }
                }
            }
        }
        // ---- hyper sheet: ambient w (modules.py:444-462) ----
        {
            f32x4 h[4], hn[4];
            dense_sv<SAVE, KB_XYZ, 0, 4, CHF(L_H1)>(cx, pe_x, nullptr, h, Ly[L_H0].bias_off, false, 0.0f, SV(act::HH, 64), SBD(sbits::BD_HH + 4 * (0), 64));
            constexpr int H_ROLLED = (CHF(L_H4B) == CHF(L_H2)) ? 3 : 2;   // H1..H3 (next chunks: H2, H3, H4B)
#pragma unroll 1
            for (int l = 0; l < H_ROLLED; ++l) {
                dense_sv<SAVE, 4, 0, 4, CHF(L_H2)>(cx, h, nullptr, hn, Ly[L_H1].bias_off + 64 * l, false, 0.0f, SV(act::HH + 64 * (l + 1), 64), SBD(sbits::BD_HH + 4 * ((l + 1)), 64));
#pragma unroll
                for (int i = 0; i < 4; ++i) h[i] = hn[i];
            }
            if (H_ROLLED == 2) {
                dense_sv<SAVE, 4, 0, 4, CHF(L_H4B)>(cx, h, nullptr, hn, Ly[L_H3].bias_off, false, 0.0f, SV(act::HH + 64 * 3, 64), SBD(sbits::BD_HH + 4 * (3), 64));
#pragma unroll
                for (int i = 0; i < 4; ++i) h[i] = hn[i];
            }
            dense<KB_XYZ, 0, 4, CHF(L_H4A)>(cx, pe_x, nullptr, hn, Ly[L_H4B].bias_off, false, 1.0f);
            dense_sv<SAVE, 4, 0, 4, CHF(L_H5)>(cx, h, nullptr, hn, 0, true, 0.0f, SV(act::HH + 4 * 64, 64), SBD(sbits::BD_HH + 4 * (4), 64));
            dense_sv<SAVE, 4, 0, 4, CHF(L_HF)>(cx, hn, nullptr, h, Ly[L_H5].bias_off, false, 0.0f, SV(act::HH + 5 * 64, 64), SBD(sbits::BD_HH + 4 * (5), 64));
            f32x4 o[1];
            dense<4, 0, 1, (MODE == FIELD_DEFORM ? CHF(L_FIRST) : CHF(L_T0))>(cx, h, nullptr, o, Ly[L_HF].bias_off, false, 1.0f);
            if (q == 0) {      // rows 0..AMB_DIM-1 of the one output tile
                stash[3] = o[0][0]; stash[4] = (AMB_DIM > 1) ? o[0][1] : 0.0f;
                if (sv_on) { SVP(act::AW, 16)[0] = o[0][0]; SVP(act::AW, 16)[1] = stash[4]; }
            }
        }
#endif
        if (xw != nullptr && q == 0 && p_raw < P) {   // hand x', w to the fine pass (the lane that wrote the stash reads it back: no barrier needed)
            float *row = xw + ((p / S) * (long)xw_row + xw_col0 + (p % S)) * 8;
            *reinterpret_cast<f32x4 *>(row) = f32x4{stash[0], stash[1], stash[2], stash[3]};
            row[4] = stash[4];
        }
        }
        }   // !XW_IN
        if constexpr (MODE == FIELD_DEFORM) continue;      // the stream has wrapped to the warp field's first layer
        __builtin_amdgcn_wave_barrier();
        if (dump) { dsl[0] = stash[0] - x[0]; dsl[1] = stash[1] - x[1]; dsl[2] = stash[2] - x[2]; dsl[3] = stash[3]; dsl[4] = stash[4]; }

        // ---- radiance trunk (modules.py:254-275) ----
        f32x4 fin[1];      // FINAL tile: raw[4q..4q+3] of this lane's point
        f32x4 feat[16];
        if (!FUSED || has_tile) {
            f32x4 h[16];
            if constexpr (FUSED) {      // (T0..T3A spelled apart from the dense instances' below: one body for both compiles the dense ones differently)
                // PE(x'), PE(w) feed T0 and, re-injected, the skip layer T3A.  The trunk part of a fused tile holds no ray direction or grid
                // blocks, so the 24 registers can stay live through T1, T2 and the encodings be built once per tile (a build is ~1,000 VALU
                // instructions per wave, and all eight waves run it at the same moment, the matrix pipe idle).  Measured (W512 frame,
                // LAB_NOTES.md): -1.3 % of the launch for the fine trunk; for FIELD_ALL_FUSED, whose tile also runs the deformation nets,
                // -0.8 % of its trunk was below that launch's own spread, but on the frame it is -3.0 ms, apart from the parent's series.
                constexpr bool ENC_ONCE = MODE == FIELD_RADIANCE_FUSED || field_enc_once6();
                f32x4 in_tr[KB_XYZ + KB_AMB];
                auto build_enc = [&]() { trunk_encodings(stash, q, in_tr); };
                build_enc();
                dense<KB_XYZ, KB_AMB, 16, CHF(L_T1)>(cx, in_tr, in_tr + KB_XYZ, h, Ly[L_T0].bias_off, false, 0.01f);
                if (do_branch) b_hdr = sp.hdr[b_slot];
                dense<16, 0, 16, CHF(L_T2)>(cx, h, nullptr, feat, Ly[L_T1].bias_off, false, 0.01f);
#pragma unroll
                for (int i = 0; i < 16; ++i) h[i] = feat[i];
                dense<16, 0, 16, CHF(L_T3B)>(cx, h, nullptr, feat, Ly[L_T2].bias_off, false, 0.01f);
#pragma unroll
                for (int i = 0; i < 16; ++i) h[i] = feat[i];
                if constexpr (XW_AHEAD) {
                    if (has_next && q == 0) {
                        const float *row = xw + ((p_next / S) * (long)xw_row + nx_src) * 8;
                        nx_a = *reinterpret_cast<const f32x4 *>(row);
                        nx_w1 = row[4];
                    }
                }
                if constexpr (!ENC_ONCE) build_enc();
                dense<KB_XYZ, KB_AMB, 16, CHF(L_T3A)>(cx, in_tr, in_tr + KB_XYZ, feat, Ly[L_T3B].bias_off, false, 1.0f);
            } else {
            {
                f32x4 in_tr[KB_XYZ + KB_AMB];
                trunk_encodings(stash, q, in_tr);
                if (sv_on) {
#pragma unroll
                    for (int b = 0; b < KB_XYZ + KB_AMB; ++b)
                        *reinterpret_cast<f32x4 *>(b < KB_XYZ ? SVP(act::PEX, 16 * KB_XYZ) + 16 * b : SVP(act::PEW, 16 * KB_AMB) + 16 * (b - KB_XYZ)) = in_tr[b];
                }
                dense_sv<SAVE, KB_XYZ, KB_AMB, 16, CHF(L_T1)>(cx, in_tr, in_tr + KB_XYZ, h, Ly[L_T0].bias_off, false, 0.01f, SV(act::T, 256), SBR(sbits::BR_T + 8 * (0), 256));
            }
            if (dump) dsl[5] = h[0][0];
            dense_sv<SAVE, 16, 0, 16, CHF(L_T2)>(cx, h, nullptr, feat, Ly[L_T1].bias_off, false, 0.01f, SV(act::T + 256, 256), SBR(sbits::BR_T + 8 * (1), 256));
            if (dump) dsl[6] = feat[0][0];
#pragma unroll
            for (int i = 0; i < 16; ++i) h[i] = feat[i];
            dense_sv<SAVE, 16, 0, 16, CHF(L_T3B)>(cx, h, nullptr, feat, Ly[L_T2].bias_off, false, 0.01f, SV(act::T + 512, 256), SBR(sbits::BR_T + 8 * (2), 256));
            if (dump) dsl[7] = feat[0][0];
#pragma unroll
            for (int i = 0; i < 16; ++i) h[i] = feat[i];
            {   // skip layer: the re-injected encoding is rebuilt here instead of staying live (24 VGPRs) through T1, T2 -- registers the dense
                // instances (237-245 VGPRs) do not have; the fine trunk above does, and builds it once
                f32x4 in_tr[KB_XYZ + KB_AMB];
                trunk_encodings(stash, q, in_tr);
                dense<KB_XYZ, KB_AMB, 16, CHF(L_T3A)>(cx, in_tr, in_tr + KB_XYZ, feat, Ly[L_T3B].bias_off, false, 1.0f);
            }
            }
#if SAHS_MODEL == 0
            dense_sv<SAVE, 16, 0, 16, CHF(L_T4)>(cx, h, nullptr, feat, 0, true, 0.01f, SV(act::T + 768, 256), SBR(sbits::BR_T + 8 * (3), 256));
#else           // 4-layer trunk: the skip layer is the last one, fc_feat follows
            dense_sv<SAVE, 16, 0, 16, CHF(L_FEAT)>(cx, h, nullptr, feat, 0, true, 0.01f, SV(act::T + 768, 256), SBR(sbits::BR_T + 8 * (3), 256));
#endif
            if (dump) dsl[8] = feat[0][0];
#pragma unroll
            for (int i = 0; i < 16; ++i) h[i] = feat[i];
#if SAHS_MODEL == 0
#pragma unroll 1
            for (int l = 4; l <= 7; ++l) {     // T4..T7 (next chunks: T5, T6, T7, FEAT, all of one size: the cap)
                dense_sv<SAVE, 16, 0, 16, CHF(L_T5)>(cx, h, nullptr, feat, Ly[L_T4].bias_off + 256 * (l - 4), false, 0.01f, SV(act::T + 256 * l, 256), SBR(sbits::BR_T + 8 * (l), 256));
                if (dump) dsl[5 + l] = feat[0][0];
#pragma unroll
                for (int i = 0; i < 16; ++i) h[i] = feat[i];
            }
#endif
            dense_sv<SAVE, 16, 0, 16, CHF(L_ALPHA)>(cx, h, nullptr, feat, Ly[L_FEAT].bias_off, false, 1.0f, SV(act::FEAT, 256));
            if (dump) dsl[13] = feat[0][0];
        }
        // fc_alpha -> FINAL tile.  What it prefetches: the branches' first chunk, or the first layer's when a fused tile wraps behind it (a
        // uniform two-way copy of this one-tile layer: NEXT is a compile-time size).  (A block of its own: inside the trunk's, the fused
        // instances compile differently.)
        if (!FUSED || has_tile) {
            if (FUSED && !do_branch) dense<16, 0, 1, CHF(L_START)>(cx, feat, nullptr, fin, Ly[L_ALPHA].bias_off, false, 1.0f);
            else dense<16, 0, 1, CHF(L_D0B)>(cx, feat, nullptr, fin, Ly[L_ALPHA].bias_off, false, 1.0f);
        }
        if constexpr (FUSED) {
            if (has_tile) {
                if (p_raw < P) *reinterpret_cast<f32x4 *>(raw + p * D_RAW + 4 * q) = fin[0];
                // live: the composite will give the sample a weight that can be non-zero (render_ops.hip: sg = max(sigma + noise, 0), the same
                // float expression; the last sample of a ray always has a weight, but with a background prior its channels are replaced)
                const long ray = p / S;
                const bool last = (p - ray * S) == S - 1;
                const float sg = fin[0][3] + (sp.noise != nullptr ? sp.noise[p] : 0.0f);      // sigma: row 15 = value 3 of the q == 3 lanes
                const bool live = q == 3 && p_raw < P && (last ? sp.has_bg == 0 : sg > 0.0f);
                const uint32_t mask = (uint32_t)(__ballot(live) >> 48);      // bit j: column j of this wave's 16 samples
                // slots: the waves' live counts through LDS (read again only after the many chunk barriers of the next tile)
                uint32_t *cnts = reinterpret_cast<uint32_t *>(lds + Lds::TOTAL_FLOATS);
                if (cx.lane == 0) cnts[cx.wave] = (uint32_t)__popc(mask);
                __syncthreads();
                uint32_t before = 0u, all = 0u;
#pragma unroll
                for (int w = 0; w < F32_THREADS / WAVE; ++w) {
                    const uint32_t c = cnts[w];
                    all += c;
                    before += w < cx.wave ? c : 0u;
                }
                before = (uint32_t)__builtin_amdgcn_readfirstlane((int)before);
                all = (uint32_t)__builtin_amdgcn_readfirstlane((int)all);
                uint32_t tail = r_head + r_cnt;
                if (tail >= r_cap) tail -= r_cap;
                const int j = cx.lane & 15;
                if ((mask >> j) & 1u) {
                    uint32_t idx = tail + before + (uint32_t)__popc(mask & ((1u << j) - 1u));
                    if (idx >= r_cap) idx -= r_cap;
                    const uint32_t slot = r_base + idx;
                    f32x4 *rec = sp.feat + (long)(slot >> 4) * (16 * 64) + q * 16 + (slot & 15u);
#pragma unroll
                    for (int b = 0; b < 16; ++b) rec[b * 64] = feat[b];
                    if (q == 0) sp.hdr[slot] = f32x4{stash[0], stash[1], stash[2], __int_as_float((int)p)};
                }
                r_cnt += all;
                r_total += all;
            }
            if (!do_branch) continue;      // the stream has wrapped to the first layer
            // the branch pass: x' -> stash (w is not needed behind the trunk), the FINAL tile behind fc_alpha from the raw row, feat from the record
            smp = __float_as_int(b_hdr[3]);
            __builtin_amdgcn_wave_barrier();
            if (q == 0) { stash[0] = b_hdr[0]; stash[1] = b_hdr[1]; stash[2] = b_hdr[2]; }
            __builtin_amdgcn_wave_barrier();
            fin[0] = *reinterpret_cast<const f32x4 *>(raw + smp * D_RAW + 4 * q);
            const f32x4 *rec = sp.feat + (long)(b_slot >> 4) * (16 * 64) + q * 16 + (b_slot & 15u);
#pragma unroll
            for (int b = 0; b < 16; ++b) feat[b] = rec[b * 64];
            r_cnt -= b_valid;
            r_head += (uint32_t)F32_PTS_PER_WG;
            if (r_head >= r_cap) r_head -= r_cap;
        }
        if (dbg != nullptr && p_raw < P) *reinterpret_cast<f32x4 *>(dsl + 24 + 4 * q) = fin[0];
        // ---- colour branch (modules.py:276-287) ----
        {
            f32x4 in_d[4];
            {
                const float *rp = rays + (smp / S) * ray_stride;
                const float rd[3] = {rp[3], rp[4], rp[5]};
                pe_blocks<3, 4, 2>(rd, q, in_d);                                  // models.py:340 (raw, un-normalised direction)
                grid_blocks(grid, stash[0], stash[1], stash[2], q, in_d + 2);     // models.py:525
                if (sv_on) {
#pragma unroll
                    for (int b = 0; b < 4; ++b) *reinterpret_cast<f32x4 *>(b < 2 ? SVP(act::DIR, 32) + 16 * b : SVP(act::GRID, 32) + 16 * (b - 2)) = in_d[b];
                }
            }
            if (dbg != nullptr && p_raw < P) {
                float *d = dbg + P * DBG_STRIDE + p * 32;
                *reinterpret_cast<f32x4 *>(d + 4 * q) = in_d[2];
                *reinterpret_cast<f32x4 *>(d + 16 + 4 * q) = in_d[3];
            }
            f32x4 c[8], cn[8];
            dense<2, 2, 8, CHF(L_D0A)>(cx, in_d, in_d + 2, c, Ly[L_D0B].bias_off, false, 1.0f);
            dense_sv<SAVE, 16, 0, 8, CHF(L_D1)>(cx, feat, nullptr, c, 0, true, 0.01f, SV(act::C, 128), SBR(sbits::BR_C + 4 * (0), 128));
            if (dump) dsl[14] = c[0][0];
#pragma unroll 1
            for (int l = 0; l < 2; ++l) {      // D1, D2
                dense_sv<SAVE, 8, 0, 8, CHF(L_D2)>(cx, c, nullptr, cn, Ly[L_D1].bias_off + 128 * l, false, 0.01f, SV(act::C + 128 * (l + 1), 128), SBR(sbits::BR_C + 4 * ((l + 1)), 128));
#pragma unroll
                for (int i = 0; i < 8; ++i) c[i] = cn[i];
            }
            dense_sv<SAVE, 8, 0, 8, CHF(L_RGB)>(cx, c, nullptr, cn, Ly[L_D3].bias_off, false, 0.01f, SV(act::C + 384, 128), SBR(sbits::BR_C + 4 * (3), 128));
            if (dump) dsl[15] = cn[0][0];
            dense<8, 0, 1, CHF(L_S0)>(cx, cn, nullptr, fin, 0, true, 1.0f);
            if (dbg != nullptr && p_raw < P) *reinterpret_cast<f32x4 *>(dsl + 40 + 4 * q) = fin[0];
        }
        // ---- seg branch (modules.py:289-294) ----
        {
            f32x4 s[8], sn[8];
            dense_sv<SAVE, 16, 0, 8, CHF(L_S1)>(cx, feat, nullptr, s, Ly[L_S0].bias_off, false, 0.01f, SV(act::S, 128), SBR(sbits::BR_S + 4 * (0), 128));
            if (dump) dsl[16] = s[0][0];
#pragma unroll 1
            for (int l = 0; l < 2; ++l) {      // S1, S2
                dense_sv<SAVE, 8, 0, 8, CHF(L_S2)>(cx, s, nullptr, sn, Ly[L_S1].bias_off + 128 * l, false, 0.01f, SV(act::S + 128 * (l + 1), 128), SBR(sbits::BR_S + 4 * ((l + 1)), 128));
#pragma unroll
                for (int i = 0; i < 8; ++i) s[i] = sn[i];
            }
            dense_sv<SAVE, 8, 0, 8, CHF(L_SEG)>(cx, s, nullptr, sn, Ly[L_S3].bias_off, false, 0.01f, SV(act::S + 384, 128), SBR(sbits::BR_S + 4 * (3), 128));
            if (dump) dsl[17] = sn[0][0];
            dense<8, 0, 1, CHF(L_START)>(cx, sn, nullptr, fin, 0, true, 1.0f);
        }
        if (FUSED ? (uint32_t)(cx.wave * F32_PTS_PER_WAVE + (cx.lane & 15)) < b_valid : p_raw < P)
            *reinterpret_cast<f32x4 *>(raw + smp * D_RAW + 4 * q) = fin[0];   // cat((rgb, seg, alpha)) modules.py:295
    }
    if constexpr (FUSED) {      // the pass's live count, once per workgroup (no value returned); the second head word: a sparse pass ran
        if (threadIdx.x == 0) {
            if (r_total != 0u) atomicAdd(sp.count, r_total);
            if (blockIdx.x == 0) sp.count[1] = 1u;
        }
    }
}

}  // namespace SAHS_NS

using namespace SAHS_NS;

// One launch of the field kernel on a block normalised for its mode (sahs_launchers.hpp: sahs_field_mode_block).
// dbg (optional, may be null): [P x 24: see DBG_STRIDE][P x 32: grid features]
template <bool SAVE, int MODE>
static int launch_field(const FieldLaunch &L, SparseArgs sp = SparseArgs{})
{
    const size_t lds_bytes = (size_t)field_lds_floats(SAVE, MODE) * sizeof(float);
    return sahs_launch_persistent<field_forward_f32_kernel<SAVE, MODE>>((L.P + F32_PTS_PER_WG - 1) / F32_PTS_PER_WG, L.num_cu, F32_THREADS, lds_bytes, L.stream,
                                                                        L.packed, L.frame, L.level, L.P, L.S, L.rays, L.ray_stride, L.zvals, L.raw, L.dbg,
                                                                        L.actbuf, L.xw, L.xw_row, L.xw_col0, L.src, L.bits, sp);
}

// The whole network and its split evaluation (see the kernel's MODE, and FieldLaunch for what each mode reads).  actbuf: a saved array of
// act:: column c starts at actbuf + c * P as for whole-network launches, so a radiance-only launch touches columns >= act::XW only and a
// deformation-only launch columns < act::XW + 16: the caller may pass a base such that only that range is backed by memory
// (sahs_layout_act_part_words).  bits (with actbuf): the sign-bit planes of the layers the launch runs (sahs_layout.hpp: sbits; mode 0:
// [deformation | radiance] planes), (P * sahs_layout_bits_part_words(mode)) 32-bit words, or null.
extern "C" int SAHS_SYM(sahs_field_f32_launch)(const FieldLaunch *in, int mode)
{
    if (in->P <= 0) return 0;
    FieldLaunch L = sahs_field_mode_block(*in, mode);
    const bool save = L.actbuf != nullptr;
    if (!save) L.bits = nullptr;
#if SAHS_MODEL == 2
    // no deformation nets in this model: the whole network only, and no x', w written unless it saves (the training forward that writes
    // its sign bits; capi: sahs_model_field_forward_save_bits)
    if (mode != FIELD_ALL || (!save && L.xw != nullptr)) return -3;
#endif
    switch (mode) {
    case FIELD_ALL: return save ? launch_field<true, FIELD_ALL>(L) : launch_field<false, FIELD_ALL>(L);
#if SAHS_MODEL != 2
    case FIELD_DEFORM: return save ? launch_field<true, FIELD_DEFORM>(L) : launch_field<false, FIELD_DEFORM>(L);
    case FIELD_RADIANCE: return save ? launch_field<true, FIELD_RADIANCE>(L) : launch_field<false, FIELD_RADIANCE>(L);
#endif
    default: return -2;
    }
}

// The sparse branches (see the kernel's MODE), one launch for the whole pass.  stage 0: FIELD_ALL_FUSED, the block read as mode 0 (x', w
// also written to xw when given); stage 1: FIELD_RADIANCE_FUSED, the block read as mode 2.  Nothing is saved and no debug planes written.
// ws: sahs_field_f32_sparse_ws_bytes(cap) bytes, 16-byte aligned: [head: two words, zeroed by the caller | headers | feat groups]; cap:
// record slots, a multiple of 128 and at least the workgroups' rings, sahs_field_f32_sparse_ring_slots(P, num_cu) (never more than P
// rounded up to 128).  noise / has_bg: the composite's noise of these samples (or null) and whether it is given a background prior --
// what decides which samples are live.  The launch adds the pass's live count to the head's first word and sets its second word to 1.
extern "C" long SAHS_SYM(sahs_field_f32_sparse_ws_bytes)(long cap) { return SPARSE_HEAD_BYTES + cap * SPARSE_RECORD_BYTES; }
extern "C" long SAHS_SYM(sahs_field_f32_sparse_ring_slots)(long P, int num_cu)
{
    if (P <= 0 || num_cu < 1) return 0;
    const long ntiles = (P + F32_PTS_PER_WG - 1) / F32_PTS_PER_WG, grid = ntiles < num_cu ? ntiles : num_cu;
    return sparse_ring_base(ntiles, grid, grid);
}
extern "C" int SAHS_SYM(sahs_field_f32_sparse_launch)(const FieldLaunch *in, int stage, const float *noise, int has_bg, void *ws, long cap)
{
    if (in->P <= 0) return 0;
    if (ws == nullptr || cap % F32_PTS_PER_WG != 0 || cap > (1L << 30)) return -4;
    if (cap < SAHS_SYM(sahs_field_f32_sparse_ring_slots)(in->P, in->num_cu)) return -4;
    char *base = static_cast<char *>(ws);
    SparseArgs sp{noise, reinterpret_cast<unsigned int *>(base), reinterpret_cast<f32x4 *>(base + SPARSE_HEAD_BYTES),
                  reinterpret_cast<f32x4 *>(base + SPARSE_HEAD_BYTES + cap * 16), (unsigned int)cap, has_bg};
    FieldLaunch L = sahs_field_mode_block(*in, stage == 0 ? FIELD_ALL : FIELD_RADIANCE);
    L.dbg = L.actbuf = nullptr;
    L.bits = nullptr;
    if (stage == 0) return launch_field<false, FIELD_ALL_FUSED>(L, sp);
#if SAHS_MODEL != 2
    if (stage == 1) return launch_field<false, FIELD_RADIANCE_FUSED>(L, sp);
#endif
    return -2;
}

// words per sample of the saved activations a launch of `part` writes / a backward of `part` reads, and the first act:: column of that
// range: part 0 whole network [0, STRIDE); 1 deformation nets [0, XW + 16); 2 radiance nets [XW, STRIDE)
extern "C" int SAHS_SYM(sahs_layout_act_part_words)(int part) { return part == 1 ? act::XW + 16 : (part == 2 ? act::STRIDE - act::XW : act::STRIDE); }
extern "C" int SAHS_SYM(sahs_layout_act_part_col0)(int part) { return part == 2 ? act::XW : 0; }
// 32-bit words per sample of the sign-bit planes of `part` (0: both, deformation planes first)
extern "C" int SAHS_SYM(sahs_layout_bits_part_words)(int part) { return part == 1 ? sbits::BD_WORDS : (part == 2 ? sbits::BR_WORDS : sbits::BD_WORDS + sbits::BR_WORDS); }
