// bwd_program.hpp -- the fused backward's view of the layer program: one table, generated from kProg (sahs_layout.hpp).
//
// The forward's kProg says which state_dict tensor a layer multiplies, its leading dimension, which of its columns are PE(x') / PE(w) /
// grid features / per-frame constants, and where a head's rows sit in the 16-float raw block.  The fused backward needs the same facts in
// three shapes, all built here so that they cannot disagree with the forward or with each other:
//   * kFwd: one entry per dense layer of the reference (the forward's split pairs merged as hb::from2 merges them, indexed by hb::LayerIdH).
//     The job tables of the weight-gradient launch are loops over it (field_bwd.hip: fused_rad / fused_def);
//   * make_rad<TILE> / make_def<TILE>: the data-gradient chains' programs of transposed layers, in 32-row tiles for the split-bf16 pipe
//     (field_bwd_chain.hip) and in 16-row tiles for the f32 pipe (field_bwd_chain_f32.hip);
//   * spot<TILE> / element: which parameter a given (row, k) of such a transposed layer is -- the one lookup both stream packers use.
// What the backward states on its own is only what kProg does not know: where the saving forward left a layer's input and output (the act::
// columns, make_table below) and the order of the chains and of the job tables.  The per-layer walk (field_bwd.hip) deliberately uses none
// of this: it is the independent statement of the network the fused walk is tested against.
#pragma once
#include <initializer_list>
#include "sahs_layout.hpp"

namespace SAHS_NS {

constexpr int DIN_LD = 16 * (KB_XYZ + KB_AMB);   // a row of the encodings' gradient [PE(x') blocks | PE(w) blocks] (din, din_a, din_b): 96 | 128 | 64 floats

namespace bwp {
using namespace hb;      // the merged layers' ids: H_W0 .. H_SEG

// ---- the table -----------------------------------------------------------------------------------------------------------------------
struct In { int col0, valid, width, plane; };      // an input segment: W's columns col0 .. col0 + valid - 1, saved as a [P x width] plane at act:: column `plane`
constexpr int HEAD = -1;                           // Dense::out of fc_rgb / fc_seg / fc_alpha / fc_final / fc_ambient: no dZ plane, their dZ is the gradient row itself
struct Dense {
    long w_off[2], b_off[2];      // in the flat parameter buffer, per level
    int ld, rows;                 // W is [rows x ld]
    int kshift;                   // a radiance head's rows sit at kshift .. of the raw block [rgb3 | seg12 | sigma] (kProg: row_shift)
    int nin; In in[3];            // hidden input first, then the re-injected ones (the order of hb::from2)
    int nfold; Fold fold[2];      // per-frame-constant columns: their gradients come from this layer's bias gradient
    int out;                      // act:: column of the layer's output plane = where its dZ goes
};
struct Table { Dense d[NUM_LAYERS_H]; int n; };

constexpr Table make_table()
{
    Table T{};
    for (int i = 0; i < NUM_LAYERS; ++i) {
        // a split pair is the injected half (carries bias and folds) followed by the hidden half (has_bias == 0)
        const Layer &b = kProg.layer[i];
        const Layer *a = (i + 1 < NUM_LAYERS && !kProg.layer[i + 1].has_bias) ? &kProg.layer[++i] : nullptr;
        Dense &D = T.d[T.n++];
        for (int l = 0; l < 2; ++l) {
            D.w_off[l] = b.w_off[l];
            D.b_off[l] = b.b_off[l];
            D.fold[l] = b.fold[l];
        }
        D.nfold = b.nfold;
        D.ld = b.src_ld;
        D.rows = b.src_rows;
        D.kshift = b.row_shift;
        for (const Layer *l : {a, &b}) {
            if (l == nullptr) continue;
            for (int s = 0; s < l->nseg; ++s) D.in[D.nin++] = In{l->seg[s].src_col, l->seg[s].valid, 16 * l->seg[s].blocks, 0};
        }
    }
    // The planes (act::, sahs_layout.hpp).  A net of `count` equally wide hidden layers from `first` leaves layer i's output at base + i * width
    // and reads it as layer i + 1's hidden input; layer 0 reads p0 .., a skip layer [hidden | p0 ..].
    auto net = [&T](int first, int count, int base, int p0, int p1 = 0, int p2 = 0) {
        const int p[3] = {p0, p1, p2};
        for (int i = 0; i < count; ++i) {
            Dense &D = T.d[first + i];
            D.out = base + i * D.rows;
            int s = 0;
            if (i > 0) D.in[s++].plane = base + (i - 1) * D.rows;
            for (int k = 0; s < D.nin; ++s, ++k) D.in[s].plane = p[k];
        }
    };
    auto head = [&T](int id, int plane) {
        T.d[id].out = HEAD;
        T.d[id].in[0].plane = plane;
    };
#if SAHS_MODEL != 2
    net(H_W0, 6, act::WH, act::E);
    head(H_WF, act::WH + 5 * WARP_H);
    net(H_H0, 6, act::HH, act::E);
    head(H_HF, act::HH + 5 * HYP_H);
#endif
    net(H_T0, TR_LAYERS, act::T, act::PEX, act::PEW);
    net(H_FEAT, 1, act::FEAT, act::T + (TR_LAYERS - 1) * TR_H);
    head(H_ALPHA, act::FEAT);
    net(H_D0, 4, act::C, act::FEAT, act::DIR, act::GRID);
    head(H_RGB, act::C + 3 * BR_H);
    net(H_S0, 4, act::S, act::FEAT);
    head(H_SEG, act::S + 3 * BR_H);
    return T;
}
constexpr Table kFwd = make_table();
constexpr bool merged_as_from2()
{
    if (kFwd.n != NUM_LAYERS_H) return false;
    for (int i = 0; i < NUM_LAYERS_H; ++i) {
        const LayerH &h = kProgH.layer[i];
        const Dense &d = kFwd.d[i];
        if (h.w_off[0] != d.w_off[0] || h.w_off[1] != d.w_off[1] || h.src_ld != d.ld || h.src_rows != d.rows || h.row_shift != d.kshift) return false;
        if (h.nseg != d.nin) return false;
        for (int s = 0; s < d.nin; ++s)
            if (h.seg[s].src_col != d.in[s].col0 || h.seg[s].valid != d.in[s].valid) return false;
    }
    return true;
}
static_assert(merged_as_from2(), "kFwd[id] is the layer hb::LayerIdH calls id");

// ---- the chains' programs --------------------------------------------------------------------------------------------------------------
// A backward layer multiplies A = (part of) W^T: its output rows are INPUT features of a forward layer (W's columns col0 ..), its K index
// runs over that layer's OUTPUT features (W's rows).  Up to three K segments (d feat sums three branches), up to two row ranges (the
// encodings' gradient: PE(x') columns, then PE(w) columns).  Tiles are TILE rows, k-blocks TILE gradients: 32 on the bf16 pipe, 16 on the
// f32 pipe.  The radiance heads read the 16-float d_raw row [drgb3 | dseg12 | dsigma] as (the start of) a k-block whose k = d_raw column:
// kshift places the head's weight rows (fc_seg: rows 0..11 at k = 3..14, fc_alpha: k = 15).
struct SegK { long w_off[2]; int ld, kshift, krows, blocks; };
struct Rows { int rows, col0, valid; };
struct BLayer {
    int NT, KB, nseg; SegK seg[3];
    int nrow; Rows row[2];
    long stream_off;      // in this part's stream (halfwords | floats)
    int chunk;            // of the stream per LDS chunk
};
template <int N> struct Prog { BLayer layer[N]; int n; long stream; };

// the gradient w.r.t. input segments in0 .. in0 + nin - 1 of forward layer id
struct Of { int id, in0 = 0, nin = 1; };
// ... summed over forward layers of.id, k1, k2, which all read those inputs at the same columns (d feat)
template <int TILE> constexpr BLayer back(Of of, int k1 = -1, int k2 = -1)
{
    BLayer L{};
    for (int k : {of.id, k1, k2}) {
        if (k < 0) continue;
        const Dense &D = kFwd.d[k];
        L.seg[L.nseg] = SegK{{D.w_off[0], D.w_off[1]}, D.ld, D.kshift, D.rows, (D.kshift + D.rows + TILE - 1) / TILE};
        L.KB += L.seg[L.nseg++].blocks;
    }
    int rows = 0;
    for (int s = of.in0; s < of.in0 + of.nin; ++s) {
        const In &I = kFwd.d[of.id].in[s];
        L.row[L.nrow++] = Rows{I.width, I.col0, I.valid};
        rows += I.width;
    }
    L.NT = (rows + TILE - 1) / TILE;
    if (TILE == 32) {      // what bf16x3_pipe.hpp: dense_x asks of a layer (its static_asserts) -- all of it zeros in the stream
        // its counted LDS waits need at least AP = 4 k-steps per tile: a head layer on its own runs over TWO blocks, the second all zeros
        if (L.KB < 2) {
            L.seg[0].blocks += 2 - L.KB;
            L.KB = 2;
        }
        // the last tile of a layer must land in accumulator set 1: the grid features' rows are padded to 2 tiles, the encodings' (96 or 128
        // rows) to 4
        L.NT += L.NT & 1;
    }
    return L;
}
template <int N> constexpr void add(Prog<N> &P, int (*pick)(int, int), int unit, BLayer L)
{
    L.stream_off = P.stream;
    L.chunk = pick(L.KB, L.NT) * L.KB * unit;
    P.stream += (long)L.NT * L.KB * unit;
    P.layer[P.n++] = L;
}
constexpr int tile_unit(int TILE) { return TILE == 32 ? 2048 : 256; }      // of the stream per tile and k-block: 32 x 32 bf16 hi + lo | 16 x 16 floats

// Radiance nets of one level in the chain's order; N names the layers (the files' R_* enums), pick is the pipe's chunking (pick_GX | pick_G).
template <int TILE, int N> constexpr Prog<N> make_rad(int (*pick)(int, int))
{
    Prog<N> P{};
    auto put = [&P, pick](BLayer L) { add(P, pick, tile_unit(TILE), L); };
    // colour branch, from its head back (modules.py:276-287), down to d grid features
    put(back<TILE>({H_RGB}));
    for (int i = 3; i >= 1; --i) put(back<TILE>({H_D0 + i}));
    put(back<TILE>({H_D0, 2}));
    // seg branch (modules.py:289-294)
    put(back<TILE>({H_SEG}));
    for (int i = 3; i >= 1; --i) put(back<TILE>({H_S0 + i}));
    // d feat = W_S0^T dS0 + W_D0[:, :256]^T dC0 + w_alpha dsigma: ONE three-segment layer on the bf16 pipe, whose dense_x takes three input
    // block arrays; the f32 pipe's dense_ep takes two, so there fc_alpha's term runs first as a layer of its own (R_FEATA, not stored) and
    // the two branches accumulate onto it (R_FEATB)
    if (TILE == 32) {
        put(back<TILE>({H_S0}, H_D0, H_ALPHA));
    } else {
        put(back<TILE>({H_ALPHA}));
        put(back<TILE>({H_S0}, H_D0));
    }
    // trunk (modules.py:267-274) from fc_feat back; a layer that reads [PE(x') | PE(w)] (skip layer 3, layer 0) also gives the encodings'
    // rows, in front of its hidden rows -- unless nothing upstream of the sample point has parameters (no deformation nets)
    put(back<TILE>({H_FEAT}));
    for (int i = TR_LAYERS - 1; i >= 1; --i) {
        if (USE_DEFORM && kFwd.d[H_T0 + i].nin > 1) put(back<TILE>({H_T0 + i, 1, kFwd.d[H_T0 + i].nin - 1}));
        put(back<TILE>({H_T0 + i}));
    }
    if (USE_DEFORM) put(back<TILE>({H_T0, 0, kFwd.d[H_T0].nin}));
    return P;
}
#if SAHS_MODEL != 2
// Deformation nets (shared by both levels): hyper sheet (modules.py:444-462, w = fc_ambient(g5)), then warp field (modules.py:371-390,
// dx = tanh(fc_final(h5))).  Their layer 0 and the skip layer's injected columns read PE(x) of the input point: no gradient wanted.
template <int TILE, int N> constexpr Prog<N> make_def(int (*pick)(int, int))
{
    Prog<N> P{};
    auto put = [&P, pick](BLayer L) { add(P, pick, tile_unit(TILE), L); };
    put(back<TILE>({H_HF}));
    for (int i = 5; i >= 1; --i) put(back<TILE>({H_H0 + i}));
    put(back<TILE>({H_WF}));
    for (int i = 5; i >= 1; --i) put(back<TILE>({H_W0 + i}));
    return P;
}
#endif

// Where row `row`, k-block b of backward layer L at `level` sits in the flat parameter buffer: its element k = TILE * b + kin is
// flat[base + (k0 + kin) * ld] for 0 <= k0 + kin < krows, zero otherwise (base < 0: a padding row, all zeros).  One thread of a packer
// resolves this once and then asks element() for each of its k.
struct Spot { long base; int ld, k0, krows; };
template <int TILE> constexpr Spot spot(const BLayer &L, int level, int row, int b)
{
    int col = -1, r0 = 0;
    for (int rs = 0; rs < L.nrow; ++rs) {
        if (row < r0 + L.row[rs].rows) {
            if (row - r0 < L.row[rs].valid) col = L.row[rs].col0 + (row - r0);
            break;
        }
        r0 += L.row[rs].rows;
    }
    int s = 0;
    while (s + 1 < L.nseg && b >= L.seg[s].blocks) b -= L.seg[s++].blocks;
    const SegK &S = L.seg[s];
    return Spot{col < 0 ? -1 : S.w_off[level] + col, S.ld, TILE * b - S.kshift, S.krows};
}
// -> index into flat, or -1 (zero)
constexpr long element(const Spot &w, int kin)
{
    const int k = w.k0 + kin;
    return (w.base < 0 || k < 0 || k >= w.krows) ? -1 : w.base + (long)k * w.ld;
}
// the layer of the stream position `at` (in the stream's units)
template <int N> constexpr const BLayer &layer_at(const Prog<N> &P, long at)
{
    int li = 0;
    while (li + 1 < N && P.layer[li + 1].stream_off <= at) ++li;
    return P.layer[li];
}

}  // namespace bwp
}  // namespace SAHS_NS
