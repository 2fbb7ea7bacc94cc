// capi.hip -- the extern "C" boundary declared in include/sahs_nerf.h: argument validation,
// error text, and the chained predict_and_render_radiance launch sequence.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#include <atomic>
#include <vector>
#include "../../include/sahs_nerf.h"
#include "sahs_common.hpp"
#include "sahs_layout.hpp"

using namespace sahs;

extern "C" {
int sahs_pack_weights_f32_launch(const float *flat, float *packed, hipStream_t stream);
int sahs_pack_weights_bf16_launch(const float *flat, float *packed, hipStream_t stream);
long sahs_field_backward_ws_words(long P);
int sahs_field_backward_launch(const float *flat, const float *frame, int level, long P, const float *actbuf, const float *d_raw,
                               float *grad_flat, float *grad_cond, float *ws, hipStream_t stream);
int sahs_stage1_loss_forward_launch(long N, const float *map_c, const float *map_f, const float *target, int target_ld, const float *mask,
                                    const float *class_w, float *stats, hipStream_t stream);
int sahs_composite_backward_launch(long N, int S, const float *raw, const float *z, const float *rays, int ray_stride, const float *noise,
                                   const float *bg, int white_bkgd, const float *d_rgb, const float *d_disp, const float *d_acc,
                                   const float *d_depth, const float *d_wlast, const float *d_weights, float *d_raw, const float *loss_map,
                                   const float *loss_target, int target_ld, const float *loss_mask, const float *loss_stats,
                                   const float *loss_gscale, hipStream_t stream);
int sahs_conditioning_backward_launch(const float *flat, const float *audio, const float *grad_cond, float *grad_flat, float *grad_audio,
                                      hipStream_t stream);
int sahs_field_forward_bf16w_launch(const float *packed, const float *frame, int level, long P, int S, const float *rays, int ray_stride,
                                    const float *zvals, float *raw, float *dbg, int num_cu, hipStream_t stream);
int sahs_field_forward_bf16w_split_launch(const float *packed, const float *frame, int level, int mode, long P, int S, const float *rays,
                                          int ray_stride, const float *zvals, float *raw, float *xw, int xw_row, int xw_col0, const int *src,
                                          int num_cu, hipStream_t stream);
int sahs_fold_conditioning_launch(const float *flat, const float *audio, const float *pose, int pose_ld, float *frame, hipStream_t stream);
int sahs_field_forward_f32_launch(const float *packed, const float *frame, int level, long P, int S, const float *rays, int ray_stride,
                                  const float *zvals, float *raw, float *dbg, float *actbuf, int num_cu, hipStream_t stream);
int sahs_ray_bundle_launch(int H, int W, float fx, float fy, float cx, float cy, const float *c2w, int ld, float *ro, float *rd,
                           hipStream_t stream);
int sahs_stratified_depths_launch(long N, int S, const float *rays, int ray_stride, int lindisp, const float *t_rand, float *z,
                                  hipStream_t stream);
int sahs_composite_forward_launch(long N, int S, const float *raw, const float *z, const float *rays, int ray_stride, const float *noise,
                                  const float *bg, int white_bkgd, float *rgb_map, float *disp, float *acc_map, float *weights,
                                  float *depth, float *w_last, int rgb_ld, int sc_ld, hipStream_t stream);
int sahs_resample_launch(long N, int S, int nf, int from_z, const float *z, const float *weights, const float *u, float *z_samples,
                         float *z_out, long long *inds, int *src, hipStream_t stream);
int sahs_ray_uniforms_launch(unsigned long long seed, int stream_id, long ray0, long N, int S, float *out, hipStream_t stream);
int sahs_route_xw_grad_launch(long N, int Sc, int nf, const int *src, const float *g_fine, float *g_coarse, float *g_new, hipStream_t stream);
long sahs_spade_stats_words(long planes);
int sahs_spade_modulate_launch(long planes, long hw, const float *x, const float *gamma, const float *beta, float eps, float slope, float *out,
                               float *stats, hipStream_t stream);
// the NeRFaceModel builds of pack.hip / field_f32.hip (sahs_model.hpp: SAHS_MODEL=1 suffix _nf, SAHS_MODEL=2 suffix _ns)
#define SAHS_DECLARE_MODEL(sfx)                                                                                                      \
    long sahs_layout_param_count##sfx(void);                                                                                        \
    long sahs_layout_packed_words_f32##sfx(void);                                                                                   \
    long sahs_layout_frame_words##sfx(void);                                                                                        \
    long sahs_layout_act_words##sfx(void);                                                                                          \
    long sahs_layout_executed_macs##sfx(int precision, int part);                                                                             \
    long sahs_field_backward_ws_words##sfx(long P);                                                                                 \
    int sahs_layout_act_part_words##sfx(int part);                                                                                  \
    int sahs_layout_act_part_col0##sfx(int part);                                                                                   \
    int sahs_layout_bits_part_words##sfx(int part);                                                                                 \
    int sahs_field_forward_f32_split_bits_launch##sfx(const float *packed, const float *frame, int level, int mode, long P, int S, \
                                                      const float *rays, int ray_stride, const float *zvals, float *raw, float *xw, \
                                                      int xw_row, int xw_col0, const int *src, float *actbuf, uint32_t *bits,       \
                                                      int num_cu, hipStream_t stream);                                              \
    int sahs_field_backward_split_launch##sfx(const float *flat, const float *frame, int level, int part, long P, const float *actbuf, \
                                              const float *d_raw, const float *xwg_in, float *xwg_out, float *grad_flat,            \
                                              float *grad_cond, float *ws, hipStream_t stream);                                     \
    int sahs_bwd_gemm_precision_state##sfx(int set);                                                                                 \
    int sahs_field_backward_launch##sfx(const float *flat, const float *frame, int level, long P, const float *actbuf,              \
                                        const float *d_raw, float *grad_flat, float *grad_cond, float *ws, hipStream_t stream);     \
    int sahs_pack_weights_f32_launch##sfx(const float *flat, float *packed, hipStream_t stream);                                   \
    int sahs_fold_conditioning_launch##sfx(const float *flat, const float *driving, const float *pose, int pose_ld, float *frame,  \
                                           hipStream_t stream);                                                                     \
    int sahs_field_forward_f32_launch##sfx(const float *packed, const float *frame, int level, long P, int S, const float *rays,   \
                                           int ray_stride, const float *zvals, float *raw, float *dbg, float *actbuf, int num_cu,   \
                                           hipStream_t stream);                                                                     \
    int sahs_field_forward_f32_split_launch##sfx(const float *packed, const float *frame, int level, int mode, long P, int S,      \
                                                 const float *rays, int ray_stride, const float *zvals, float *raw, float *xw,      \
                                                 int xw_row, int xw_col0, const int *src, float *actbuf, int num_cu,                \
                                                 hipStream_t stream);                                                               \
    long sahs_field_backward_fused_ws_words##sfx(int part, long P);                                                                 \
    int sahs_field_backward_fused_launch##sfx(const float *flat, const float *frame, int level, int part, long P, const float *actbuf, \
                                              const uint32_t *bits, const float *d_raw, const float *xwg_in, float *xwg_out,        \
                                              float *grad_flat, float *grad_cond, float *ws, int num_cu, hipStream_t stream);
SAHS_DECLARE_MODEL()
SAHS_DECLARE_MODEL(_nf)
SAHS_DECLARE_MODEL(_ns)
int sahs_bf16w_exact_leaky_state(int set);
int sahs_bf16w_exact_leaky_state_nf(int set);
int sahs_bf16w_exact_leaky_state_ns(int set);
// NeRFaceModel (with deformation) in mixed precision: bf16 radiance nets (field_bf16w.hip built with SAHS_MODEL=1), fp32 deformation nets
long sahs_layout_packed_words_bf16_nf(void);
int sahs_pack_weights_bf16_launch_nf(const float *flat, float *packed, hipStream_t stream);
int sahs_field_forward_bf16w_split_launch_nf(const float *packed, const float *frame, int level, int mode, long P, int S, const float *rays,
                                             int ray_stride, const float *zvals, float *raw, float *xw, int xw_row, int xw_col0, const int *src,
                                             int num_cu, hipStream_t stream);
// AudioFaceModel, SAHS_BF16X3: operands split into bf16 hi + lo (field_bf16x3.hip): radiance launch and, since round 3, deformation launch
long sahs_layout_packed_words_bf16x3(void);
int sahs_pack_weights_bf16x3_launch(const float *flat, float *packed, hipStream_t stream);
int sahs_field_deform_bf16x3_launch(const float *packed, const float *frame, int level, long P, int S, const float *rays, int ray_stride,
                                    const float *zvals, float *xw, int xw_row, int xw_col0, int num_cu, hipStream_t stream);
// NeRFaceModel with deformation nets (field_bf16x3.hip, SAHS_MODEL=1): both launches of its SAHS_BF16X3 split chain; the deformation
// kernel also for its mixed-precision path's deformation launches
long sahs_layout_packed_words_bf16x3_nf(void);
int sahs_pack_weights_bf16x3_launch_nf(const float *flat, float *packed, hipStream_t stream);
int sahs_field_deform_bf16x3_launch_nf(const float *packed, const float *frame, int level, long P, int S, const float *rays, int ray_stride,
                                       const float *zvals, float *xw, int xw_row, int xw_col0, int num_cu, hipStream_t stream);
int sahs_field_radiance_bf16x3_launch_nf(const float *packed, const float *frame, int level, long P, int S, const float *rays, int ray_stride,
                                         float *raw, const float *xw, int xw_row, const int *src, int num_cu, hipStream_t stream);
int sahs_field_deform_bf16x3_save_launch_nf(const float *packed, const float *frame, int level, long P, int S, const float *rays, int ray_stride,
                                            const float *zvals, float *xw, int xw_row, int xw_col0, float *actbuf, uint32_t *bits, int num_cu,
                                            hipStream_t stream);
int sahs_field_radiance_bf16x3_save_launch_nf(const float *packed, const float *frame, int level, long P, int S, const float *rays, int ray_stride,
                                              float *raw, const float *xw, int xw_row, const int *src, float *actbuf, uint32_t *bits, int num_cu,
                                              hipStream_t stream);
// NeRFaceModel without deformation nets (field_bf16x3.hip, SAHS_MODEL=2): the whole network on the split-operand pipe
long sahs_layout_packed_words_bf16x3_ns(void);
int sahs_pack_weights_bf16x3_launch_ns(const float *flat, float *packed, hipStream_t stream);
int sahs_field_forward_bf16x3_launch_ns(const float *packed, const float *frame, int level, long P, int S, const float *rays, int ray_stride,
                                        const float *zvals, float *raw, int num_cu, hipStream_t stream);
int sahs_field_forward_bf16x3_save_launch_ns(const float *packed, const float *frame, int level, long P, int S, const float *rays, int ray_stride,
                                             const float *zvals, float *raw, float *actbuf, uint32_t *bits, int num_cu, hipStream_t stream);
int sahs_field_radiance_bf16x3_launch(const float *packed, const float *frame, int level, long P, int S, const float *rays, int ray_stride,
                                      float *raw, const float *xw, int xw_row, const int *src, int num_cu, hipStream_t stream);
// ... that also write the saved activations and sign-bit planes of their part (training with the forward on this pipe)
int sahs_field_deform_bf16x3_save_launch(const float *packed, const float *frame, int level, long P, int S, const float *rays, int ray_stride,
                                         const float *zvals, float *xw, int xw_row, int xw_col0, float *actbuf, uint32_t *bits, int num_cu, hipStream_t stream);
int sahs_field_radiance_bf16x3_save_launch(const float *packed, const float *frame, int level, long P, int S, const float *rays, int ray_stride,
                                           float *raw, const float *xw, int xw_row, const int *src, float *actbuf, uint32_t *bits, int num_cu,
                                           hipStream_t stream);
// NeRFaceModel without deformation nets (person_1.yml): the whole network in bf16
long sahs_layout_packed_words_bf16_ns(void);
int sahs_pack_weights_bf16_launch_ns(const float *flat, float *packed, hipStream_t stream);
int sahs_field_forward_bf16w_launch_ns(const float *packed, const float *frame, int level, long P, int S, const float *rays, int ray_stride,
                                       const float *zvals, float *raw, float *dbg, int num_cu, hipStream_t stream);
}

static thread_local char g_err[512] = "";

static int fail(int code, const char *fmt, const char *a = "", long b = 0)
{
    snprintf(g_err, sizeof(g_err), fmt, a, b);
    return code;
}
static int hip_fail(const char *what, int e)
{
    snprintf(g_err, sizeof(g_err), "%s: HIP error %d (%s)", what, e, hipGetErrorString((hipError_t)e));
    return 100 + e;
}
#define REQUIRE(cond, name) do { if (!(cond)) return fail(1, "%s: invalid argument (%ld)", name, (long)__LINE__); } while (0)
#define ALIGNED16(p) ((reinterpret_cast<uintptr_t>(p) & 15u) == 0)

static int num_cus()     // of the CURRENT device (cached per device; the persistent field kernels launch one workgroup per CU)
{
    static std::atomic<int> cache[sahs_once::MAX_DEVICES];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= sahs_once::MAX_DEVICES) return 256;
    int n = cache[dev].load(std::memory_order_relaxed);
    if (n == 0) {
        int v = 0;
        n = (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? v : 256;
        cache[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}

// ---- launch probe (sahs_probe_*): while armed on the calling thread, every FIELD-kernel launch the library makes is bracketed by two
// HIP events recorded on the launch stream -- how bench.py times the kernels of the product's own call chain ----
struct Probe {
    bool armed = false;
    int cap = 0, n = 0, dropped = 0;
    std::vector<hipEvent_t> ev;      // two per launch
    std::vector<int> kind;
    std::vector<long> samples;
};
static thread_local Probe g_probe;
static inline int probe_kind(int model, int precision, int level, int part) { return model << 16 | level << 12 | part << 8 | precision; }
template <class F> static inline int probed(int kind, long samples, hipStream_t st, F &&launch)
{
    Probe &p = g_probe;
    if (!p.armed) return launch();
    if (p.n >= p.cap) { ++p.dropped; return launch(); }
    (void)hipEventRecord(p.ev[2 * p.n], st);
    const int e = launch();
    (void)hipEventRecord(p.ev[2 * p.n + 1], st);
    p.kind[p.n] = kind;
    p.samples[p.n] = samples;
    ++p.n;
    return e;
}

extern "C" {

int sahs_abi_version(void) { return SAHS_ABI_VERSION; }

int sahs_probe_arm(int capacity)
{
    Probe &p = g_probe;
    REQUIRE(capacity >= 1 && capacity <= 65536, "sahs_probe_arm(1 <= capacity <= 65536)");
    while ((int)p.ev.size() < 2 * capacity) {
        hipEvent_t e;
        const hipError_t r = hipEventCreate(&e);
        if (r != hipSuccess) return hip_fail("sahs_probe_arm", (int)r);
        p.ev.push_back(e);
    }
    p.kind.assign(capacity, 0);
    p.samples.assign(capacity, 0);
    p.cap = capacity;
    p.n = p.dropped = 0;
    p.armed = true;
    return 0;
}
int sahs_probe_disarm(void) { g_probe.armed = false; return 0; }
int sahs_probe_count(void) { return g_probe.n; }
int sahs_probe_dropped(void) { return g_probe.dropped; }
int sahs_probe_read(int i, int *kind, long *samples, float *ms)
{
    Probe &p = g_probe;
    REQUIRE(i >= 0 && i < p.n && kind && samples && ms, "sahs_probe_read");
    hipError_t r = hipEventSynchronize(p.ev[2 * i + 1]);
    if (r == hipSuccess) r = hipEventElapsedTime(ms, p.ev[2 * i], p.ev[2 * i + 1]);
    if (r != hipSuccess) return hip_fail("sahs_probe_read", (int)r);
    *kind = p.kind[i];
    *samples = p.samples[i];
    return 0;
}
const char *sahs_last_error(void) { return g_err; }
long sahs_param_count(void) { return kFlat.total; }
long sahs_packed_words(int precision)
{
    if (precision == SAHS_BF16X3) return sahs_layout_packed_words_bf16x3() + PACK_FLOATS;     // [hi/lo radiance streams | fp32 pack (deformation nets)]
    return precision == SAHS_F32 ? PACK_FLOATS : (precision == SAHS_BF16 ? hb::PACKH_WORDS : -1);
}
long sahs_frame_words(void) { return FRAME_FLOATS; }

int sahs_pack_weights(const float *flat_params, void *packed, int precision, void *stream)
{
    REQUIRE(flat_params && packed, "sahs_pack_weights");
    REQUIRE(ALIGNED16(packed), "sahs_pack_weights(packed alignment)");
    if (precision == SAHS_BF16X3) {
        int e = sahs_pack_weights_bf16x3_launch(flat_params, (float *)packed, (hipStream_t)stream);
        if (!e) e = sahs_pack_weights_f32_launch(flat_params, (float *)packed + sahs_layout_packed_words_bf16x3(), (hipStream_t)stream);
        return e ? hip_fail("sahs_pack_weights", e) : 0;
    }
    if (precision != SAHS_F32 && precision != SAHS_BF16) return fail(2, "sahs_pack_weights: unknown precision %s%ld", "", precision);
    int e = precision == SAHS_F32 ? sahs_pack_weights_f32_launch(flat_params, (float *)packed, (hipStream_t)stream)
                                  : sahs_pack_weights_bf16_launch(flat_params, (float *)packed, (hipStream_t)stream);
    return e ? hip_fail("sahs_pack_weights", e) : 0;
}

int sahs_fold_conditioning(const float *flat_params, const float *audio, const float *pose, int pose_ld, float *frame, void *stream)
{
    REQUIRE(flat_params && audio && pose && frame && pose_ld >= 4, "sahs_fold_conditioning");
    REQUIRE(ALIGNED16(frame), "sahs_fold_conditioning(frame alignment)");
    int e = sahs_fold_conditioning_launch(flat_params, audio, pose, pose_ld, frame, (hipStream_t)stream);
    return e ? hip_fail("sahs_fold_conditioning", e) : 0;
}

int sahs_get_ray_bundle(int H, int W, float fx, float fy, float cx, float cy, const float *c2w, int ld, float *ro, float *rd, void *stream)
{
    REQUIRE(H > 0 && W > 0 && c2w && ro && rd && ld >= 4, "sahs_get_ray_bundle");
    int e = sahs_ray_bundle_launch(H, W, fx, fy, cx, cy, c2w, ld, ro, rd, (hipStream_t)stream);
    return e ? hip_fail("sahs_get_ray_bundle", e) : 0;
}

int sahs_ray_uniforms(uint64_t seed, int stream_id, long ray0, long N, int S, float *out, void *stream)
{
    if (N == 0) return 0;
    REQUIRE(out && N >= 0 && S >= 1 && ray0 >= 0, "sahs_ray_uniforms");
    int e = sahs_ray_uniforms_launch(seed, stream_id, ray0, N, S, out, (hipStream_t)stream);
    return e ? hip_fail("sahs_ray_uniforms", e) : 0;
}

int sahs_stratified_depths(long N, int S, const float *rays, int ray_stride, int lindisp, const float *t_rand, float *z, void *stream)
{
    if (N == 0) return 0;
    REQUIRE(N >= 0 && S >= 1 && rays && z && ray_stride >= 8, "sahs_stratified_depths");
    int e = sahs_stratified_depths_launch(N, S, rays, ray_stride, lindisp, t_rand, z, (hipStream_t)stream);
    return e ? hip_fail("sahs_stratified_depths", e) : 0;
}

int sahs_field_forward(const void *packed, const float *frame, int level, long N, int S, const float *rays, int ray_stride,
                       const float *z, float *raw, float *dbg, int precision, void *stream)
{
    if (N == 0) return 0;
    REQUIRE(packed && frame && rays && z && raw, "sahs_field_forward");
    REQUIRE((level == 0 || level == 1) && N >= 0 && S >= 1 && ray_stride >= 8, "sahs_field_forward(shape)");
    REQUIRE(ALIGNED16(packed) && ALIGNED16(frame) && ALIGNED16(raw) && (!dbg || ALIGNED16(dbg)), "sahs_field_forward(alignment)");
    hipStream_t st = (hipStream_t)stream;
    if (precision == SAHS_BF16X3)
        return fail(2, "sahs_field_forward: SAHS_BF16X3 runs through sahs_model_field_forward_split / sahs_model_render_rays_rows (it needs the xw "
                       "workspace)%s%ld", "", 0L);
    if (precision != SAHS_F32 && precision != SAHS_BF16) return fail(2, "sahs_field_forward: unknown precision %s%ld", "", precision);
    int e = probed(probe_kind(SAHS_MODEL_AUDIO, precision, level, 0), N * S, st, [&] {
        return precision == SAHS_F32
                   ? sahs_field_forward_f32_launch((const float *)packed, frame, level, N * S, S, rays, ray_stride, z, raw, dbg, nullptr, num_cus(), st)
                   : sahs_field_forward_bf16w_launch((const float *)packed, frame, level, N * S, S, rays, ray_stride, z, raw, dbg, num_cus(), st);
    });
    return e ? hip_fail("sahs_field_forward", e) : 0;
}

int sahs_composite_forward(long N, int S, const float *raw, const float *z, const float *rays, int ray_stride, const float *noise,
                           const float *bg, int white_background, float *rgb, float *disp, float *acc, float *weights, float *depth,
                           void *stream)
{
    if (N == 0) return 0;
    REQUIRE(raw && z && rays && rgb && disp && acc && weights && depth && ray_stride >= 6, "sahs_composite_forward");
    REQUIRE(N >= 0 && S >= 1 && S <= 256 && ALIGNED16(raw), "sahs_composite_forward(shape: 1 <= S <= 256)");
    int e = sahs_composite_forward_launch(N, S, raw, z, rays, ray_stride, noise, bg, white_background, rgb, disp, acc, weights, depth,
                                          nullptr, 15, 1, (hipStream_t)stream);
    return e ? hip_fail("sahs_composite_forward", e) : 0;
}

int sahs_resample(long N, int S, int nf, const float *z, const float *weights, const float *u, float *z_samples, float *z_out,
                  int64_t *inds, void *stream)
{
    if (N == 0) return 0;
    REQUIRE(z && weights && z_out, "sahs_resample");
    REQUIRE(N >= 0 && S >= 3 && S <= 256 && nf >= 1 && nf <= 256, "sahs_resample(shape: 3 <= S <= 256, 1 <= nf <= 256)");
    int e = sahs_resample_launch(N, S, nf, 1, z, weights, u, z_samples, z_out, (long long *)inds, nullptr, (hipStream_t)stream);
    return e ? hip_fail("sahs_resample", e) : 0;
}

int sahs_resample_merge(long N, int S, int nf, const float *z, const float *weights, const float *u, float *z_samples, float *z_out,
                        int32_t *src, void *stream)
{
    if (N == 0) return 0;
    REQUIRE(z && weights && z_out && z_samples && src, "sahs_resample_merge");
    REQUIRE(N >= 0 && S >= 3 && S <= 256 && nf >= 1 && nf <= 256, "sahs_resample_merge(shape: 3 <= S <= 256, 1 <= nf <= 256)");
    int e = sahs_resample_launch(N, S, nf, 1, z, weights, u, z_samples, z_out, nullptr, src, (hipStream_t)stream);
    return e ? hip_fail("sahs_resample_merge", e) : 0;
}

int sahs_sample_pdf(long N, int nb, int ns, const float *bins, const float *weights, const float *u, float *samples, int64_t *inds,
                    void *stream)
{
    if (N == 0) return 0;
    REQUIRE(bins && weights && samples, "sahs_sample_pdf");
    REQUIRE(N >= 0 && nb >= 2 && nb < 256 && ns >= 1 && ns <= 256, "sahs_sample_pdf(shape: 2 <= nb < 256, 1 <= ns <= 256)");
    int e = sahs_resample_launch(N, nb + 1, ns, 0, bins, weights, u, samples, nullptr, (long long *)inds, nullptr, (hipStream_t)stream);
    return e ? hip_fail("sahs_sample_pdf", e) : 0;
}

int sahs_backward_gemm_precision(int precision)
{
    if (precision < 0) return sahs_bwd_gemm_precision_state(-1) ? SAHS_BF16X3 : SAHS_F32;
    if (precision != SAHS_F32 && precision != SAHS_BF16X3) return -1;
    const int v = precision == SAHS_BF16X3 ? 3 : 0;
    sahs_bwd_gemm_precision_state(v);
    sahs_bwd_gemm_precision_state_nf(v);
    sahs_bwd_gemm_precision_state_ns(v);
    return precision;
}

int sahs_bf16_exact_leaky(int enable)
{
    if (enable < 0) return sahs_bf16w_exact_leaky_state(-1);
    sahs_bf16w_exact_leaky_state_nf(enable);
    sahs_bf16w_exact_leaky_state_ns(enable);
    return sahs_bf16w_exact_leaky_state(enable);
}

long sahs_act_words_per_sample(void) { return act::STRIDE; }
long sahs_field_backward_workspace_words(long P) { return sahs_field_backward_ws_words(P); }

int sahs_field_forward_save(const void *packed, const float *frame, int level, long N, int S, const float *rays, int ray_stride,
                            const float *z, float *raw, float *act_out, void *stream)
{
    REQUIRE(packed && frame && rays && z && raw && act_out, "sahs_field_forward_save");
    REQUIRE((level == 0 || level == 1) && N >= 0 && S >= 1 && ray_stride >= 8, "sahs_field_forward_save(shape)");
    REQUIRE(ALIGNED16(packed) && ALIGNED16(frame) && ALIGNED16(raw) && ALIGNED16(act_out), "sahs_field_forward_save(alignment)");
    int e = sahs_field_forward_f32_launch((const float *)packed, frame, level, N * S, S, rays, ray_stride, z, raw, nullptr, act_out, num_cus(),
                                          (hipStream_t)stream);
    return e ? hip_fail("sahs_field_forward_save", e) : 0;
}

int sahs_field_backward(const float *flat_params, const float *frame, int level, long P, const float *act_in, const float *d_raw,
                        float *grad_flat, float *grad_cond, float *workspace, void *stream)
{
    REQUIRE(flat_params && frame && act_in && d_raw && grad_flat && grad_cond && workspace, "sahs_field_backward");
    REQUIRE((level == 0 || level == 1) && P >= 0 && P <= 4000000L, "sahs_field_backward(0 <= P <= 4e6 samples per call)");
    int e = sahs_field_backward_launch(flat_params, frame, level, P, act_in, d_raw, grad_flat, grad_cond, workspace, (hipStream_t)stream);
    return e ? hip_fail("sahs_field_backward", e) : 0;
}

int sahs_composite_backward(long N, int S, const float *raw, const float *z, const float *rays, int ray_stride, const float *noise,
                            const float *bg, int white_background, const float *d_rgb, const float *d_disp, const float *d_acc,
                            const float *d_depth, const float *d_wlast, const float *d_weights, float *d_raw, void *stream)
{
    REQUIRE(raw && z && rays && d_raw && ray_stride >= 6 && ALIGNED16(raw) && ALIGNED16(d_raw), "sahs_composite_backward");
    REQUIRE(N >= 0 && S >= 1 && S <= 256, "sahs_composite_backward(shape: 1 <= S <= 256)");
    if (N == 0) return 0;
    int e = sahs_composite_backward_launch(N, S, raw, z, rays, ray_stride, noise, bg, white_background, d_rgb, d_disp, d_acc, d_depth, d_wlast,
                                           d_weights, d_raw, nullptr, nullptr, 0, nullptr, nullptr, nullptr, (hipStream_t)stream);
    return e ? hip_fail("sahs_composite_backward", e) : 0;
}

int sahs_stage1_loss_forward(long N, const float *map_coarse, const float *map_fine, const float *target, int target_ld, const float *mask,
                             const float *class_weights, float *stats, void *stream)
{
    REQUIRE((map_coarse || map_fine) && target && mask && class_weights && stats && target_ld >= 3 && N >= 1, "sahs_stage1_loss_forward");
    int e = sahs_stage1_loss_forward_launch(N, map_coarse, map_fine, target, target_ld, mask, class_weights, stats, (hipStream_t)stream);
    return e ? hip_fail("sahs_stage1_loss_forward", e) : 0;
}

int sahs_composite_backward_loss(long N, int S, const float *raw, const float *z, const float *rays, int ray_stride, const float *noise,
                                 const float *bg, int white_background, const float *d_rgb, const float *d_disp, const float *d_acc,
                                 const float *d_depth, const float *d_wlast, const float *loss_map, const float *loss_target, int target_ld,
                                 const float *loss_mask, const float *loss_stats, const float *loss_gscale, float *d_raw, void *stream)
{
    REQUIRE(raw && z && rays && d_raw && ray_stride >= 6 && ALIGNED16(raw) && ALIGNED16(d_raw), "sahs_composite_backward_loss");
    REQUIRE(loss_map && loss_target && loss_mask && loss_stats && target_ld >= 3, "sahs_composite_backward_loss(loss operands)");
    REQUIRE(N >= 0 && S >= 1 && S <= 256, "sahs_composite_backward_loss(shape: 1 <= S <= 256)");
    if (N == 0) return 0;
    int e = sahs_composite_backward_launch(N, S, raw, z, rays, ray_stride, noise, bg, white_background, d_rgb, d_disp, d_acc, d_depth, d_wlast,
                                           nullptr, d_raw, loss_map, loss_target, target_ld, loss_mask, loss_stats, loss_gscale,
                                           (hipStream_t)stream);
    return e ? hip_fail("sahs_composite_backward_loss", e) : 0;
}

int sahs_conditioning_backward(const float *flat_params, const float *audio, const float *grad_cond, float *grad_flat, float *grad_audio,
                               void *stream)
{
    REQUIRE(flat_params && audio && grad_cond && grad_flat, "sahs_conditioning_backward");
    int e = sahs_conditioning_backward_launch(flat_params, audio, grad_cond, grad_flat, grad_audio, (hipStream_t)stream);
    return e ? hip_fail("sahs_conditioning_backward", e) : 0;
}

typedef int (*field_fn_t)(const void *, const float *, int, long, int, const float *, int, const float *, float *, float *, int, void *);

static int render_rays_chain(field_fn_t field, const char *who, const void *packed, const float *frame, int precision, long N,
                             const float *rays, int ray_stride, int Sc, int nf, int lindisp, int white_background, const float *bg,
                             const float *t_rand, const float *noise_c, const float *u, const float *noise_f, float *z_c, float *z_f,
                             float *raw, float *weights, float *rgb_c, float *disp_c, float *acc_c, float *rgb_f, float *disp_f,
                             float *acc_f, float *w_bg, float *depth_f, void *stream, int rgb_ld = 15, int sc_ld = 1)
{
    if (N == 0) return 0;   // an empty ray chunk: nothing to launch (its tensors have null data pointers)
    REQUIRE(packed && frame && rays && z_c && raw && weights && rgb_c && disp_c && acc_c && w_bg && depth_f, who);
    REQUIRE(nf == 0 || (z_f && rgb_f && disp_f && acc_f), who);
    hipStream_t st = (hipStream_t)stream;
    int e;
    if ((e = sahs_stratified_depths(N, Sc, rays, ray_stride, lindisp, t_rand, z_c, stream))) return e;
    if ((e = field(packed, frame, 0, N, Sc, rays, ray_stride, z_c, raw, nullptr, precision, stream))) return e;
    REQUIRE(Sc <= 256, who);
    // the coarse depth is written only when there is no fine pass (the reference returns depth_fine only)
    e = sahs_composite_forward_launch(N, Sc, raw, z_c, rays, ray_stride, noise_c, bg, white_background, rgb_c, disp_c, acc_c, weights,
                                      nf == 0 ? depth_f : nullptr, nf == 0 ? w_bg : nullptr, rgb_ld, sc_ld, st);
    if (e) return hip_fail(who, e);
    if (nf > 0) {
        const int Sf = Sc + nf;
        REQUIRE(Sf <= 256, who);
        if ((e = sahs_resample(N, Sc, nf, z_c, weights, u, nullptr, z_f, nullptr, stream))) return e;
        if ((e = field(packed, frame, 1, N, Sf, rays, ray_stride, z_f, raw, nullptr, precision, stream))) return e;
        e = sahs_composite_forward_launch(N, Sf, raw, z_f, rays, ray_stride, noise_f, bg, white_background, rgb_f, disp_f, acc_f,
                                          weights, depth_f, w_bg, rgb_ld, sc_ld, st);
        if (e) return hip_fail(who, e);
    }
    return 0;
}

int sahs_render_rays(const void *packed, const float *frame, int precision, long N, const float *rays, int ray_stride, int Sc, int nf,
                     int lindisp, int white_background, const float *bg, const float *t_rand, const float *noise_c, const float *u,
                     const float *noise_f, float *z_c, float *z_f, float *raw, float *weights, float *rgb_c, float *disp_c,
                     float *acc_c, float *rgb_f, float *disp_f, float *acc_f, float *w_bg, float *depth_f, void *stream)
{
    return render_rays_chain(sahs_field_forward, "sahs_render_rays", packed, frame, precision, N, rays, ray_stride, Sc, nf, lindisp,
                             white_background, bg, t_rand, noise_c, u, noise_f, z_c, z_f, raw, weights, rgb_c, disp_c, acc_c, rgb_f, disp_f,
                             acc_f, w_bg, depth_f, stream);
}

// ---- every built architecture behind one family: sahs_model_*(model, ...) ----
// model: SAHS_MODEL_AUDIO (the functions above), SAHS_MODEL_NERFACE (config/expression/person_2|3.yml),
// SAHS_MODEL_NERFACE_STATIC (config/expression/person_1.yml: no warp, no hyper sheet).
struct ModelFns {
    long (*param_count)(void);
    long (*packed_words_f32)(void);
    long (*frame_words)(void);
    int (*pack_f32)(const float *, float *, hipStream_t);
    int (*fold)(const float *, const float *, const float *, int, float *, hipStream_t);
    int (*field_f32)(const float *, const float *, int, long, int, const float *, int, const float *, float *, float *, float *, int, hipStream_t);
    long (*act_words)(void);
    long (*bwd_ws_words)(long);
    int (*bwd)(const float *, const float *, int, long, const float *, const float *, float *, float *, float *, hipStream_t);
};
static const ModelFns kModels[3] = {
    {sahs_layout_param_count, sahs_layout_packed_words_f32, sahs_layout_frame_words, sahs_pack_weights_f32_launch,
     sahs_fold_conditioning_launch, sahs_field_forward_f32_launch, sahs_layout_act_words, sahs_field_backward_ws_words,
     sahs_field_backward_launch},
    {sahs_layout_param_count_nf, sahs_layout_packed_words_f32_nf, sahs_layout_frame_words_nf, sahs_pack_weights_f32_launch_nf,
     sahs_fold_conditioning_launch_nf, sahs_field_forward_f32_launch_nf, sahs_layout_act_words_nf, sahs_field_backward_ws_words_nf,
     sahs_field_backward_launch_nf},
    {sahs_layout_param_count_ns, sahs_layout_packed_words_f32_ns, sahs_layout_frame_words_ns, sahs_pack_weights_f32_launch_ns,
     sahs_fold_conditioning_launch_ns, sahs_field_forward_f32_launch_ns, sahs_layout_act_words_ns, sahs_field_backward_ws_words_ns,
     sahs_field_backward_launch_ns},
};
#define REQUIRE_MODEL(m, name) do { if ((m) < 0 || (m) > 2) return fail(3, "%s: unknown model %ld", name, (long)(m)); } while (0)

long sahs_model_param_count(int model) { return (model < 0 || model > 2) ? -1 : kModels[model].param_count(); }
// NeRFaceModel, mixed precision: word offset of the split-operand streams behind [bf16 radiance pack | fp32 pack], 16-byte aligned
static long nf_mixed_x3_off() { return (sahs_layout_packed_words_bf16_nf() + kModels[SAHS_MODEL_NERFACE].packed_words_f32() + 3) / 4 * 4; }
long sahs_model_packed_words(int model, int precision)
{
    if (model < 0 || model > 2) return -1;
    if (model == SAHS_MODEL_AUDIO) return sahs_packed_words(precision);
    if (model == SAHS_MODEL_NERFACE && precision == SAHS_BF16)     // mixed precision: [bf16 radiance pack | fp32 pack | hi/lo streams (deformation nets)]
        return nf_mixed_x3_off() + sahs_layout_packed_words_bf16x3_nf();
    if (model == SAHS_MODEL_NERFACE_STATIC && precision == SAHS_BF16) return sahs_layout_packed_words_bf16_ns();
    if (model == SAHS_MODEL_NERFACE && precision == SAHS_BF16X3)     // the AudioFaceModel's layout: [hi/lo streams | fp32 pack (SAHS_X3_DEFORM=f32)]
        return sahs_layout_packed_words_bf16x3_nf() + kModels[model].packed_words_f32();
    if (model == SAHS_MODEL_NERFACE_STATIC && precision == SAHS_BF16X3) return sahs_layout_packed_words_bf16x3_ns();
    return precision == SAHS_F32 ? kModels[model].packed_words_f32() : -1;
}
// SAHS_X3_DEFORM=f32 (read once): the split chains' deformation launches run on the fp32 kernel instead of the split-operand one (A/B aid)
static bool x3_deform_on_f32()
{
    static const bool v = getenv("SAHS_X3_DEFORM") != nullptr && strcmp(getenv("SAHS_X3_DEFORM"), "f32") == 0;
    return v;
}
long sahs_model_executed_macs_part(int model, int precision, int part)
{
    if (model < 0 || model > 2 || precision < SAHS_F32 || precision > SAHS_BF16X3 || part < 0 || part > 2) return -1;
    if (precision == SAHS_BF16X3)       // three bf16 MFMAs per product, every net
    {
        if (model == SAHS_MODEL_NERFACE_STATIC) return 3 * sahs_layout_executed_macs_ns(SAHS_BF16, part);      // (no deformation nets: part 1 is 0)
        auto macs = model == SAHS_MODEL_AUDIO ? sahs_layout_executed_macs : sahs_layout_executed_macs_nf;
        if (x3_deform_on_f32())       // the deformation launches are the fp32 kernel's then: price them as what is issued
            return (part != 2 ? macs(SAHS_F32, 1) : 0) + (part != 1 ? 3 * macs(SAHS_BF16, 2) : 0);
        return 3 * macs(SAHS_BF16, part);
    }
    if (model == SAHS_MODEL_NERFACE_STATIC && part != 0) return part == 2 ? sahs_layout_executed_macs_ns(precision == SAHS_F32 ? SAHS_F32 : SAHS_BF16, 0) : 0;
    if (model == SAHS_MODEL_NERFACE && precision == SAHS_BF16)      // mixed: split-operand deformation nets (3 MFMAs per product) + bf16 radiance nets
        return (part != 2 ? (x3_deform_on_f32() ? sahs_layout_executed_macs_nf(SAHS_F32, 1) : 3 * sahs_layout_executed_macs_nf(SAHS_BF16, 1)) : 0) +
               (part != 1 ? sahs_layout_executed_macs_nf(SAHS_BF16, 2) : 0);
    return model == 0 ? sahs_layout_executed_macs(precision, part)
                      : (model == 1 ? sahs_layout_executed_macs_nf(precision, part) : sahs_layout_executed_macs_ns(precision, part));
}
long sahs_model_executed_macs_per_sample(int model, int precision) { return sahs_model_executed_macs_part(model, precision, 0); }
long sahs_model_frame_words(int model) { return (model < 0 || model > 2) ? -1 : kModels[model].frame_words(); }

int sahs_model_pack_weights(int model, const float *flat_params, void *packed, int precision, void *stream)
{
    REQUIRE_MODEL(model, "sahs_model_pack_weights");
    if (model == SAHS_MODEL_AUDIO) return sahs_pack_weights(flat_params, packed, precision, stream);
    REQUIRE(flat_params && packed && ALIGNED16(packed), "sahs_model_pack_weights");
    if (model == SAHS_MODEL_NERFACE && precision == SAHS_BF16) {
        int e = sahs_pack_weights_bf16_launch_nf(flat_params, (float *)packed, (hipStream_t)stream);
        if (!e) e = kModels[model].pack_f32(flat_params, (float *)packed + sahs_layout_packed_words_bf16_nf(), (hipStream_t)stream);
        if (!e) e = sahs_pack_weights_bf16x3_launch_nf(flat_params, (float *)packed + nf_mixed_x3_off(), (hipStream_t)stream);
        return e ? hip_fail("sahs_model_pack_weights", e) : 0;
    }
    if (model == SAHS_MODEL_NERFACE_STATIC && precision == SAHS_BF16) {
        int e = sahs_pack_weights_bf16_launch_ns(flat_params, (float *)packed, (hipStream_t)stream);
        return e ? hip_fail("sahs_model_pack_weights", e) : 0;
    }
    if (model == SAHS_MODEL_NERFACE && precision == SAHS_BF16X3) {
        int e = sahs_pack_weights_bf16x3_launch_nf(flat_params, (float *)packed, (hipStream_t)stream);
        if (!e) e = kModels[model].pack_f32(flat_params, (float *)packed + sahs_layout_packed_words_bf16x3_nf(), (hipStream_t)stream);
        return e ? hip_fail("sahs_model_pack_weights", e) : 0;
    }
    if (model == SAHS_MODEL_NERFACE_STATIC && precision == SAHS_BF16X3) {
        int e = sahs_pack_weights_bf16x3_launch_ns(flat_params, (float *)packed, (hipStream_t)stream);
        return e ? hip_fail("sahs_model_pack_weights", e) : 0;
    }
    if (precision != SAHS_F32) return fail(2, "sahs_model_pack_weights: precision %s%ld is not built for this model", "", precision);
    int e = kModels[model].pack_f32(flat_params, (float *)packed, (hipStream_t)stream);
    return e ? hip_fail("sahs_model_pack_weights", e) : 0;
}

int sahs_model_fold_conditioning(int model, const float *flat_params, const float *driving, const float *pose, int pose_ld, float *frame,
                                 void *stream)
{
    REQUIRE_MODEL(model, "sahs_model_fold_conditioning");
    REQUIRE(flat_params && driving && pose && frame && pose_ld >= 4 && ALIGNED16(frame), "sahs_model_fold_conditioning");
    int e = kModels[model].fold(flat_params, driving, pose, pose_ld, frame, (hipStream_t)stream);
    return e ? hip_fail("sahs_model_fold_conditioning", e) : 0;
}

static int field_forward_model(int model, const void *packed, const float *frame, int level, long N, int S, const float *rays,
                               int ray_stride, const float *z, float *raw, float *dbg, int precision, void *stream)
{
    if (model == SAHS_MODEL_AUDIO) return sahs_field_forward(packed, frame, level, N, S, rays, ray_stride, z, raw, dbg, precision, stream);
    if (N == 0) return 0;
    REQUIRE(packed && frame && rays && z && raw, "sahs_model_field_forward");
    REQUIRE((level == 0 || level == 1) && N >= 0 && S >= 1 && ray_stride >= 8, "sahs_model_field_forward(shape)");
    REQUIRE(ALIGNED16(packed) && ALIGNED16(frame) && ALIGNED16(raw) && (!dbg || ALIGNED16(dbg)), "sahs_model_field_forward(alignment)");
    if (model == SAHS_MODEL_NERFACE && (precision == SAHS_BF16 || precision == SAHS_BF16X3))
        return fail(2, "sahs_model_field_forward: the mixed-precision and SAHS_BF16X3 NeRFaceModel run through sahs_model_field_forward_split / "
                       "sahs_model_render_rays_rows (they need the xw workspace)%s%ld", "", 0L);
    hipStream_t st = (hipStream_t)stream;
    if (model == SAHS_MODEL_NERFACE_STATIC && precision == SAHS_BF16) {
        int e = probed(probe_kind(model, precision, level, 0), N * S, st, [&] {
            return sahs_field_forward_bf16w_launch_ns((const float *)packed, frame, level, N * S, S, rays, ray_stride, z, raw, dbg, num_cus(), st);
        });
        return e ? hip_fail("sahs_model_field_forward", e) : 0;
    }
    if (model == SAHS_MODEL_NERFACE_STATIC && precision == SAHS_BF16X3) {      // the whole network on the split-operand pipe (no debug planes)
        int e = probed(probe_kind(model, precision, level, 0), N * S, st, [&] {
            return sahs_field_forward_bf16x3_launch_ns((const float *)packed, frame, level, N * S, S, rays, ray_stride, z, raw, num_cus(), st);
        });
        return e ? hip_fail("sahs_model_field_forward", e) : 0;
    }
    if (precision != SAHS_F32) return fail(2, "sahs_model_field_forward: precision %s%ld is not built for this model", "", precision);
    int e = probed(probe_kind(model, precision, level, 0), N * S, st, [&] {
        return kModels[model].field_f32((const float *)packed, frame, level, N * S, S, rays, ray_stride, z, raw, dbg, nullptr, num_cus(), st);
    });
    return e ? hip_fail("sahs_model_field_forward", e) : 0;
}

int sahs_model_field_forward(int model, const void *packed, const float *frame, int level, long N, int S, const float *rays, int ray_stride,
                             const float *z, float *raw, float *dbg, int precision, void *stream)
{
    REQUIRE_MODEL(model, "sahs_model_field_forward");
    return field_forward_model(model, packed, frame, level, N, S, rays, ray_stride, z, raw, dbg, precision, stream);
}

long sahs_model_act_words_per_sample(int model) { return (model < 0 || model > 2) ? -1 : kModels[model].act_words(); }
long sahs_model_field_backward_workspace_words(int model, long P) { return (model < 0 || model > 2) ? -1 : kModels[model].bwd_ws_words(P); }

int sahs_model_field_forward_save(int model, const void *packed, const float *frame, int level, long N, int S, const float *rays,
                                  int ray_stride, const float *z, float *raw, float *act_out, void *stream)
{
    REQUIRE_MODEL(model, "sahs_model_field_forward_save");
    REQUIRE(packed && frame && rays && z && raw && act_out, "sahs_model_field_forward_save");
    REQUIRE((level == 0 || level == 1) && N >= 0 && S >= 1 && ray_stride >= 8, "sahs_model_field_forward_save(shape)");
    REQUIRE(ALIGNED16(packed) && ALIGNED16(frame) && ALIGNED16(raw) && ALIGNED16(act_out), "sahs_model_field_forward_save(alignment)");
    int e = kModels[model].field_f32((const float *)packed, frame, level, N * S, S, rays, ray_stride, z, raw, nullptr, act_out, num_cus(),
                                     (hipStream_t)stream);
    return e ? hip_fail("sahs_model_field_forward_save", e) : 0;
}

int sahs_model_field_backward(int model, const float *flat_params, const float *frame, int level, long P, const float *act_in,
                              const float *d_raw, float *grad_flat, float *grad_cond, float *workspace, void *stream)
{
    REQUIRE_MODEL(model, "sahs_model_field_backward");
    REQUIRE(flat_params && frame && act_in && d_raw && grad_flat && grad_cond && workspace, "sahs_model_field_backward");
    REQUIRE((level == 0 || level == 1) && P >= 0 && P <= 4000000L, "sahs_model_field_backward(0 <= P <= 4e6 samples per call)");
    int e = kModels[model].bwd(flat_params, frame, level, P, act_in, d_raw, grad_flat, grad_cond, workspace, (hipStream_t)stream);
    return e ? hip_fail("sahs_model_field_backward", e) : 0;
}

static int field_nf(const void *pk, const float *fr, int lv, long N, int S, const float *r, int rs, const float *z, float *raw, float *dbg, int pr, void *st)
{ return field_forward_model(SAHS_MODEL_NERFACE, pk, fr, lv, N, S, r, rs, z, raw, dbg, pr, st); }
static int field_ns(const void *pk, const float *fr, int lv, long N, int S, const float *r, int rs, const float *z, float *raw, float *dbg, int pr, void *st)
{ return field_forward_model(SAHS_MODEL_NERFACE_STATIC, pk, fr, lv, N, S, r, rs, z, raw, dbg, pr, st); }

int sahs_model_render_rays(int model, const void *packed, const float *frame, int precision, long N, const float *rays, int ray_stride,
                           int Sc, int nf, int lindisp, int white_background, const float *bg, const float *t_rand, const float *noise_c,
                           const float *u, const float *noise_f, float *z_c, float *z_f, float *raw, float *weights, float *rgb_c,
                           float *disp_c, float *acc_c, float *rgb_f, float *disp_f, float *acc_f, float *w_bg, float *depth_f, void *stream)
{
    REQUIRE_MODEL(model, "sahs_model_render_rays");
    field_fn_t f = model == SAHS_MODEL_AUDIO ? sahs_field_forward : (model == SAHS_MODEL_NERFACE ? field_nf : field_ns);
    return render_rays_chain(f, "sahs_model_render_rays", packed, frame, precision, N, rays, ray_stride, Sc, nf, lindisp, white_background, bg,
                             t_rand, noise_c, u, noise_f, z_c, z_f, raw, weights, rgb_c, disp_c, acc_c, rgb_f, disp_f, acc_f, w_bg, depth_f, stream);
}

/* The split evaluation of the field (csrc/field_f32.hip, MODE): 0 whole network + x', w written to xw; 1 deformation nets only;
 * 2 radiance net only, x', w fetched from xw through src. */
int sahs_model_field_forward_split(int model, const void *packed, const float *frame, int precision, int level, int mode, long N, int S,
                                   const float *rays, int ray_stride, const float *z, float *raw, float *xw, int xw_row, int xw_col0,
                                   const int32_t *src, void *stream)
{
    REQUIRE_MODEL(model, "sahs_model_field_forward_split");
    if (N == 0) return 0;
    if (model == SAHS_MODEL_NERFACE_STATIC) return fail(4, "sahs_model_field_forward_split: this model has no deformation nets%s%ld", "", 0L);
    REQUIRE(packed && frame && rays && xw && (level == 0 || level == 1) && N >= 0 && S >= 1 && ray_stride >= 8 && mode >= 0 && mode <= 2,
            "sahs_model_field_forward_split");
    const bool x3 = precision == SAHS_BF16X3, audio = model == SAHS_MODEL_AUDIO;
    const bool mixed = (precision == SAHS_BF16 && model == SAHS_MODEL_NERFACE) || x3;
    REQUIRE((mode == 1 || raw) && (mode == 2 || z) && (mode != 2 || src || mixed), "sahs_model_field_forward_split(buffers of the mode)");
    REQUIRE(xw_col0 >= 0 && xw_row >= xw_col0 + (mode == 2 ? 0 : S) && ALIGNED16(xw) && ALIGNED16(packed) && ALIGNED16(frame) && (!raw || ALIGNED16(raw)),
            "sahs_model_field_forward_split(xw layout / alignment)");
    hipStream_t st = (hipStream_t)stream;
    if (mixed) {      // deformation launch, then radiance launch (mode 0 = both, one after the other)
        // packed: SAHS_BF16X3 [hi/lo streams | fp32 pack]; the NeRFaceModel's mixed precision [bf16 radiance pack | fp32 pack | hi/lo streams]
        const float *pk16 = (const float *)packed;
        const float *pk32 = pk16 + (x3 ? (audio ? sahs_layout_packed_words_bf16x3() : sahs_layout_packed_words_bf16x3_nf()) : sahs_layout_packed_words_bf16_nf());
        REQUIRE(mode != 0 || xw_col0 == 0, "sahs_model_field_forward_split(mixed precision, mode 0: xw_col0 must be 0)");
        int e = 0;
        // the deformation nets run on the split-operand pipe (field_bf16x3.hip; round 3 -- SAHS_X3_DEFORM=f32 in the environment keeps them
        // on the fp32 kernel, the A/B reference and the form round 2 shipped): SAHS_BF16X3, and the mixed-precision NeRFaceModel, whose
        // radiance nets are plain bf16 anyway
        const bool x3_deform_f32 = x3_deform_on_f32();
        if (mode != 2 && !x3_deform_f32)
            e = probed(probe_kind(model, SAHS_BF16X3, level, 1), N * S, st, [&] {
                return x3 && audio ? sahs_field_deform_bf16x3_launch(pk16, frame, level, N * S, S, rays, ray_stride, z, xw, xw_row, xw_col0, num_cus(), st)
                                   : sahs_field_deform_bf16x3_launch_nf(pk16 + (x3 ? 0 : nf_mixed_x3_off()), frame, level, N * S, S, rays, ray_stride, z, xw,
                                                                        xw_row, xw_col0, num_cus(), st);
            });
        else if (mode != 2)
            e = probed(probe_kind(model, SAHS_F32, level, 1), N * S, st, [&] {
                return audio ? sahs_field_forward_f32_split_launch(pk32, frame, level, 1, N * S, S, rays, ray_stride, z, nullptr, xw, xw_row, xw_col0, nullptr,
                                                                   nullptr, num_cus(), st)
                             : sahs_field_forward_f32_split_launch_nf(pk32, frame, level, 1, N * S, S, rays, ray_stride, z, nullptr, xw, xw_row, xw_col0, nullptr,
                                                                      nullptr, num_cus(), st);
            });
        if (!e && mode != 1)
            e = probed(probe_kind(model, precision, level, 2), N * S, st, [&] {
                const int *sp = mode == 2 ? src : nullptr;
                return !x3   ? sahs_field_forward_bf16w_split_launch_nf(pk16, frame, level, 2, N * S, S, rays, ray_stride, nullptr, raw, xw, xw_row, 0, sp,
                                                                        num_cus(), st)
                       : audio ? sahs_field_radiance_bf16x3_launch(pk16, frame, level, N * S, S, rays, ray_stride, raw, xw, xw_row, sp, num_cus(), st)
                               : sahs_field_radiance_bf16x3_launch_nf(pk16, frame, level, N * S, S, rays, ray_stride, raw, xw, xw_row, sp, num_cus(), st);
            });
        return e ? hip_fail("sahs_model_field_forward_split", e) : 0;
    }
    if (precision != SAHS_F32 && !(precision == SAHS_BF16 && model == SAHS_MODEL_AUDIO))
        return fail(4, "sahs_model_field_forward_split: precision %s%ld is not built for this model", "", (long)precision);
    int e = probed(probe_kind(model, precision, level, mode), N * S, st, [&] {
        return precision == SAHS_BF16
                   ? sahs_field_forward_bf16w_split_launch((const float *)packed, frame, level, mode, N * S, S, rays, ray_stride, z, raw, xw, xw_row, xw_col0,
                                                           src, num_cus(), st)
               : model == SAHS_MODEL_AUDIO
                   ? sahs_field_forward_f32_split_launch((const float *)packed, frame, level, mode, N * S, S, rays, ray_stride, z, raw, xw, xw_row, xw_col0,
                                                         src, nullptr, num_cus(), st)
                   : sahs_field_forward_f32_split_launch_nf((const float *)packed, frame, level, mode, N * S, S, rays, ray_stride, z, raw, xw, xw_row,
                                                            xw_col0, src, nullptr, num_cus(), st);
    });
    return e ? hip_fail("sahs_model_field_forward_split", e) : 0;
}

// ---- training with the deformation nets evaluated once per depth: the split launches with saved activations, the backward cut at
// the (x', w) seam, and the routing of the fine pass's seam gradient through the merge permutation ----
long sahs_model_act_words_part(int model, int part)
{
    if (model < 0 || model > 2 || part < 0 || part > 3) return -1;
    const int p = part == 3 ? 0 : part;
    return model == SAHS_MODEL_AUDIO ? sahs_layout_act_part_words(p) : (model == SAHS_MODEL_NERFACE ? sahs_layout_act_part_words_nf(p) : sahs_layout_act_part_words_ns(p));
}
static long act_col0(int model, int part)
{
    const int p = part == 3 ? 0 : part;
    return model == SAHS_MODEL_AUDIO ? sahs_layout_act_part_col0(p) : (model == SAHS_MODEL_NERFACE ? sahs_layout_act_part_col0_nf(p) : sahs_layout_act_part_col0_ns(p));
}

int sahs_model_field_forward_split_save(int model, const void *packed, const float *frame, int level, int mode, long N, int S, const float *rays,
                                        int ray_stride, const float *z, float *raw, float *xw, int xw_row, int xw_col0, const int32_t *src,
                                        float *act_out, void *stream)
{
    const char *who = "sahs_model_field_forward_split_save";
    REQUIRE_MODEL(model, who);
    if (N == 0) return 0;
    if (model == SAHS_MODEL_NERFACE_STATIC) return fail(4, "%s: this model has no deformation nets%ld", who, 0L);
    REQUIRE(packed && frame && rays && xw && act_out && (level == 0 || level == 1) && N >= 0 && S >= 1 && ray_stride >= 8 && mode >= 0 && mode <= 2, who);
    REQUIRE((mode == 1 || raw) && (mode == 2 || z) && (mode != 2 || src), "sahs_model_field_forward_split_save(buffers of the mode)");
    REQUIRE(xw_col0 >= 0 && xw_row >= xw_col0 + (mode == 2 ? 0 : S) && ALIGNED16(xw) && ALIGNED16(packed) && ALIGNED16(frame) && (!raw || ALIGNED16(raw)) &&
            ALIGNED16(act_out), "sahs_model_field_forward_split_save(xw layout / alignment)");
    const long P = N * S;
    float *base = act_out - act_col0(model, mode) * P;       // column c of the act:: table at base + c * P; only the part's columns are touched
    int e = model == SAHS_MODEL_AUDIO
                ? sahs_field_forward_f32_split_launch((const float *)packed, frame, level, mode, P, S, rays, ray_stride, z, raw, xw, xw_row, xw_col0, src, base,
                                                      num_cus(), (hipStream_t)stream)
                : sahs_field_forward_f32_split_launch_nf((const float *)packed, frame, level, mode, P, S, rays, ray_stride, z, raw, xw, xw_row, xw_col0, src,
                                                         base, num_cus(), (hipStream_t)stream);
    return e ? hip_fail(who, e) : 0;
}

int sahs_model_field_backward_split(int model, const float *flat_params, const float *frame, int level, int part, long P, const float *act_in,
                                    const float *d_raw, const float *xw_grad_in, float *xw_grad_out, float *grad_flat, float *grad_cond,
                                    float *workspace, void *stream)
{
    const char *who = "sahs_model_field_backward_split";
    REQUIRE_MODEL(model, who);
    if (part == 0) part = 3;
    REQUIRE(flat_params && frame && act_in && grad_flat && grad_cond && workspace && part >= 1 && part <= 3, who);
    REQUIRE((level == 0 || level == 1) && P >= 0 && P <= 4000000L, "sahs_model_field_backward_split(0 <= P <= 4e6 samples per call)");
    REQUIRE(((part & 2) ? d_raw != nullptr : xw_grad_in != nullptr) && (part != 2 || xw_grad_out != nullptr),
            "sahs_model_field_backward_split(d_raw for the radiance part, xw_grad_in for the deformation part alone, xw_grad_out for the radiance part alone)");
    if (model == SAHS_MODEL_NERFACE_STATIC && part != 3) return fail(4, "%s: this model has no deformation nets%ld", who, 0L);
    const float *base = act_in - act_col0(model, part) * P;
    int e = model == SAHS_MODEL_AUDIO ? sahs_field_backward_split_launch(flat_params, frame, level, part, P, base, d_raw, xw_grad_in, xw_grad_out, grad_flat,
                                                                         grad_cond, workspace, (hipStream_t)stream)
            : model == SAHS_MODEL_NERFACE ? sahs_field_backward_split_launch_nf(flat_params, frame, level, part, P, base, d_raw, xw_grad_in, xw_grad_out,
                                                                                grad_flat, grad_cond, workspace, (hipStream_t)stream)
                                          : sahs_field_backward_split_launch_ns(flat_params, frame, level, part, P, base, d_raw, xw_grad_in, xw_grad_out,
                                                                                grad_flat, grad_cond, workspace, (hipStream_t)stream);
    return e ? hip_fail(who, e) : 0;
}

long sahs_model_bits_words_part(int model, int part)
{
    if (model < 0 || model > 2 || part < 0 || part > 3) return 0;
    const int p = part == 3 ? 0 : part;
    return model == SAHS_MODEL_AUDIO ? sahs_layout_bits_part_words(p) : (model == SAHS_MODEL_NERFACE ? sahs_layout_bits_part_words_nf(p) : sahs_layout_bits_part_words_ns(p));
}

static int split_bits_launch(int model, const float *packed, const float *frame, int level, int mode, long P, int S, const float *rays, int ray_stride,
                             const float *z, float *raw, float *xw, int xw_row, int xw_col0, const int32_t *src, float *base, uint32_t *bits, hipStream_t st)
{
    auto f = model == SAHS_MODEL_AUDIO ? sahs_field_forward_f32_split_bits_launch
                                       : (model == SAHS_MODEL_NERFACE ? sahs_field_forward_f32_split_bits_launch_nf : sahs_field_forward_f32_split_bits_launch_ns);
    return f(packed, frame, level, mode, P, S, rays, ray_stride, z, raw, xw, xw_row, xw_col0, src, base, bits, num_cus(), st);
}

// the whole-network training forward (sahs_model_field_forward_save) that also writes the sign-bit planes: the saving forward of the
// NeRFaceModel without deformation nets, whose training does not go through the split evaluation
int sahs_model_field_forward_save_bits(int model, const void *packed, const float *frame, int level, long N, int S, const float *rays, int ray_stride,
                                       const float *z, float *raw, float *act_out, uint32_t *bits_out, void *stream)
{
    const char *who = "sahs_model_field_forward_save_bits";
    REQUIRE_MODEL(model, who);
    REQUIRE(packed && frame && rays && z && raw && act_out && bits_out, who);
    REQUIRE((level == 0 || level == 1) && N >= 0 && S >= 1 && ray_stride >= 8, "sahs_model_field_forward_save_bits(shape)");
    REQUIRE(ALIGNED16(packed) && ALIGNED16(frame) && ALIGNED16(raw) && ALIGNED16(act_out) && ALIGNED16(bits_out), "sahs_model_field_forward_save_bits(alignment)");
    const long P = N * S;
    REQUIRE(P <= 4000000L, "sahs_model_field_forward_save_bits(at most 4e6 samples per call)");
    if (P == 0) return 0;
    int e = split_bits_launch(model, (const float *)packed, frame, level, 0, P, S, rays, ray_stride, z, raw, nullptr, 0, 0, nullptr, act_out, bits_out,
                              (hipStream_t)stream);
    return e ? hip_fail(who, e) : 0;
}

int sahs_model_field_forward_split_save_bits(int model, const void *packed, const float *frame, int level, int mode, long N, int S, const float *rays,
                                             int ray_stride, const float *z, float *raw, float *xw, int xw_row, int xw_col0, const int32_t *src,
                                             float *act_out, uint32_t *bits_out, void *stream)
{
    const char *who = "sahs_model_field_forward_split_save_bits";
    REQUIRE_MODEL(model, who);
    if (model == SAHS_MODEL_NERFACE_STATIC) return fail(4, "%s: this model has no deformation nets (its saving forward: sahs_model_field_forward_save_bits)%ld", who, 0L);
    if (N == 0) return 0;
    REQUIRE(packed && frame && rays && xw && act_out && bits_out && (level == 0 || level == 1) && N >= 0 && S >= 1 && ray_stride >= 8 && mode >= 0 && mode <= 2, who);
    REQUIRE((mode == 1 || raw) && (mode == 2 || z) && (mode != 2 || src), "sahs_model_field_forward_split_save_bits(buffers of the mode)");
    REQUIRE(xw_col0 >= 0 && xw_row >= xw_col0 + (mode == 2 ? 0 : S) && ALIGNED16(xw) && ALIGNED16(packed) && ALIGNED16(frame) && (!raw || ALIGNED16(raw)) &&
            ALIGNED16(act_out) && ALIGNED16(bits_out), "sahs_model_field_forward_split_save_bits(xw layout / alignment)");
    const long P = N * S;
    REQUIRE(P <= 4000000L, "sahs_model_field_forward_split_save_bits(at most 4e6 samples per call)");
    float *base = act_out - act_col0(model, mode) * P;
    int e = split_bits_launch(model, (const float *)packed, frame, level, mode, P, S, rays, ray_stride, z, raw, xw, xw_row, xw_col0, src, base, bits_out,
                              (hipStream_t)stream);
    return e ? hip_fail(who, e) : 0;
}

// the saving forward on the split-operand pipe: the buffers of sahs_model_field_forward_split_save_bits written by the SAHS_BF16X3 kernels
// (`packed` = that precision's weights), modes 1 and 2
int sahs_model_field_forward_split_save_bits_x3(int model, const void *packed, const float *frame, int level, int mode, long N, int S, const float *rays,
                                                int ray_stride, const float *z, float *raw, float *xw, int xw_row, int xw_col0, const int32_t *src,
                                                float *act_out, uint32_t *bits_out, void *stream)
{
    const char *who = "sahs_model_field_forward_split_save_bits_x3";
    REQUIRE_MODEL(model, who);
    if (model == SAHS_MODEL_NERFACE_STATIC)
        return fail(4, "%s: this model has no deformation nets (its saving forward on this pipe: sahs_model_field_forward_save_bits_x3)%ld", who, 0L);
    if (N == 0) return 0;
    REQUIRE(packed && frame && rays && xw && act_out && bits_out && (level == 0 || level == 1) && N >= 0 && S >= 1 && ray_stride >= 8 && (mode == 1 || mode == 2),
            "sahs_model_field_forward_split_save_bits_x3(mode 1 = deformation nets or 2 = radiance nets)");
    REQUIRE((mode == 1 || raw) && (mode == 2 || z) && (mode != 2 || src), "sahs_model_field_forward_split_save_bits_x3(buffers of the mode)");
    REQUIRE(xw_col0 >= 0 && xw_row >= xw_col0 + (mode == 2 ? 0 : S) && ALIGNED16(xw) && ALIGNED16(packed) && ALIGNED16(frame) && (!raw || ALIGNED16(raw)) &&
            ALIGNED16(act_out) && ALIGNED16(bits_out), "sahs_model_field_forward_split_save_bits_x3(xw layout / alignment)");
    const long P = N * S;
    REQUIRE(P <= 4000000L, "sahs_model_field_forward_split_save_bits_x3(at most 4e6 samples per call)");
    float *base = act_out - act_col0(model, mode) * P;
    hipStream_t st = (hipStream_t)stream;
    const bool audio = model == SAHS_MODEL_AUDIO;
    int e = probed(probe_kind(model, SAHS_BF16X3, level, mode), P, st, [&] {
        const float *pk = (const float *)packed;
        if (mode == 1)
            return (audio ? sahs_field_deform_bf16x3_save_launch : sahs_field_deform_bf16x3_save_launch_nf)(pk, frame, level, P, S, rays, ray_stride, z, xw, xw_row,
                                                                                                            xw_col0, base, bits_out, num_cus(), st);
        return (audio ? sahs_field_radiance_bf16x3_save_launch : sahs_field_radiance_bf16x3_save_launch_nf)(pk, frame, level, P, S, rays, ray_stride, raw, xw, xw_row,
                                                                                                            src, base, bits_out, num_cus(), st);
    });
    return e ? hip_fail(who, e) : 0;
}

// the whole-network saving forward on the split-operand pipe: the buffers of sahs_model_field_forward_save_bits written by the SAHS_BF16X3
// kernel (`packed` = that precision's weights).  The NeRFaceModel without deformation nets; the others save through the split form
int sahs_model_field_forward_save_bits_x3(int model, const void *packed, const float *frame, int level, long N, int S, const float *rays, int ray_stride,
                                          const float *z, float *raw, float *act_out, uint32_t *bits_out, void *stream)
{
    const char *who = "sahs_model_field_forward_save_bits_x3";
    REQUIRE_MODEL(model, who);
    if (model != SAHS_MODEL_NERFACE_STATIC)
        return fail(4, "%s: this model saves through the split chain on this pipe (sahs_model_field_forward_split_save_bits_x3)%ld", who, 0L);
    REQUIRE(packed && frame && rays && z && raw && act_out && bits_out, who);
    REQUIRE((level == 0 || level == 1) && N >= 0 && S >= 1 && ray_stride >= 8, "sahs_model_field_forward_save_bits_x3(shape)");
    REQUIRE(ALIGNED16(packed) && ALIGNED16(frame) && ALIGNED16(raw) && ALIGNED16(act_out) && ALIGNED16(bits_out), "sahs_model_field_forward_save_bits_x3(alignment)");
    const long P = N * S;
    REQUIRE(P <= 4000000L, "sahs_model_field_forward_save_bits_x3(at most 4e6 samples per call)");
    if (P == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    int e = probed(probe_kind(model, SAHS_BF16X3, level, 0), P, st, [&] {
        return sahs_field_forward_bf16x3_save_launch_ns((const float *)packed, frame, level, P, S, rays, ray_stride, z, raw, act_out, bits_out, num_cus(), st);
    });
    return e ? hip_fail(who, e) : 0;
}

long sahs_model_field_backward_fused_workspace_words(int model, int part, long P)
{
    if (model < 0 || model > 2 || part < 1 || part > 3 || P < 0) return -1;
    return model == SAHS_MODEL_AUDIO ? sahs_field_backward_fused_ws_words(part, P)
           : (model == SAHS_MODEL_NERFACE ? sahs_field_backward_fused_ws_words_nf(part, P) : sahs_field_backward_fused_ws_words_ns(part, P));
}

int sahs_model_field_backward_fused(int model, const float *flat_params, const float *frame, int level, int part, long P, const float *act_in,
                                    const uint32_t *bits_in, const float *d_raw, const float *xw_grad_in, float *xw_grad_out, float *grad_flat,
                                    float *grad_cond, float *workspace, void *stream)
{
    const char *who = "sahs_model_field_backward_fused";
    REQUIRE_MODEL(model, who);
    if (model == SAHS_MODEL_NERFACE_STATIC && part != 3) return fail(4, "%s: this model has no deformation nets%ld", who, 0L);
    REQUIRE(flat_params && frame && act_in && bits_in && grad_flat && grad_cond && workspace && part >= 1 && part <= 3, who);
    REQUIRE((level == 0 || level == 1) && P >= 0 && P <= 4000000L, "sahs_model_field_backward_fused(0 <= P <= 4e6 samples per call)");
    REQUIRE(((part & 2) ? d_raw != nullptr : xw_grad_in != nullptr) && (part != 2 || xw_grad_out != nullptr),
            "sahs_model_field_backward_fused(d_raw for the radiance part, xw_grad_in for the deformation part alone, xw_grad_out for the radiance part alone)");
    REQUIRE(ALIGNED16(act_in) && ALIGNED16(bits_in) && ALIGNED16(workspace) && (!d_raw || ALIGNED16(d_raw)) && (!xw_grad_in || ALIGNED16(xw_grad_in)) &&
            (!xw_grad_out || ALIGNED16(xw_grad_out)), "sahs_model_field_backward_fused(alignment)");
    if (P == 0) return 0;
    const float *base = act_in - act_col0(model, part) * P;
    auto f = model == SAHS_MODEL_AUDIO ? sahs_field_backward_fused_launch
                                       : (model == SAHS_MODEL_NERFACE ? sahs_field_backward_fused_launch_nf : sahs_field_backward_fused_launch_ns);
    int e = f(flat_params, frame, level, part, P, base, bits_in, d_raw, xw_grad_in, xw_grad_out, grad_flat, grad_cond, workspace, num_cus(), (hipStream_t)stream);
    return e ? hip_fail(who, e) : 0;
}

int sahs_route_xw_grad(long N, int Sc, int nf, const int32_t *src, const float *g_fine, float *g_coarse, float *g_new, void *stream)
{
    if (N == 0) return 0;
    REQUIRE(src && g_fine && g_coarse && g_new && N >= 0 && Sc >= 1 && nf >= 1 && ALIGNED16(g_fine) && ALIGNED16(g_coarse) && ALIGNED16(g_new),
            "sahs_route_xw_grad");
    int e = sahs_route_xw_grad_launch(N, Sc, nf, src, g_fine, g_coarse, g_new, (hipStream_t)stream);
    return e ? hip_fail("sahs_route_xw_grad", e) : 0;
}

long sahs_spade_modulate_workspace_words(long planes) { return planes > 0 ? sahs_spade_stats_words(planes) : 0; }

int sahs_spade_modulate(long planes, long hw, const float *x, const float *gamma, const float *beta, float eps, float slope, float *out,
                        float *stats, void *stream)
{
    if (planes == 0 || hw == 0) return 0;
    REQUIRE(planes > 0 && planes <= 2147483647L && hw > 0 && x && gamma && beta && out && stats && eps > 0.0f, "sahs_spade_modulate");
    int e = sahs_spade_modulate_launch(planes, hw, x, gamma, beta, eps, slope, out, stats, (hipStream_t)stream);
    return e ? hip_fail("sahs_spade_modulate", e) : 0;
}

int sahs_composite_forward_rows(long N, int S, const float *raw, const float *z, const float *rays, int ray_stride, const float *noise,
                                const float *bg, int white_background, float *weights, float *rows, int row_ld, int fine_pass, void *stream)
{
    if (N == 0) return 0;
    REQUIRE(raw && z && rays && weights && rows && ray_stride >= 6 && row_ld >= SAHS_ROW_COLUMNS, "sahs_composite_forward_rows");
    REQUIRE(N >= 0 && S >= 1 && S <= 256 && ALIGNED16(raw), "sahs_composite_forward_rows(shape: 1 <= S <= 256)");
    int e = fine_pass ? sahs_composite_forward_launch(N, S, raw, z, rays, ray_stride, noise, bg, white_background, rows + SAHS_ROW_RGB_F,
                                                      rows + SAHS_ROW_DISP_F, rows + SAHS_ROW_ACC_F, weights, rows + SAHS_ROW_DEPTH_F,
                                                      rows + SAHS_ROW_W_BG, row_ld, row_ld, (hipStream_t)stream)
                      : sahs_composite_forward_launch(N, S, raw, z, rays, ray_stride, noise, bg, white_background, rows + SAHS_ROW_RGB_C,
                                                      rows + SAHS_ROW_DISP_C, rows + SAHS_ROW_ACC_C, weights, nullptr, nullptr, row_ld,
                                                      row_ld, (hipStream_t)stream);
    return e ? hip_fail("sahs_composite_forward_rows", e) : 0;
}

int sahs_model_render_rays_rows(int model, const void *packed, const float *frame, int precision, long N, const float *rays,
                                int ray_stride, int Sc, int nf, int lindisp, int white_background, const float *bg, const float *t_rand,
                                const float *noise_c, const float *u, const float *noise_f, float *z_c, float *z_f, float *raw,
                                float *weights, float *rows, int row_ld, float *xw, int32_t *src, float *z_new, void *stream)
{
    REQUIRE_MODEL(model, "sahs_model_render_rays_rows");
    if (N == 0) return 0;
    REQUIRE(rows && row_ld >= SAHS_ROW_COLUMNS, "sahs_model_render_rays_rows(rows)");
    if (model != SAHS_MODEL_NERFACE_STATIC && ((precision == SAHS_BF16 && model == SAHS_MODEL_NERFACE) || precision == SAHS_BF16X3))
        REQUIRE(xw && src && z_new && nf > 0, "sahs_model_render_rays_rows(a mixed-precision model needs the xw / src / z_new workspace and nf > 0)");
    if (xw && src && z_new && nf > 0 && model != SAHS_MODEL_NERFACE_STATIC &&
        (precision == SAHS_F32 || precision == SAHS_BF16 || precision == SAHS_BF16X3
         )) {
        // the deformation nets are shared by the two levels and the fine depths contain the coarse ones: evaluate them once per depth
        const char *who = "sahs_model_render_rays_rows";
        REQUIRE(packed && frame && rays && z_c && z_f && raw && weights && Sc + nf <= 256, who);
        const int Sf = Sc + nf;
        hipStream_t st = (hipStream_t)stream;
        int e;
        if ((e = sahs_stratified_depths(N, Sc, rays, ray_stride, lindisp, t_rand, z_c, stream))) return e;
        if ((e = sahs_model_field_forward_split(model, packed, frame, precision, 0, 0, N, Sc, rays, ray_stride, z_c, raw, xw, Sf, 0, nullptr, stream))) return e;
        e = sahs_composite_forward_launch(N, Sc, raw, z_c, rays, ray_stride, noise_c, bg, white_background, rows + SAHS_ROW_RGB_C, rows + SAHS_ROW_DISP_C,
                                          rows + SAHS_ROW_ACC_C, weights, nullptr, nullptr, row_ld, row_ld, st);
        if (e) return hip_fail(who, e);
        if ((e = sahs_resample_merge(N, Sc, nf, z_c, weights, u, z_new, z_f, src, stream))) return e;
        if ((e = sahs_model_field_forward_split(model, packed, frame, precision, 1, 1, N, nf, rays, ray_stride, z_new, nullptr, xw, Sf, Sc, nullptr, stream))) return e;
        if ((e = sahs_model_field_forward_split(model, packed, frame, precision, 1, 2, N, Sf, rays, ray_stride, nullptr, raw, xw, Sf, 0, src, stream))) return e;
        e = sahs_composite_forward_launch(N, Sf, raw, z_f, rays, ray_stride, noise_f, bg, white_background, rows + SAHS_ROW_RGB_F, rows + SAHS_ROW_DISP_F,
                                          rows + SAHS_ROW_ACC_F, weights, rows + SAHS_ROW_DEPTH_F, rows + SAHS_ROW_W_BG, row_ld, row_ld, st);
        return e ? hip_fail(who, e) : 0;
    }
    field_fn_t f = model == SAHS_MODEL_AUDIO ? sahs_field_forward : (model == SAHS_MODEL_NERFACE ? field_nf : field_ns);
    return render_rays_chain(f, "sahs_model_render_rays_rows", packed, frame, precision, N, rays, ray_stride, Sc, nf, lindisp, white_background,
                             bg, t_rand, noise_c, u, noise_f, z_c, z_f, raw, weights, rows + SAHS_ROW_RGB_C, rows + SAHS_ROW_DISP_C,
                             rows + SAHS_ROW_ACC_C, rows + SAHS_ROW_RGB_F, rows + SAHS_ROW_DISP_F, rows + SAHS_ROW_ACC_F, rows + SAHS_ROW_W_BG,
                             rows + SAHS_ROW_DEPTH_F, stream, row_ld, row_ld);
}

}  // extern "C"
