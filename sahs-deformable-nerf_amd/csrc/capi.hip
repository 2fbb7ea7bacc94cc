// capi.hip -- the extern "C" boundary declared in include/sahs_nerf.h: argument validation,
// error text, and the chained predict_and_render_radiance launch sequence.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <vector>
#include "../../include/sahs_nerf.h"
#include "sahs_common.hpp"
#include "sahs_launchers.hpp"

static thread_local char g_err[512] = "";

__attribute__((format(printf, 2, 3))) static int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
static int hip_fail(const char *what, int e)
{
    snprintf(g_err, sizeof(g_err), "%s: HIP error %d (%s)", what, e, hipGetErrorString((hipError_t)e));
    return 100 + e;
}
#define REQUIRE(cond, name) do { if (!(cond)) return fail(1, "%s: invalid argument (capi.hip:%d)", name, __LINE__); } while (0)
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

// Where one composite writes its maps: as separate tensors (rgb rows of 15 floats, scalars contiguous), or as the coarse / fine columns of
// a rows buffer (include/sahs_nerf.h: SAHS_ROW_*).  depth and w_last may be null (a coarse pass that a fine pass follows writes neither).
struct CompositeOut {
    float *rgb, *disp, *acc, *depth, *w_last;
    int rgb_ld, sc_ld;
};
static CompositeOut composite_tensors(float *rgb, float *disp, float *acc, float *depth, float *w_last) { return {rgb, disp, acc, depth, w_last, 15, 1}; }
static CompositeOut composite_rows(float *rows, int row_ld, bool fine)
{
    if (fine) return {rows + SAHS_ROW_RGB_F, rows + SAHS_ROW_DISP_F, rows + SAHS_ROW_ACC_F, rows + SAHS_ROW_DEPTH_F, rows + SAHS_ROW_W_BG, row_ld, row_ld};
    return {rows + SAHS_ROW_RGB_C, rows + SAHS_ROW_DISP_C, rows + SAHS_ROW_ACC_C, nullptr, nullptr, row_ld, row_ld};
}
static int composite_launch(long N, int S, const float *raw, const float *z, const float *rays, int ray_stride, const float *noise, const float *bg,
                            int white_background, float *weights, const CompositeOut &o, hipStream_t st)
{
    return sahs_composite_forward_launch(N, S, raw, z, rays, ray_stride, noise, bg, white_background, o.rgb, o.disp, o.acc, weights, o.depth, o.w_last,
                                         o.rgb_ld, o.sc_ld, st);
}

int sahs_composite_forward(long N, int S, const float *raw, const float *z, const float *rays, int ray_stride, const float *noise,
                           const float *bg, int white_background, float *rgb, float *disp, float *acc, float *weights, float *depth,
                           void *stream)
{
    if (N == 0) return 0;
    REQUIRE(raw && z && rays && rgb && disp && acc && weights && depth && ray_stride >= 6, "sahs_composite_forward");
    REQUIRE(N >= 0 && S >= 1 && S <= 256 && ALIGNED16(raw), "sahs_composite_forward(shape: 1 <= S <= 256)");
    int e = composite_launch(N, S, raw, z, rays, ray_stride, noise, bg, white_background, weights, composite_tensors(rgb, disp, acc, depth, nullptr),
                             (hipStream_t)stream);
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

int sahs_route_xw_grad(long N, int Sc, int nf, const int32_t *src, const float *g_fine, float *g_coarse, float *g_new, void *stream)
{
    if (N == 0) return 0;
    REQUIRE(src && g_fine && g_coarse && g_new && N >= 0 && Sc >= 1 && nf >= 1 && ALIGNED16(g_fine) && ALIGNED16(g_coarse) && ALIGNED16(g_new),
            "sahs_route_xw_grad");
    int e = sahs_route_xw_grad_launch(N, Sc, nf, src, g_fine, g_coarse, g_new, (hipStream_t)stream);
    return e ? hip_fail("sahs_route_xw_grad", e) : 0;
}

// A float argument is taken as the SHORTEST decimal that rounds to it, read back in double: a caller writes beta2 = 0.999f and means 0.999
// (torch forms 1 - beta2 = 1.0000000000000009e-3 in double), while the float's own value gives 1 - 0.99900001287 = 9.99987e-4 -- 1.3e-5 relative off
// in every second-moment update, a hundred times the rounding error of the fp32 update itself.
static double decimal_double(float x)
{
    char buf[32];
    for (int digits = 1; digits <= 9; ++digits) {
        snprintf(buf, sizeof(buf), "%.*g", digits, (double)x);
        if (strtof(buf, nullptr) == x) return strtod(buf, nullptr);
    }
    return (double)x;
}

int sahs_adam_step(float *params, const float *grad, float *exp_avg, float *exp_avg_sq, long n, float lr, float beta1, float beta2, float eps,
                   long step, float grad_scale, void *stream)
{
    if (n == 0) return 0;
    REQUIRE(params && grad && exp_avg && exp_avg_sq && n > 0 && step >= 1, "sahs_adam_step");
    REQUIRE(std::isfinite(lr) && lr > 0.0f && std::isfinite(eps) && eps > 0.0f && std::isfinite(grad_scale), "sahs_adam_step(lr > 0, eps > 0, finite)");
    REQUIRE(beta1 >= 0.0f && beta1 < 1.0f && beta2 >= 0.0f && beta2 < 1.0f, "sahs_adam_step(0 <= beta < 1)");
    const uintptr_t p = reinterpret_cast<uintptr_t>(params), g = reinterpret_cast<uintptr_t>(grad), m = reinterpret_cast<uintptr_t>(exp_avg),
                    v = reinterpret_cast<uintptr_t>(exp_avg_sq), bytes = (uintptr_t)n * sizeof(float);
    REQUIRE(((p | g | m | v) & 3u) == 0, "sahs_adam_step(4-byte aligned buffers)");
    auto overlap = [bytes](uintptr_t a, uintptr_t b) { return a < b + bytes && b < a + bytes; };
    REQUIRE(!overlap(p, m) && !overlap(p, v) && !overlap(m, v), "sahs_adam_step(params, exp_avg, exp_avg_sq must not overlap)");
    const double b1 = decimal_double(beta1), b2 = decimal_double(beta2);
    const double bc1 = 1.0 - std::pow(b1, (double)step), bc2 = 1.0 - std::pow(b2, (double)step);
    int e = sahs_adam_step_launch(params, grad, exp_avg, exp_avg_sq, n, (float)(1.0 - b1), (float)b2, (float)(1.0 - b2),
                                  (float)(decimal_double(lr) / bc1), (float)std::sqrt(bc2), (float)decimal_double(eps), grad_scale,
                                  (hipStream_t)stream);
    return e ? hip_fail("sahs_adam_step", e) : 0;
}

long sahs_spade_modulate_workspace_words(long planes) { return planes > 0 ? sahs_spade_stats_words(planes) : 0; }
long sahs_spade_modulate_backward_workspace_words(long planes) { return planes > 0 ? sahs_spade_stats_words(planes) : 0; }

// the fp32 and the bf16 entries (tensors as bf16 bit patterns; stats / work stay fp32) validate alike and refuse under their own names
#define SPADE_REQUIRE(cond, what) do { if (!(cond)) return fail(1, "%s%s: invalid argument (capi.hip:%d)", who, what, __LINE__); } while (0)
static int spade_forward(const char *who, int bf16, long planes, long hw, const void *x, const void *gamma, const void *beta, float eps,
                         float slope, void *out, float *stats, void *stream)
{
    if (planes == 0 || hw == 0) return 0;
    SPADE_REQUIRE(planes > 0 && hw > 0 && x && gamma && beta && out && stats && eps > 0.0f, "");
    SPADE_REQUIRE(planes <= 65535, "(planes <= 65535: one plane per gridDim.y)");
    int e = sahs_spade_modulate_launch(planes, hw, x, gamma, beta, eps, slope, out, stats, bf16, (hipStream_t)stream);
    return e ? hip_fail(who, e) : 0;
}
static int spade_backward(const char *who, int bf16, long planes, long hw, const void *x, const void *gamma, const void *out, const float *stats,
                          const void *grad_out, float eps, float slope, void *dx, void *dgamma, void *dbeta, float *work, void *stream)
{
    if (planes == 0 || hw == 0) return 0;
    SPADE_REQUIRE(planes > 0 && hw > 0 && x && gamma && stats && grad_out && eps > 0.0f, "");
    SPADE_REQUIRE(planes <= 65535, "(planes <= 65535: one plane per gridDim.y)");
    SPADE_REQUIRE(slope >= 0.0f && (out || slope == 1.0f), "(slope >= 0; out may be null only for slope 1)");
    SPADE_REQUIRE(dx || dgamma || dbeta, "(at least one of dx, dgamma, dbeta)");
    SPADE_REQUIRE(work || !dx, "(dx needs the workspace)");
    int e = sahs_spade_modulate_backward_launch(planes, hw, x, gamma, slope == 1.0f ? nullptr : out, stats, grad_out, eps, slope, dx, dgamma, dbeta,
                                                work, bf16, (hipStream_t)stream);
    return e ? hip_fail(who, e) : 0;
}
static int spade_frozen(const char *who, int bf16, long batch, long channels, long h, long w, long map_batch, int up, const void *x,
                        const void *gamma, const void *beta, float eps, float slope, void *out, float *stats, void *stream)
{
    if (batch == 0 || channels == 0 || h == 0 || w == 0) return 0;
    SPADE_REQUIRE(batch > 0 && channels > 0 && h > 0 && w > 0 && x && gamma && beta && out && stats && eps > 0.0f, "");
    SPADE_REQUIRE(up == 0 || up == 1, "(up is 0 or 1)");
    SPADE_REQUIRE(map_batch == 1 || map_batch == batch, "(gamma and beta have a batch of 1, shared by every frame, or of `batch`)");
    SPADE_REQUIRE(channels <= 65535, "(channels <= 65535: one channel per gridDim.y; the batch is not limited)");
    int e = sahs_spade_modulate_frozen_launch(batch, channels, map_batch == 1, h, w, up, x, gamma, beta, eps, slope, out, stats, bf16,
                                              (hipStream_t)stream);
    return e ? hip_fail(who, e) : 0;
}
#undef SPADE_REQUIRE

long sahs_spade_modulate_frozen_workspace_words(long batch, long channels)
{
    return batch > 0 && channels > 0 ? sahs_spade_stats_words(batch * channels) : 0;
}
int sahs_spade_modulate_frozen(long batch, long channels, long h, long w, long map_batch, int up, const float *x, const float *gamma,
                               const float *beta, float eps, float slope, float *out, float *stats, void *stream)
{
    return spade_frozen("sahs_spade_modulate_frozen", 0, batch, channels, h, w, map_batch, up, x, gamma, beta, eps, slope, out, stats, stream);
}
int sahs_spade_modulate_frozen_bf16(long batch, long channels, long h, long w, long map_batch, int up, const unsigned short *x,
                                    const unsigned short *gamma, const unsigned short *beta, float eps, float slope, unsigned short *out,
                                    float *stats, void *stream)
{
    return spade_frozen("sahs_spade_modulate_frozen_bf16", 1, batch, channels, h, w, map_batch, up, x, gamma, beta, eps, slope, out, stats,
                        stream);
}

int sahs_spade_modulate(long planes, long hw, const float *x, const float *gamma, const float *beta, float eps, float slope, float *out,
                        float *stats, void *stream)
{
    return spade_forward("sahs_spade_modulate", 0, planes, hw, x, gamma, beta, eps, slope, out, stats, stream);
}
int sahs_spade_modulate_backward(long planes, long hw, const float *x, const float *gamma, const float *out, const float *stats,
                                 const float *grad_out, float eps, float slope, float *dx, float *dgamma, float *dbeta, float *work, void *stream)
{
    return spade_backward("sahs_spade_modulate_backward", 0, planes, hw, x, gamma, out, stats, grad_out, eps, slope, dx, dgamma, dbeta, work, stream);
}
int sahs_spade_modulate_bf16(long planes, long hw, const unsigned short *x, const unsigned short *gamma, const unsigned short *beta, float eps,
                             float slope, unsigned short *out, float *stats, void *stream)
{
    return spade_forward("sahs_spade_modulate_bf16", 1, planes, hw, x, gamma, beta, eps, slope, out, stats, stream);
}
int sahs_spade_modulate_backward_bf16(long planes, long hw, const unsigned short *x, const unsigned short *gamma, const unsigned short *out,
                                      const float *stats, const unsigned short *grad_out, float eps, float slope, unsigned short *dx,
                                      unsigned short *dgamma, unsigned short *dbeta, float *work, void *stream)
{
    return spade_backward("sahs_spade_modulate_backward_bf16", 1, planes, hw, x, gamma, out, stats, grad_out, eps, slope, dx, dgamma, dbeta, work,
                          stream);
}

// the fused, batched spectral norm: the tables are host arrays of device pointers; every refusal names what it refuses
static int spectral_norm_shapes(const char *who, int jobs, const int *h, const int *w)
{
    if (jobs < 1 || jobs > SAHS_SPECTRAL_NORM_MAX_JOBS)
        return fail(1, "%s: jobs = %d, must be 1 .. %d (capi.hip:%d)", who, jobs, SAHS_SPECTRAL_NORM_MAX_JOBS, __LINE__);
    if (!h || !w) return fail(1, "%s: null pointer for the table h or w (capi.hip:%d)", who, __LINE__);
    for (int k = 0; k < jobs; ++k)
        if (h[k] < 1 || w[k] < 1 || (long)h[k] * w[k] >= 2147483648L)
            return fail(1, "%s: job %d is %d x %d, needs h >= 1, w >= 1, h * w < 2^31 (capi.hip:%d)", who, k, h[k], w[k], __LINE__);
    return 0;
}
#define SN_TABLE(who, t) do { if (!(t)) return fail(1, "%s: null pointer for the table %s (capi.hip:%d)", who, #t, __LINE__); \
    for (int k_ = 0; k_ < jobs; ++k_) if (!(t)[k_]) return fail(1, "%s: null pointer %s[%d] (capi.hip:%d)", who, #t, k_, __LINE__); } while (0)

int sahs_spectral_norm_forward(int jobs, const float *const *W, float *const *u, float *const *v, void *const *out, float *const *saved,
                               const int *h, const int *w, int out_bf16, int power_iteration, float eps, void *stream)
{
    const char *who = "sahs_spectral_norm_forward";
    if (int e = spectral_norm_shapes(who, jobs, h, w)) return e;
    SN_TABLE(who, W); SN_TABLE(who, u); SN_TABLE(who, v); SN_TABLE(who, out); SN_TABLE(who, saved);
    if (!(eps > 0.0f)) return fail(1, "%s: eps = %g, must be > 0 (capi.hip:%d)", who, (double)eps, __LINE__);
    if (power_iteration != 0 && power_iteration != 1)
        return fail(1, "%s: power_iteration = %d, must be 0 (eval) or 1 (training) (capi.hip:%d)", who, power_iteration, __LINE__);
    int e = sahs_spectral_norm_forward_launch(jobs, W, u, v, out, saved, h, w, out_bf16 != 0, power_iteration, eps, (hipStream_t)stream);
    return e ? hip_fail(who, e) : 0;
}

int sahs_spectral_norm_backward(int jobs, const float *const *W, const float *const *saved, const void *const *grad_out, float *const *dW,
                                const int *h, const int *w, int grad_bf16, void *stream)
{
    const char *who = "sahs_spectral_norm_backward";
    if (int e = spectral_norm_shapes(who, jobs, h, w)) return e;
    SN_TABLE(who, W); SN_TABLE(who, saved); SN_TABLE(who, grad_out); SN_TABLE(who, dW);
    int e = sahs_spectral_norm_backward_launch(jobs, W, saved, grad_out, dW, h, w, grad_bf16 != 0, (hipStream_t)stream);
    return e ? hip_fail(who, e) : 0;
}

// image metrics: every refusal names what it refuses, before any HIP call
static bool image_metrics_shape(long B, int H, int W, int C)
{
    return B >= 0 && H >= 7 && W >= 7 && H <= 32768 && W <= 32768 && C >= 1 && C <= 4 && B * sahs_image_metrics_tiles(H, W) < 2147483648L;
}

size_t sahs_image_metrics_workspace_bytes(long B, int H, int W, int C)
{
    return image_metrics_shape(B, H, W, C) ? (size_t)B * (size_t)sahs_image_metrics_tiles(H, W) * (size_t)(C + 2) * sizeof(double) : 0;
}

int sahs_image_metrics(const void *a, const void *b, int dtype, long B, int H, int W, int C, const long *stride_a, const long *stride_b,
                       double ssim_data_range, double *out, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "sahs_image_metrics";
    if (dtype != SAHS_IMAGE_U8 && dtype != SAHS_IMAGE_F32)
        return fail(1, "%s: dtype = %d, must be SAHS_IMAGE_U8 (0) or SAHS_IMAGE_F32 (1) (capi.hip:%d)", who, dtype, __LINE__);
    if (H < 7 || W < 7 || H > 32768 || W > 32768)
        return fail(1, "%s: images of %d x %d pixels, the 7 x 7 window needs 7 <= H, W (<= 32768) (capi.hip:%d)", who, H, W, __LINE__);
    if (C < 1 || C > 4) return fail(1, "%s: C = %d channels, must be 1 .. 4 (capi.hip:%d)", who, C, __LINE__);
    if (!image_metrics_shape(B, H, W, C))
        return fail(1, "%s: B = %ld images, needs B >= 0 and B * tiles < 2^31 (capi.hip:%d)", who, B, __LINE__);
    if (!(ssim_data_range > 0.0) || !std::isfinite(ssim_data_range))
        return fail(1, "%s: ssim_data_range = %g, must be finite and > 0 (capi.hip:%d)", who, ssim_data_range, __LINE__);
    if (B == 0) return 0;
    if (!a || !b || !stride_a || !stride_b || !out || !workspace)
        return fail(1, "%s: null pointer for %s (capi.hip:%d)", who, !a ? "a" : !b ? "b" : !stride_a ? "stride_a" : !stride_b ? "stride_b" :
                    !out ? "out" : "workspace", __LINE__);
    for (int k = 0; k < 4; ++k)
        if (stride_a[k] < 0 || stride_b[k] < 0)
            return fail(1, "%s: stride %d is negative (%ld, %ld) (capi.hip:%d)", who, k, stride_a[k], stride_b[k], __LINE__);
    const uintptr_t elem = dtype == SAHS_IMAGE_F32 ? 3u : 0u;
    if (((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & elem) != 0)
        return fail(1, "%s: a and b must be aligned to their 4-byte elements (capi.hip:%d)", who, __LINE__);
    if (((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(workspace)) & 7u) != 0)
        return fail(1, "%s: out and workspace must be 8-byte aligned (capi.hip:%d)", who, __LINE__);
    const size_t need = sahs_image_metrics_workspace_bytes(B, H, W, C);
    if (workspace_bytes < need)
        return fail(1, "%s: workspace of %zu bytes, needs %zu (sahs_image_metrics_workspace_bytes) (capi.hip:%d)", who, workspace_bytes, need, __LINE__);
    int e = sahs_image_metrics_launch(a, b, dtype == SAHS_IMAGE_F32, B, H, W, C, stride_a, stride_b, ssim_data_range, out,
                                      static_cast<double *>(workspace), (hipStream_t)stream);
    return e ? hip_fail(who, e) : 0;
}

// image loss: every refusal names what it refuses, before any HIP call
static bool image_loss_shape(long B, int H, int W, int C)
{
    return B >= 0 && H >= 7 && W >= 7 && H <= 32768 && W <= 32768 && C >= 1 && C <= 4 && B * sahs_image_loss_tiles(H, W) < 2147483648L;
}

size_t sahs_image_loss_workspace_bytes(long B, int H, int W, int C)
{
    return image_loss_shape(B, H, W, C) ? (size_t)B * (size_t)sahs_image_loss_tiles(H, W) * (size_t)(C + 2) * sizeof(double) : 0;
}

int sahs_image_loss(const float *pred, const float *target, long B, int H, int W, int C, const long *stride_pred, const long *stride_target,
                    double w_l2, double w_l1, double w_ssim, int clamp, double ssim_data_range, float *grad, const long *stride_grad,
                    double *out, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "sahs_image_loss";
    if (H < 7 || W < 7 || H > 32768 || W > 32768)
        return fail(1, "%s: images of %d x %d pixels, the 7 x 7 window needs 7 <= H, W (<= 32768) (capi.hip:%d)", who, H, W, __LINE__);
    if (C < 1 || C > 4) return fail(1, "%s: C = %d channels, must be 1 .. 4 (capi.hip:%d)", who, C, __LINE__);
    if (!image_loss_shape(B, H, W, C))
        return fail(1, "%s: B = %ld images, needs B >= 0 and B * tiles < 2^31 (capi.hip:%d)", who, B, __LINE__);
    if (!std::isfinite(w_l2) || !std::isfinite(w_l1) || !std::isfinite(w_ssim))
        return fail(1, "%s: weights w_l2 = %g, w_l1 = %g, w_ssim = %g, must be finite (capi.hip:%d)", who, w_l2, w_l1, w_ssim, __LINE__);
    if (!(ssim_data_range > 0.0) || !std::isfinite(ssim_data_range))
        return fail(1, "%s: ssim_data_range = %g, must be finite and > 0 (capi.hip:%d)", who, ssim_data_range, __LINE__);
    if (B == 0) return 0;
    if (!pred || !target || !stride_pred || !stride_target || !out || !workspace || (grad && !stride_grad))
        return fail(1, "%s: null pointer for %s (capi.hip:%d)", who, !pred ? "pred" : !target ? "target" : !stride_pred ? "stride_pred" :
                    !stride_target ? "stride_target" : !out ? "out" : !workspace ? "workspace" : "stride_grad (grad asked for)", __LINE__);
    for (int k = 0; k < 4; ++k)
        if (stride_pred[k] < 0 || stride_target[k] < 0 || (grad && stride_grad[k] < 0))
            return fail(1, "%s: stride %d is negative (%ld, %ld, grad %ld) (capi.hip:%d)", who, k, stride_pred[k], stride_target[k],
                        grad ? stride_grad[k] : 0L, __LINE__);
    if (((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(target)) & 3u) != 0)
        return fail(1, "%s: pred and target must be aligned to their 4-byte elements (capi.hip:%d)", who, __LINE__);
    if ((reinterpret_cast<uintptr_t>(grad) & 3u) != 0)
        return fail(1, "%s: grad must be aligned to its 4-byte elements (capi.hip:%d)", who, __LINE__);
    if (((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(workspace)) & 7u) != 0)
        return fail(1, "%s: out and workspace must be 8-byte aligned (capi.hip:%d)", who, __LINE__);
    const size_t need = sahs_image_loss_workspace_bytes(B, H, W, C);
    if (workspace_bytes < need)
        return fail(1, "%s: workspace of %zu bytes, needs %zu (sahs_image_loss_workspace_bytes) (capi.hip:%d)", who, workspace_bytes, need, __LINE__);
    int e = sahs_image_loss_launch(pred, target, B, H, W, C, stride_pred, stride_target, w_l2, w_l1, w_ssim, clamp, ssim_data_range, grad,
                                   stride_grad, out, static_cast<double *>(workspace), (hipStream_t)stream);
    return e ? hip_fail(who, e) : 0;
}

// frame products: every refusal names what it refuses, before any HIP call
static bool frame_products_shape(long B, int H, int W)
{
    return B >= 0 && H >= 1 && W >= 1 && H <= 32768 && W <= 32768 && B * sahs_frame_products_tiles(H, W) < 2147483648L;
}

size_t sahs_frame_products_workspace_bytes(long B, int H, int W)
{
    return frame_products_shape(B, H, W) ? (size_t)B * (size_t)sahs_frame_products_tiles(H, W) * 16u : 0;
}

int sahs_frame_products(const float *rgb, int C, const long *stride_rgb, const float *disp, const float *w_bg, const float *intrinsics,
                        long B, int H, int W, int clean, int central_difference, unsigned char *image, unsigned char *seg,
                        unsigned char *normals_u8, float *normals_f32, unsigned char *disparity, void *workspace, size_t workspace_bytes,
                        void *stream)
{
    const char *who = "sahs_frame_products";
    if (H < 1 || W < 1 || H > 32768 || W > 32768)
        return fail(1, "%s: frames of %d x %d pixels, needs 1 <= H, W <= 32768 (capi.hip:%d)", who, H, W, __LINE__);
    if (C != 3 && C != 15)
        return fail(1, "%s: C = %d channels, must be 3 (rgb) or 15 (rgb and the 12 class scores) (capi.hip:%d)", who, C, __LINE__);
    if (!frame_products_shape(B, H, W))
        return fail(1, "%s: B = %ld frames, needs B >= 0 and B * tiles < 2^31 (capi.hip:%d)", who, B, __LINE__);
    if (seg && C != 15)
        return fail(1, "%s: seg asked for with C = 3: the mask colours need the 12 class scores, C = 15 (capi.hip:%d)", who, __LINE__);
    if ((normals_u8 || normals_f32) && (!disp || !intrinsics))
        return fail(1, "%s: normals asked for without %s: the normal map needs disp and the intrinsics [fx, fy, cx, cy] (capi.hip:%d)", who,
                    !disp ? "disp" : "intrinsics", __LINE__);
    if (disparity && !disp) return fail(1, "%s: disparity asked for without disp (capi.hip:%d)", who, __LINE__);
    if ((image || seg) && (!rgb || !stride_rgb))
        return fail(1, "%s: image or seg asked for with a null %s (capi.hip:%d)", who, !rgb ? "rgb" : "stride_rgb", __LINE__);
    if (stride_rgb)
        for (int k = 0; k < 3; ++k)
            if (stride_rgb[k] < 0) return fail(1, "%s: stride %d is negative (%ld) (capi.hip:%d)", who, k, stride_rgb[k], __LINE__);
    if (intrinsics && (!std::isfinite(intrinsics[0]) || !std::isfinite(intrinsics[1]) || intrinsics[0] == 0.0f || intrinsics[1] == 0.0f))
        return fail(1, "%s: intrinsics fx = %g, fy = %g, must be finite and not 0 (capi.hip:%d)", who, (double)intrinsics[0],
                    (double)intrinsics[1], __LINE__);
    if (B == 0) return 0;
    if (((reinterpret_cast<uintptr_t>(rgb) | reinterpret_cast<uintptr_t>(disp) | reinterpret_cast<uintptr_t>(w_bg) |
          reinterpret_cast<uintptr_t>(normals_f32)) & 3u) != 0)
        return fail(1, "%s: rgb, disp, w_bg and normals_f32 must be aligned to their 4-byte elements (capi.hip:%d)", who, __LINE__);
    if (disparity) {
        if (!workspace) return fail(1, "%s: null pointer for workspace (disparity asked for) (capi.hip:%d)", who, __LINE__);
        if ((reinterpret_cast<uintptr_t>(workspace) & 15u) != 0) return fail(1, "%s: workspace must be 16-byte aligned (capi.hip:%d)", who, __LINE__);
        const size_t need = sahs_frame_products_workspace_bytes(B, H, W);
        if (workspace_bytes < need)
            return fail(1, "%s: workspace of %zu bytes, needs %zu (sahs_frame_products_workspace_bytes) (capi.hip:%d)", who, workspace_bytes, need,
                        __LINE__);
    }
    const int d = central_difference ? 2 : 1;
    if (H <= d || W <= d) { normals_u8 = nullptr; normals_f32 = nullptr; }      // an empty plane: nothing to write
    if (!image && !seg && !normals_u8 && !normals_f32 && !disparity) return 0;
    int e = sahs_frame_products_launch(rgb, C, stride_rgb, disp, clean ? w_bg : nullptr, intrinsics, B, H, W, clean, central_difference, image, seg,
                                       normals_u8, normals_f32, disparity, workspace, (hipStream_t)stream);
    return e ? hip_fail(who, e) : 0;
}

// LPIPS, the scaling layer and the distance head, and their backward: every refusal names what it refuses, before any HIP call
static int lpips_prepare_checked(const char *who, const char *na, const char *nb, const void *a, const void *b, int a_is_float, int b_is_float,
                                 long B, int H, int W, int C, const long *stride_a, const long *stride_b, int normalize, int clamp, float *out,
                                 void *stream)
{
    if (C != 3) return fail(1, "%s: C = %d channels, LPIPS scores RGB images: C must be 3 (capi.hip:%d)", who, C, __LINE__);
    if (H < SAHS_LPIPS_MIN_SIDE || W < SAHS_LPIPS_MIN_SIDE || H > 32768 || W > 32768)
        return fail(1, "%s: images of %d x %d pixels, AlexNet's second max-pool needs %d <= H, W (<= 32768) (capi.hip:%d)", who, H, W,
                    SAHS_LPIPS_MIN_SIDE, __LINE__);
    if (B < 0 || 2 * B * (long)H * W >= 2147483648L * 256)
        return fail(1, "%s: B = %ld images, needs B >= 0 and 2 B H W < 2^39 (capi.hip:%d)", who, B, __LINE__);
    if (B == 0) return 0;
    if (!a || !b || !stride_a || !stride_b || !out)
        return fail(1, "%s: null pointer for %s%s (capi.hip:%d)", who, a && b && (!stride_a || !stride_b) ? "stride_" : "",
                    !a ? na : !b ? nb : !stride_a ? na : !stride_b ? nb : "out", __LINE__);
    for (int k = 0; k < 4; ++k)
        if (stride_a[k] < 0 || stride_b[k] < 0)
            return fail(1, "%s: stride %d is negative (%ld, %ld) (capi.hip:%d)", who, k, stride_a[k], stride_b[k], __LINE__);
    if ((reinterpret_cast<uintptr_t>(a) & (a_is_float ? 3u : 0u)) != 0 || (reinterpret_cast<uintptr_t>(b) & (b_is_float ? 3u : 0u)) != 0 ||
        (reinterpret_cast<uintptr_t>(out) & 3u) != 0)
        return fail(1, "%s: %s, %s and out must be aligned to their 4-byte elements (capi.hip:%d)", who, na, nb, __LINE__);
    int e = sahs_lpips_prepare_launch(a, b, a_is_float, b_is_float, B, H, W, stride_a, stride_b, normalize != 0, clamp != 0, out, (hipStream_t)stream);
    return e ? hip_fail(who, e) : 0;
}

int sahs_lpips_prepare(const void *a, const void *b, int dtype, long B, int H, int W, int C, const long *stride_a, const long *stride_b,
                       int normalize, float *out, void *stream)
{
    const char *who = "sahs_lpips_prepare";
    if (dtype != SAHS_IMAGE_U8 && dtype != SAHS_IMAGE_F32)
        return fail(1, "%s: dtype = %d, must be SAHS_IMAGE_U8 (0) or SAHS_IMAGE_F32 (1) (capi.hip:%d)", who, dtype, __LINE__);
    const int f = dtype == SAHS_IMAGE_F32;
    return lpips_prepare_checked(who, "a", "b", a, b, f, f, B, H, W, C, stride_a, stride_b, normalize, 0, out, stream);
}

int sahs_lpips_prepare_loss(const float *pred, const void *target, int target_dtype, long B, int H, int W, int C, const long *stride_pred,
                            const long *stride_target, int normalize, int clamp, float *out, void *stream)
{
    const char *who = "sahs_lpips_prepare_loss";
    if (target_dtype != SAHS_IMAGE_U8 && target_dtype != SAHS_IMAGE_F32)
        return fail(1, "%s: target_dtype = %d, must be SAHS_IMAGE_U8 (0) or SAHS_IMAGE_F32 (1) (capi.hip:%d)", who, target_dtype, __LINE__);
    return lpips_prepare_checked(who, "pred", "target", pred, target, 1, target_dtype == SAHS_IMAGE_F32, B, H, W, C, stride_pred, stride_target,
                                 normalize, clamp, out, stream);
}

int sahs_lpips_prepare_grad(const float *pred, const float *gx, long B, int H, int W, int C, const long *stride_pred, int normalize, int clamp,
                            float *grad, const long *stride_grad, void *stream)
{
    const char *who = "sahs_lpips_prepare_grad";
    if (C != 3) return fail(1, "%s: C = %d channels, LPIPS scores RGB images: C must be 3 (capi.hip:%d)", who, C, __LINE__);
    if (H < SAHS_LPIPS_MIN_SIDE || W < SAHS_LPIPS_MIN_SIDE || H > 32768 || W > 32768)
        return fail(1, "%s: images of %d x %d pixels, AlexNet's second max-pool needs %d <= H, W (<= 32768) (capi.hip:%d)", who, H, W,
                    SAHS_LPIPS_MIN_SIDE, __LINE__);
    if (B < 0 || 2 * B * (long)H * W >= 2147483648L * 256)
        return fail(1, "%s: B = %ld images, needs B >= 0 and 2 B H W < 2^39 (capi.hip:%d)", who, B, __LINE__);
    if (B == 0) return 0;
    if (!pred || !gx || !stride_pred || !grad || !stride_grad)
        return fail(1, "%s: null pointer for %s (capi.hip:%d)", who, !pred ? "pred" : !gx ? "gx" : !stride_pred ? "stride_pred" : !grad ? "grad" :
                    "stride_grad", __LINE__);
    for (int k = 0; k < 4; ++k)
        if (stride_pred[k] < 0 || stride_grad[k] < 0)
            return fail(1, "%s: stride %d is negative (%ld, grad %ld) (capi.hip:%d)", who, k, stride_pred[k], stride_grad[k], __LINE__);
    if (((reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(gx) | reinterpret_cast<uintptr_t>(grad)) & 3u) != 0)
        return fail(1, "%s: pred, gx and grad must be aligned to their 4-byte elements (capi.hip:%d)", who, __LINE__);
    int e = sahs_lpips_prepare_grad_launch(pred, gx, B, H, W, stride_pred, normalize != 0, clamp != 0, grad, stride_grad, (hipStream_t)stream);
    return e ? hip_fail(who, e) : 0;
}

static bool lpips_distance_shape(int jobs, long B, const long *hw)
{
    if (jobs < 1 || jobs > SAHS_LPIPS_MAX_JOBS || B < 0 || !hw) return false;
    for (int k = 0; k < jobs; ++k)
        if (hw[k] < 1 || hw[k] > (1L << 30)) return false;
    return B * sahs_lpips_distance_tiles(jobs, hw) < 2147483648L;
}

size_t sahs_lpips_distance_workspace_bytes(int jobs, long B, const long *hw)
{
    return lpips_distance_shape(jobs, B, hw) ? (size_t)B * (size_t)sahs_lpips_distance_tiles(jobs, hw) * sizeof(double) : 0;
}

size_t sahs_lpips_head_stats_bytes(int jobs, long B, const long *hw)
{
    return lpips_distance_shape(jobs, B, hw) ? (size_t)B * (size_t)sahs_lpips_head_pixels(jobs, hw) * 3u * sizeof(double) : 0;
}

// the job table of the head's entries: 0, or the refusal's code.  ta, tb: the names of the two feature tables (tb null: one table)
static int lpips_head_tables(const char *who, int jobs, const float *const *fa, const char *ta, const float *const *fb, const char *tb,
                             const float *const *weights, const int *C, const long *hw, long B, bool *empty)
{
    *empty = false;
    if (jobs < 1 || jobs > SAHS_LPIPS_MAX_JOBS)
        return fail(1, "%s: jobs = %d, must be 1 .. %d (capi.hip:%d)", who, jobs, SAHS_LPIPS_MAX_JOBS, __LINE__);
    if (!C || !hw) return fail(1, "%s: null pointer for the table %s (capi.hip:%d)", who, !C ? "C" : "hw", __LINE__);
    for (int k = 0; k < jobs; ++k) {
        if (C[k] < 1 || C[k] > SAHS_LPIPS_MAX_CHANNELS)
            return fail(1, "%s: job %d has C = %d channels, must be 1 .. %d (capi.hip:%d)", who, k, C[k], SAHS_LPIPS_MAX_CHANNELS, __LINE__);
        if (hw[k] < 1 || hw[k] > (1L << 30))
            return fail(1, "%s: job %d has hw = %ld pixels, must be 1 .. 2^30 (capi.hip:%d)", who, k, hw[k], __LINE__);
    }
    if (!lpips_distance_shape(jobs, B, hw))
        return fail(1, "%s: B = %ld images, needs B >= 0 and B * tiles < 2^31 (capi.hip:%d)", who, B, __LINE__);
    if (B == 0) { *empty = true; return 0; }
    if (!fa || (tb && !fb) || !weights)
        return fail(1, "%s: null pointer for %s (capi.hip:%d)", who, !fa ? ta : (tb && !fb) ? tb : "weights", __LINE__);
    for (int k = 0; k < jobs; ++k) {
        if (!fa[k] || (tb && !fb[k]) || !weights[k])
            return fail(1, "%s: null pointer %s[%d] (capi.hip:%d)", who, !fa[k] ? ta : (tb && !fb[k]) ? tb : "weights", k, __LINE__);
        if (((reinterpret_cast<uintptr_t>(fa[k]) | (tb ? reinterpret_cast<uintptr_t>(fb[k]) : 0u) | reinterpret_cast<uintptr_t>(weights[k])) & 3u) != 0)
            return tb ? fail(1, "%s: %s[%d], %s[%d] and weights[%d] must be aligned to their 4-byte elements (capi.hip:%d)", who, ta, k, tb, k, k,
                             __LINE__)
                      : fail(1, "%s: %s[%d] and weights[%d] must be aligned to their 4-byte elements (capi.hip:%d)", who, ta, k, k, __LINE__);
    }
    return 0;
}

int sahs_lpips_distance(int jobs, const float *const *features, const float *const *weights, const int *C, const long *hw, long B,
                        double *out, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "sahs_lpips_distance";
    bool empty;
    if (int code = lpips_head_tables(who, jobs, features, "features", nullptr, nullptr, weights, C, hw, B, &empty)) return code;
    if (empty) return 0;
    if (!out || !workspace) return fail(1, "%s: null pointer for %s (capi.hip:%d)", who, !out ? "out" : "workspace", __LINE__);
    if (((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(workspace)) & 7u) != 0)
        return fail(1, "%s: out and workspace must be 8-byte aligned (capi.hip:%d)", who, __LINE__);
    const size_t need = sahs_lpips_distance_workspace_bytes(jobs, B, hw);
    if (workspace_bytes < need)
        return fail(1, "%s: workspace of %zu bytes, needs %zu (sahs_lpips_distance_workspace_bytes) (capi.hip:%d)", who, workspace_bytes, need,
                    __LINE__);
    const float *second[SAHS_LPIPS_MAX_JOBS];      // rows [B, 2B) of each tensor
    for (int k = 0; k < jobs; ++k) second[k] = features[k] + B * C[k] * hw[k];
    int e = sahs_lpips_head_forward_launch(jobs, features, second, weights, C, hw, B, out, nullptr, static_cast<double *>(workspace),
                                           (hipStream_t)stream);
    return e ? hip_fail(who, e) : 0;
}

int sahs_lpips_head_forward(int jobs, const float *const *fa, const float *const *fb, const float *const *weights, const int *C, const long *hw,
                            long B, double *out, double *stats, size_t stats_bytes, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "sahs_lpips_head_forward";
    bool empty;
    if (int code = lpips_head_tables(who, jobs, fa, "fa", fb, "fb", weights, C, hw, B, &empty)) return code;
    if (empty) return 0;
    if (!out || !workspace) return fail(1, "%s: null pointer for %s (capi.hip:%d)", who, !out ? "out" : "workspace", __LINE__);
    if (((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(stats)) & 7u) != 0)
        return fail(1, "%s: out, stats and workspace must be 8-byte aligned (capi.hip:%d)", who, __LINE__);
    const size_t need = sahs_lpips_distance_workspace_bytes(jobs, B, hw), need_stats = sahs_lpips_head_stats_bytes(jobs, B, hw);
    if (workspace_bytes < need)
        return fail(1, "%s: workspace of %zu bytes, needs %zu (sahs_lpips_distance_workspace_bytes) (capi.hip:%d)", who, workspace_bytes, need,
                    __LINE__);
    if (stats && stats_bytes < need_stats)
        return fail(1, "%s: stats of %zu bytes, needs %zu (sahs_lpips_head_stats_bytes) (capi.hip:%d)", who, stats_bytes, need_stats, __LINE__);
    int e = sahs_lpips_head_forward_launch(jobs, fa, fb, weights, C, hw, B, out, stats, static_cast<double *>(workspace), (hipStream_t)stream);
    return e ? hip_fail(who, e) : 0;
}

int sahs_lpips_head_backward(int jobs, const float *const *fa, const float *const *fb, const float *const *weights, const int *C, const long *hw,
                             long B, const void *g, int g_is_double, const double *stats, size_t stats_bytes, float *const *grad_a, void *stream)
{
    const char *who = "sahs_lpips_head_backward";
    bool empty;
    if (int code = lpips_head_tables(who, jobs, fa, "fa", fb, "fb", weights, C, hw, B, &empty)) return code;
    if (empty) return 0;
    if (!g || !stats || !grad_a) return fail(1, "%s: null pointer for %s (capi.hip:%d)", who, !g ? "g" : !stats ? "stats" : "grad_a", __LINE__);
    for (int k = 0; k < jobs; ++k) {
        if (!grad_a[k]) return fail(1, "%s: null pointer grad_a[%d] (capi.hip:%d)", who, k, __LINE__);
        if ((reinterpret_cast<uintptr_t>(grad_a[k]) & 3u) != 0)
            return fail(1, "%s: grad_a[%d] must be aligned to its 4-byte elements (capi.hip:%d)", who, k, __LINE__);
    }
    if ((reinterpret_cast<uintptr_t>(stats) & 7u) != 0 || (reinterpret_cast<uintptr_t>(g) & (g_is_double ? 7u : 3u)) != 0)
        return fail(1, "%s: stats must be 8-byte aligned and g aligned to its %d-byte elements (capi.hip:%d)", who, g_is_double ? 8 : 4, __LINE__);
    const size_t need_stats = sahs_lpips_head_stats_bytes(jobs, B, hw);
    if (stats_bytes < need_stats)
        return fail(1, "%s: stats of %zu bytes, needs %zu (sahs_lpips_head_stats_bytes) (capi.hip:%d)", who, stats_bytes, need_stats, __LINE__);
    int e = sahs_lpips_head_backward_launch(jobs, fa, fb, weights, C, hw, B, g, g_is_double != 0, stats, grad_a, (hipStream_t)stream);
    return e ? hip_fail(who, e) : 0;
}

int sahs_composite_forward_rows(long N, int S, const float *raw, const float *z, const float *rays, int ray_stride, const float *noise,
                                const float *bg, int white_background, float *weights, float *rows, int row_ld, int fine_pass, void *stream)
{
    if (N == 0) return 0;
    REQUIRE(raw && z && rays && weights && rows && ray_stride >= 6 && row_ld >= SAHS_ROW_COLUMNS, "sahs_composite_forward_rows");
    REQUIRE(N >= 0 && S >= 1 && S <= 256 && ALIGNED16(raw), "sahs_composite_forward_rows(shape: 1 <= S <= 256)");
    int e = composite_launch(N, S, raw, z, rays, ray_stride, noise, bg, white_background, weights, composite_rows(rows, row_ld, fine_pass != 0),
                             (hipStream_t)stream);
    return e ? hip_fail("sahs_composite_forward_rows", e) : 0;
}

// ---- every built architecture in one table row: the per-model entries the ABI reaches (nullptr: that model's build has none) ----
// model: SAHS_MODEL_AUDIO, SAHS_MODEL_NERFACE (config/expression/person_2|3.yml),
// SAHS_MODEL_NERFACE_STATIC (config/expression/person_1.yml: no warp, no hyper sheet).
enum Kernel { K_NONE, K_F32, K_BF16, K_X3 };         // the field kernel a launch runs on (ModelFns::field)
enum Pack { PK_NONE, PK_F32, PK_BF16, PK_X3 };      // the weight packings of a model build (pack.hip): fp32, bf16 stream, hi/lo streams
typedef int (*pack_fn)(const float *, float *, hipStream_t);
struct ModelFns {
    bool deformation_nets;
    long (*param_count)(void);
    long (*frame_words)(void);
    long (*act_words)(void);
    long (*packed_words[4])(void);      // per Pack
    pack_fn pack[4];
    long (*executed_macs)(int, int);
    int (*act_part_words)(int);
    int (*act_part_col0)(int);
    int (*bits_part_words)(int);
    int (*fold)(const float *, const float *, const float *, int, float *, hipStream_t);
    int (*bwd_gemm_precision_state)(int);
    int (*bf16w_exact_leaky_state)(int);
    // the field forward of each Kernel (field_f32.hip, field_bf16w.hip, field_bf16x3.hip): a FieldLaunch and its mode
    int (*field[4])(const FieldLaunch *, int);
    // ... and the inference render's sparse branches: the one-launch pass, the bytes of a record workspace and the slots a pass's rings need
    decltype(&sahs_field_f32_sparse_launch) f32_sparse;
    decltype(&sahs_field_f32_sparse_ws_bytes) f32_sparse_ws_bytes;
    decltype(&sahs_field_f32_sparse_ring_slots) f32_sparse_ring_slots;
    // backward (field_bwd.hip): per-layer walk, cut at the (x', w) seam, fused walk
    long (*bwd_ws_words)(long);
    decltype(&sahs_field_backward_launch) bwd;
    decltype(&sahs_field_backward_split_launch) bwd_split;
    long (*fused_ws_words)(int, long);
    decltype(&sahs_field_backward_fused_launch) bwd_fused;
};
#define SAHS_MODEL_ROW(sfx, deform)                                                                                                    \
    deform, sahs_layout_param_count##sfx, sahs_layout_frame_words##sfx, sahs_layout_act_words##sfx,                                 \
        {nullptr, sahs_layout_packed_words_f32##sfx, sahs_layout_packed_words_bf16##sfx, sahs_layout_packed_words_bf16x3##sfx},      \
        {nullptr, sahs_pack_weights_f32_launch##sfx, sahs_pack_weights_bf16_launch##sfx, sahs_pack_weights_bf16x3_launch##sfx},      \
        sahs_layout_executed_macs##sfx, sahs_layout_act_part_words##sfx, sahs_layout_act_part_col0##sfx, sahs_layout_bits_part_words##sfx, \
        sahs_fold_conditioning_launch##sfx, sahs_bwd_gemm_precision_state##sfx, sahs_bf16w_exact_leaky_state##sfx,                  \
        {nullptr, sahs_field_f32_launch##sfx, sahs_field_bf16w_launch##sfx, sahs_field_bf16x3_launch##sfx},                          \
        sahs_field_f32_sparse_launch##sfx, sahs_field_f32_sparse_ws_bytes##sfx, sahs_field_f32_sparse_ring_slots##sfx,               \
        sahs_field_backward_ws_words##sfx, sahs_field_backward_launch##sfx, sahs_field_backward_split_launch##sfx,                  \
        sahs_field_backward_fused_ws_words##sfx, sahs_field_backward_fused_launch##sfx
static const ModelFns kModels[3] = {{SAHS_MODEL_ROW(, true)}, {SAHS_MODEL_ROW(_nf, true)}, {SAHS_MODEL_ROW(_ns, false)}};
#undef SAHS_MODEL_ROW

// ---- every (model, precision) pair, described once ----
struct Pipe {
    Pack seg[3];        // the packed buffer: these packings back to back from word 0, each at a 16-byte boundary (none: not built)
    Kernel whole;       // the whole-network launch (sahs_model_field_forward); K_NONE: the pair exists only as the split chain
    Kernel split;       // the split evaluation (sahs_model_field_forward_split) as one launch per mode
    Kernel chain;       // ... or as the split chain: the deformation nets on the split-operand kernel (SAHS_X3_DEFORM=f32: on the fp32
                        // kernel), then the radiance nets on this one
    int def_prec, def_x, rad_prec, rad_x;      // executed MACs per part: the layer program of this precision (pack.hip) x MFMAs per product
};
static const Pipe kPipes[3][4] = {
    {   // SAHS_MODEL_AUDIO
        {{PK_F32}, K_F32, K_F32, K_NONE, SAHS_F32, 1, SAHS_F32, 1},
        {{PK_BF16}, K_BF16, K_BF16, K_NONE, SAHS_BF16, 1, SAHS_BF16, 1},
        {{}, K_NONE, K_NONE, K_NONE, SAHS_BF16, 1, SAHS_BF16, 1},      // precision id 2: not built, priced as the bf16 layer program
        {{PK_X3, PK_F32}, K_NONE, K_NONE, K_X3, SAHS_BF16, 3, SAHS_BF16, 3},
    },
    {   // SAHS_MODEL_NERFACE; SAHS_BF16 is mixed: split-operand deformation nets, bf16 radiance nets
        {{PK_F32}, K_F32, K_F32, K_NONE, SAHS_F32, 1, SAHS_F32, 1},
        {{PK_BF16, PK_F32, PK_X3}, K_NONE, K_NONE, K_BF16, SAHS_BF16, 3, SAHS_BF16, 1},
        {{}, K_NONE, K_NONE, K_NONE, SAHS_BF16, 1, SAHS_BF16, 1},
        {{PK_X3, PK_F32}, K_NONE, K_NONE, K_X3, SAHS_BF16, 3, SAHS_BF16, 3},
    },
    {   // SAHS_MODEL_NERFACE_STATIC: no deformation nets (its layer program prices part 1 at 0), no split evaluation
        {{PK_F32}, K_F32, K_NONE, K_NONE, SAHS_F32, 1, SAHS_F32, 1},
        {{PK_BF16}, K_BF16, K_NONE, K_NONE, SAHS_BF16, 1, SAHS_BF16, 1},
        {{}, K_NONE, K_NONE, K_NONE, SAHS_BF16, 1, SAHS_BF16, 1},
        {{PK_X3}, K_X3, K_NONE, K_NONE, SAHS_BF16, 3, SAHS_BF16, 3},
    },
};
static const Pipe *pipe_of(int model, int precision) { return precision >= 0 && precision <= 3 ? &kPipes[model][precision] : nullptr; }
// the pair's packed layout: off[k] = word offset of packing k; returns the total words (-1: the pair is not built)
static long packed_layout(int model, const Pipe *p, long off[4])
{
    long end = -1;
    for (int i = 0; p && i < 3 && p->seg[i] != PK_NONE; ++i) {
        off[p->seg[i]] = end < 0 ? 0 : (end + 3) / 4 * 4;
        end = off[p->seg[i]] + kModels[model].packed_words[p->seg[i]]();
    }
    return end;
}
// SAHS_X3_DEFORM=f32 (read once): the split chains' deformation launches run on the fp32 kernel instead of the split-operand one (A/B aid)
static bool x3_deform_on_f32()
{
    static const bool v = getenv("SAHS_X3_DEFORM") != nullptr && strcmp(getenv("SAHS_X3_DEFORM"), "f32") == 0;
    return v;
}
static long act_col0(int model, int part) { return kModels[model].act_part_col0(part == 3 ? 0 : part); }
#define REQUIRE_MODEL(m, name) do { if ((m) < 0 || (m) > 2) return fail(3, "%s: unknown model %d", name, (int)(m)); } while (0)

long sahs_param_count(void) { return sahs_model_param_count(SAHS_MODEL_AUDIO); }
long sahs_packed_words(int precision) { return sahs_model_packed_words(SAHS_MODEL_AUDIO, precision); }
long sahs_frame_words(void) { return sahs_model_frame_words(SAHS_MODEL_AUDIO); }
long sahs_act_words_per_sample(void) { return sahs_model_act_words_per_sample(SAHS_MODEL_AUDIO); }
long sahs_field_backward_workspace_words(long P) { return sahs_model_field_backward_workspace_words(SAHS_MODEL_AUDIO, P); }

long sahs_model_param_count(int model) { return (model < 0 || model > 2) ? -1 : kModels[model].param_count(); }
long sahs_model_frame_words(int model) { return (model < 0 || model > 2) ? -1 : kModels[model].frame_words(); }
long sahs_model_act_words_per_sample(int model) { return (model < 0 || model > 2) ? -1 : kModels[model].act_words(); }
long sahs_model_field_backward_workspace_words(int model, long P) { return (model < 0 || model > 2) ? -1 : kModels[model].bwd_ws_words(P); }
long sahs_model_packed_words(int model, int precision)
{
    long off[4];
    return (model < 0 || model > 2) ? -1 : packed_layout(model, pipe_of(model, precision), off);
}
long sahs_model_executed_macs_part(int model, int precision, int part)
{
    if (model < 0 || model > 2 || precision < SAHS_F32 || precision > SAHS_BF16X3 || part < 0 || part > 2) return -1;
    const ModelFns &m = kModels[model];
    const Pipe &p = kPipes[model][precision];
    // priced as what is issued: with SAHS_X3_DEFORM=f32 the chain's deformation launches are the fp32 kernel's
    const long def = p.chain != K_NONE && x3_deform_on_f32() ? m.executed_macs(SAHS_F32, 1) : p.def_x * m.executed_macs(p.def_prec, 1);
    const long rad = p.rad_x * m.executed_macs(p.rad_prec, 2);
    return (part != 2 ? def : 0) + (part != 1 ? rad : 0);
}
long sahs_model_executed_macs_per_sample(int model, int precision) { return sahs_model_executed_macs_part(model, precision, 0); }
long sahs_model_act_words_part(int model, int part)
{
    return (model < 0 || model > 2 || part < 0 || part > 3) ? -1 : kModels[model].act_part_words(part == 3 ? 0 : part);
}
long sahs_model_bits_words_part(int model, int part)
{
    return (model < 0 || model > 2 || part < 0 || part > 3) ? 0 : kModels[model].bits_part_words(part == 3 ? 0 : part);
}
long sahs_model_field_backward_fused_workspace_words(int model, int part, long P)
{
    return (model < 0 || model > 2 || part < 1 || part > 3 || P < 0) ? -1 : kModels[model].fused_ws_words(part, P);
}

int sahs_backward_gemm_precision(int precision)
{
    if (precision < 0) return kModels[SAHS_MODEL_AUDIO].bwd_gemm_precision_state(-1) ? SAHS_BF16X3 : SAHS_F32;
    if (precision != SAHS_F32 && precision != SAHS_BF16X3) return -1;
    for (const ModelFns &m : kModels) m.bwd_gemm_precision_state(precision == SAHS_BF16X3 ? 3 : 0);
    return precision;
}

int sahs_bf16_exact_leaky(int enable)
{
    if (enable < 0) return kModels[SAHS_MODEL_AUDIO].bf16w_exact_leaky_state(-1);
    int r = 0;
    for (int i = 2; i >= 0; --i) r = kModels[i].bf16w_exact_leaky_state(enable);      // the AudioFaceModel's answer
    return r;
}

static int pack_weights(const char *who, int model, const float *flat_params, void *packed, int precision, void *stream)
{
    REQUIRE(flat_params && packed && ALIGNED16(packed), who);
    long off[4];
    if (packed_layout(model, pipe_of(model, precision), off) < 0) return fail(2, "%s: precision %d is not built for this model", who, precision);
    int e = 0;
    for (Pack s : kPipes[model][precision].seg)
        if (s != PK_NONE && !e) e = kModels[model].pack[s](flat_params, (float *)packed + off[s], (hipStream_t)stream);
    return e ? hip_fail(who, e) : 0;
}
int sahs_pack_weights(const float *flat_params, void *packed, int precision, void *stream)
{
    return pack_weights("sahs_pack_weights", SAHS_MODEL_AUDIO, flat_params, packed, precision, stream);
}
int sahs_model_pack_weights(int model, const float *flat_params, void *packed, int precision, void *stream)
{
    REQUIRE_MODEL(model, "sahs_model_pack_weights");
    return pack_weights("sahs_model_pack_weights", model, flat_params, packed, precision, stream);
}

static int fold_conditioning(const char *who, int model, const float *flat_params, const float *driving, const float *pose, int pose_ld,
                             float *frame, void *stream)
{
    REQUIRE(flat_params && driving && pose && frame && pose_ld >= 4 && ALIGNED16(frame), who);
    int e = kModels[model].fold(flat_params, driving, pose, pose_ld, frame, (hipStream_t)stream);
    return e ? hip_fail(who, e) : 0;
}
int sahs_fold_conditioning(const float *flat_params, const float *audio, const float *pose, int pose_ld, float *frame, void *stream)
{
    return fold_conditioning("sahs_fold_conditioning", SAHS_MODEL_AUDIO, flat_params, audio, pose, pose_ld, frame, stream);
}
int sahs_model_fold_conditioning(int model, const float *flat_params, const float *driving, const float *pose, int pose_ld, float *frame,
                                 void *stream)
{
    REQUIRE_MODEL(model, "sahs_model_fold_conditioning");
    return fold_conditioning("sahs_model_fold_conditioning", model, flat_params, driving, pose, pose_ld, frame, stream);
}

// the whole network, one launch
static int field_forward(const char *who, int model, const void *packed, const float *frame, int level, long N, int S, const float *rays,
                         int ray_stride, const float *z, float *raw, float *dbg, int precision, void *stream)
{
    if (N == 0) return 0;
    REQUIRE(packed && frame && rays && z && raw, who);
    REQUIRE((level == 0 || level == 1) && N >= 0 && S >= 1 && ray_stride >= 8, who);
    REQUIRE(ALIGNED16(packed) && ALIGNED16(frame) && ALIGNED16(raw) && (!dbg || ALIGNED16(dbg)), who);
    const Pipe *p = pipe_of(model, precision);
    long off[4];
    if (packed_layout(model, p, off) < 0) return fail(2, "%s: precision %d is not built for this model", who, precision);
    if (p->whole == K_NONE)
        return fail(2, "%s: precision %d of this model runs through sahs_model_field_forward_split / sahs_model_render_rays_rows (it needs the "
                       "xw workspace)", who, precision);
    hipStream_t st = (hipStream_t)stream;
    const FieldLaunch L{.packed = (const float *)packed, .frame = frame, .level = level, .P = N * S, .S = S, .rays = rays, .ray_stride = ray_stride,
                        .zvals = z, .raw = raw, .dbg = dbg, .num_cu = num_cus(), .stream = st};      // (the split-operand kernels have no debug planes)
    int e = probed(probe_kind(model, precision, level, 0), N * S, st, [&] { return kModels[model].field[p->whole](&L, 0); });
    return e ? hip_fail(who, e) : 0;
}
int sahs_field_forward(const void *packed, const float *frame, int level, long N, int S, const float *rays, int ray_stride,
                       const float *z, float *raw, float *dbg, int precision, void *stream)
{
    return field_forward("sahs_field_forward", SAHS_MODEL_AUDIO, packed, frame, level, N, S, rays, ray_stride, z, raw, dbg, precision, stream);
}
int sahs_model_field_forward(int model, const void *packed, const float *frame, int level, long N, int S, const float *rays, int ray_stride,
                             const float *z, float *raw, float *dbg, int precision, void *stream)
{
    REQUIRE_MODEL(model, "sahs_model_field_forward");
    return field_forward("sahs_model_field_forward", model, packed, frame, level, N, S, rays, ray_stride, z, raw, dbg, precision, stream);
}

/* The split evaluation of the field (csrc/field_f32.hip, MODE): 0 whole network + x', w written to xw; 1 deformation nets only;
 * 2 radiance net only, x', w fetched from xw through src. */
int sahs_model_field_forward_split(int model, const void *packed, const float *frame, int precision, int level, int mode, long N, int S,
                                   const float *rays, int ray_stride, const float *z, float *raw, float *xw, int xw_row, int xw_col0,
                                   const int32_t *src, void *stream)
{
    const char *who = "sahs_model_field_forward_split";
    REQUIRE_MODEL(model, who);
    if (N == 0) return 0;
    const ModelFns &m = kModels[model];
    if (!m.deformation_nets) return fail(4, "%s: this model has no deformation nets", who);
    REQUIRE(packed && frame && rays && xw && (level == 0 || level == 1) && N >= 0 && S >= 1 && ray_stride >= 8 && mode >= 0 && mode <= 2, who);
    const Pipe *p = pipe_of(model, precision);
    const bool chain = p && p->chain != K_NONE;
    REQUIRE((mode == 1 || raw) && (mode == 2 || z) && (mode != 2 || src || chain), who);      // (the buffers of the mode)
    REQUIRE(xw_col0 >= 0 && xw_row >= xw_col0 + (mode == 2 ? 0 : S) && ALIGNED16(xw) && ALIGNED16(packed) && ALIGNED16(frame) && (!raw || ALIGNED16(raw)),
            who);
    const float *pk = (const float *)packed;
    const long P = N * S;
    hipStream_t st = (hipStream_t)stream;
    FieldLaunch L{.packed = pk, .frame = frame, .level = level, .P = P, .S = S, .rays = rays, .ray_stride = ray_stride, .zvals = z, .raw = raw,
                  .xw = xw, .xw_row = xw_row, .xw_col0 = xw_col0, .src = mode == 2 ? src : nullptr, .num_cu = num_cus(), .stream = st};
    int e = 0;
    if (chain) {      // deformation launch, then radiance launch (mode 0 = both, one after the other)
        REQUIRE(mode != 0 || xw_col0 == 0, who);
        long off[4];
        packed_layout(model, p, off);
        if (mode != 2) {
            const bool f32 = x3_deform_on_f32();
            L.packed = pk + off[f32 ? PK_F32 : PK_X3];
            e = probed(probe_kind(model, f32 ? SAHS_F32 : SAHS_BF16X3, level, 1), P, st, [&] { return m.field[f32 ? K_F32 : K_X3](&L, 1); });
        }
        if (!e && mode != 1) {
            L.packed = pk + off[p->chain == K_BF16 ? PK_BF16 : PK_X3];
            e = probed(probe_kind(model, precision, level, 2), P, st, [&] { return m.field[p->chain](&L, 2); });
        }
        return e ? hip_fail(who, e) : 0;
    }
    if (!p || p->split == K_NONE) return fail(4, "%s: precision %d is not built for this model", who, precision);
    e = probed(probe_kind(model, precision, level, mode), P, st, [&] { return m.field[p->split](&L, mode); });
    return e ? hip_fail(who, e) : 0;
}

// ---- training with the deformation nets evaluated once per depth: the split launches with saved activations, the backward cut at
// the (x', w) seam, and the routing of the fine pass's seam gradient through the merge permutation ----

// The seven saving forwards (the training forward that keeps its activations, column c of the act:: table at base + c * P; a split form
// touches only its part's columns), validated once and launched through the table.  A form is: whole network or split evaluation
// (mode, xw, src); fp32 kernel or split-operand kernels (x3: probed, modes 1 and 2 when split, the static model only when whole); with
// or without sign-bit planes.  Where the public entry points always differed, they still do, by that last flag:
//   - the forms with sign bits cap P at 4e6; the others take any P;
//   - whole network: with sign bits, P == 0 returns 0 after the checks; without, it reaches the launcher;
//   - split: N == 0 returns 0 before the checks; without sign bits, before the no-deformation-nets check too (which then answers 0, not 4).
struct SaveForm {
    const char *who;
    bool split, x3, bits;
};
static int field_forward_save(const SaveForm &f, int model, const void *packed, const float *frame, int level, int mode, long N, int S,
                              const float *rays, int ray_stride, const float *z, float *raw, float *xw, int xw_row, int xw_col0,
                              const int32_t *src, float *act_out, uint32_t *bits_out, void *stream)
{
    const char *who = f.who;
    REQUIRE_MODEL(model, who);
    const ModelFns &m = kModels[model];
    if (f.split && !f.bits && N == 0) return 0;
    if (f.split && !m.deformation_nets)
        return fail(4, "%s: this model has no deformation nets (its saving forward: sahs_model_field_forward_save%s)", who,
                    f.x3 ? "_bits_x3" : (f.bits ? "_bits" : ""));
    if (!f.split && f.x3 && m.deformation_nets)
        return fail(4, "%s: this model saves through the split chain on this pipe (sahs_model_field_forward_split_save_bits_x3)", who);
    if (f.split && N == 0) return 0;
    REQUIRE(packed && frame && rays && act_out && (!f.bits || bits_out) && (f.split ? xw != nullptr : z && raw), who);
    REQUIRE((level == 0 || level == 1) && N >= 0 && S >= 1 && ray_stride >= 8, who);
    if (f.split) {
        REQUIRE(f.x3 ? (mode == 1 || mode == 2) : (mode >= 0 && mode <= 2), who);
        REQUIRE((mode == 1 || raw) && (mode == 2 || z) && (mode != 2 || src), who);      // (the buffers of the mode)
        REQUIRE(xw_col0 >= 0 && xw_row >= xw_col0 + (mode == 2 ? 0 : S) && ALIGNED16(xw), who);
    }
    REQUIRE(ALIGNED16(packed) && ALIGNED16(frame) && (!raw || ALIGNED16(raw)) && ALIGNED16(act_out) && (!f.bits || ALIGNED16(bits_out)), who);
    const long P = N * S;
    REQUIRE(!f.bits || P <= 4000000L, who);      // (at most 4e6 samples per call)
    if (!f.split && f.bits && P == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    // (a whole-network form has mode 0, no xw and no src; column 0 of its part is column 0 of the table: the base is act_out)
    const FieldLaunch L{.packed = (const float *)packed, .frame = frame, .level = level, .P = P, .S = S, .rays = rays, .ray_stride = ray_stride,
                        .zvals = z, .raw = raw, .xw = xw, .xw_row = xw_row, .xw_col0 = xw_col0, .src = src,
                        .actbuf = act_out - act_col0(model, mode) * P, .bits = bits_out, .num_cu = num_cus(), .stream = st};
    int e = f.x3 ? probed(probe_kind(model, SAHS_BF16X3, level, mode), P, st, [&] { return m.field[K_X3](&L, mode); })
                 : m.field[K_F32](&L, mode);
    return e ? hip_fail(who, e) : 0;
}

int sahs_field_forward_save(const void *packed, const float *frame, int level, long N, int S, const float *rays, int ray_stride,
                            const float *z, float *raw, float *act_out, void *stream)
{
    return field_forward_save({"sahs_field_forward_save", false, false, false}, SAHS_MODEL_AUDIO, packed, frame, level, 0, N, S, rays,
                              ray_stride, z, raw, nullptr, 0, 0, nullptr, act_out, nullptr, stream);
}
int sahs_model_field_forward_save(int model, const void *packed, const float *frame, int level, long N, int S, const float *rays,
                                  int ray_stride, const float *z, float *raw, float *act_out, void *stream)
{
    return field_forward_save({"sahs_model_field_forward_save", false, false, false}, model, packed, frame, level, 0, N, S, rays, ray_stride,
                              z, raw, nullptr, 0, 0, nullptr, act_out, nullptr, stream);
}
// the whole-network saving forward that also writes the sign-bit planes: the NeRFaceModel without deformation nets, whose training does
// not go through the split evaluation
int sahs_model_field_forward_save_bits(int model, const void *packed, const float *frame, int level, long N, int S, const float *rays, int ray_stride,
                                       const float *z, float *raw, float *act_out, uint32_t *bits_out, void *stream)
{
    return field_forward_save({"sahs_model_field_forward_save_bits", false, false, true}, model, packed, frame, level, 0, N, S, rays,
                              ray_stride, z, raw, nullptr, 0, 0, nullptr, act_out, bits_out, stream);
}
// ... on the split-operand pipe (`packed` = the SAHS_BF16X3 pack): the NeRFaceModel without deformation nets; the others save through
// the split form
int sahs_model_field_forward_save_bits_x3(int model, const void *packed, const float *frame, int level, long N, int S, const float *rays, int ray_stride,
                                          const float *z, float *raw, float *act_out, uint32_t *bits_out, void *stream)
{
    return field_forward_save({"sahs_model_field_forward_save_bits_x3", false, true, true}, model, packed, frame, level, 0, N, S, rays,
                              ray_stride, z, raw, nullptr, 0, 0, nullptr, act_out, bits_out, stream);
}
int sahs_model_field_forward_split_save(int model, const void *packed, const float *frame, int level, int mode, long N, int S, const float *rays,
                                        int ray_stride, const float *z, float *raw, float *xw, int xw_row, int xw_col0, const int32_t *src,
                                        float *act_out, void *stream)
{
    return field_forward_save({"sahs_model_field_forward_split_save", true, false, false}, model, packed, frame, level, mode, N, S, rays,
                              ray_stride, z, raw, xw, xw_row, xw_col0, src, act_out, nullptr, stream);
}
int sahs_model_field_forward_split_save_bits(int model, const void *packed, const float *frame, int level, int mode, long N, int S, const float *rays,
                                             int ray_stride, const float *z, float *raw, float *xw, int xw_row, int xw_col0, const int32_t *src,
                                             float *act_out, uint32_t *bits_out, void *stream)
{
    return field_forward_save({"sahs_model_field_forward_split_save_bits", true, false, true}, model, packed, frame, level, mode, N, S, rays,
                              ray_stride, z, raw, xw, xw_row, xw_col0, src, act_out, bits_out, stream);
}
// ... on the split-operand pipe (`packed` = the SAHS_BF16X3 pack), modes 1 and 2
int sahs_model_field_forward_split_save_bits_x3(int model, const void *packed, const float *frame, int level, int mode, long N, int S, const float *rays,
                                                int ray_stride, const float *z, float *raw, float *xw, int xw_row, int xw_col0, const int32_t *src,
                                                float *act_out, uint32_t *bits_out, void *stream)
{
    return field_forward_save({"sahs_model_field_forward_split_save_bits_x3", true, true, true}, model, packed, frame, level, mode, N, S, rays,
                              ray_stride, z, raw, xw, xw_row, xw_col0, src, act_out, bits_out, stream);
}

static int field_backward(const char *who, int model, const float *flat_params, const float *frame, int level, long P, const float *act_in,
                          const float *d_raw, float *grad_flat, float *grad_cond, float *workspace, void *stream)
{
    REQUIRE(flat_params && frame && act_in && d_raw && grad_flat && grad_cond && workspace, who);
    REQUIRE((level == 0 || level == 1) && P >= 0 && P <= 4000000L, who);      // (0 <= P <= 4e6 samples per call)
    int e = kModels[model].bwd(flat_params, frame, level, P, act_in, d_raw, grad_flat, grad_cond, workspace, (hipStream_t)stream);
    return e ? hip_fail(who, e) : 0;
}
int sahs_field_backward(const float *flat_params, const float *frame, int level, long P, const float *act_in, const float *d_raw,
                        float *grad_flat, float *grad_cond, float *workspace, void *stream)
{
    return field_backward("sahs_field_backward", SAHS_MODEL_AUDIO, flat_params, frame, level, P, act_in, d_raw, grad_flat, grad_cond,
                          workspace, stream);
}
int sahs_model_field_backward(int model, const float *flat_params, const float *frame, int level, long P, const float *act_in,
                              const float *d_raw, float *grad_flat, float *grad_cond, float *workspace, void *stream)
{
    REQUIRE_MODEL(model, "sahs_model_field_backward");
    return field_backward("sahs_model_field_backward", model, flat_params, frame, level, P, act_in, d_raw, grad_flat, grad_cond, workspace,
                          stream);
}

int sahs_model_field_backward_split(int model, const float *flat_params, const float *frame, int level, int part, long P, const float *act_in,
                                    const float *d_raw, const float *xw_grad_in, float *xw_grad_out, float *grad_flat, float *grad_cond,
                                    float *workspace, void *stream)
{
    const char *who = "sahs_model_field_backward_split";
    REQUIRE_MODEL(model, who);
    if (part == 0) part = 3;
    REQUIRE(flat_params && frame && act_in && grad_flat && grad_cond && workspace && part >= 1 && part <= 3, who);
    REQUIRE((level == 0 || level == 1) && P >= 0 && P <= 4000000L, who);      // (0 <= P <= 4e6 samples per call)
    // d_raw for the radiance part, xw_grad_in for the deformation part alone, xw_grad_out for the radiance part alone
    REQUIRE(((part & 2) ? d_raw != nullptr : xw_grad_in != nullptr) && (part != 2 || xw_grad_out != nullptr), who);
    const ModelFns &m = kModels[model];
    if (!m.deformation_nets && part != 3) return fail(4, "%s: this model has no deformation nets", who);
    int e = m.bwd_split(flat_params, frame, level, part, P, act_in - act_col0(model, part) * P, d_raw, xw_grad_in, xw_grad_out, grad_flat,
                        grad_cond, workspace, (hipStream_t)stream);
    return e ? hip_fail(who, e) : 0;
}

int sahs_model_field_backward_fused(int model, const float *flat_params, const float *frame, int level, int part, long P, const float *act_in,
                                    const uint32_t *bits_in, const float *d_raw, const float *xw_grad_in, float *xw_grad_out, float *grad_flat,
                                    float *grad_cond, float *workspace, void *stream)
{
    const char *who = "sahs_model_field_backward_fused";
    REQUIRE_MODEL(model, who);
    const ModelFns &m = kModels[model];
    if (!m.deformation_nets && part != 3) return fail(4, "%s: this model has no deformation nets", who);
    REQUIRE(flat_params && frame && act_in && bits_in && grad_flat && grad_cond && workspace && part >= 1 && part <= 3, who);
    REQUIRE((level == 0 || level == 1) && P >= 0 && P <= 4000000L, who);      // (0 <= P <= 4e6 samples per call)
    // d_raw for the radiance part, xw_grad_in for the deformation part alone, xw_grad_out for the radiance part alone
    REQUIRE(((part & 2) ? d_raw != nullptr : xw_grad_in != nullptr) && (part != 2 || xw_grad_out != nullptr), who);
    REQUIRE(ALIGNED16(act_in) && ALIGNED16(bits_in) && ALIGNED16(workspace) && (!d_raw || ALIGNED16(d_raw)) && (!xw_grad_in || ALIGNED16(xw_grad_in)) &&
            (!xw_grad_out || ALIGNED16(xw_grad_out)), who);
    if (P == 0) return 0;
    int e = m.bwd_fused(flat_params, frame, level, part, P, act_in - act_col0(model, part) * P, bits_in, d_raw, xw_grad_in, xw_grad_out,
                        grad_flat, grad_cond, workspace, num_cus(), (hipStream_t)stream);
    return e ? hip_fail(who, e) : 0;
}

// ---- sparse branches (fp32 inference render): see csrc/field_f32.hip, FIELD_ALL_FUSED / FIELD_RADIANCE_FUSED ----
// One radiance evaluation of the render chain: ONE launch over the pass, the workspace holding the workgroups' record rings (never more
// than the pass's samples rounded up to a tile, at most 512 slots per CU; the caller has checked that they fit), and ONE probe record of
// the kind and sample count the dense launch has.  The workspace's head afterwards holds [live records of the pass | 1].
// stage: 0 whole network (coarse pass, plain chain's fine pass), 1 radiance nets on x', w from xw through src.
static long sparse_capacity(int model, size_t ws_bytes)      // record slots (a multiple of 128) a workspace of ws_bytes holds
{
    const ModelFns &m = kModels[model];
    const long head = m.f32_sparse_ws_bytes(0), rec = m.f32_sparse_ws_bytes(1) - head;
    if ((long)ws_bytes < head) return 0;
    long cap = ((long)ws_bytes - head) / rec / 128 * 128;
    return cap > (1L << 30) ? (1L << 30) : cap;
}
static int field_forward_sparse(const char *who, int model, const FieldLaunch &L, int stage, int part, const float *noise, int has_bg, void *ws, long cap)
{
    int e = probed(probe_kind(model, SAHS_F32, L.level, part), L.P, L.stream, [&] {
        hipError_t he = hipMemsetAsync(ws, 0, 8, L.stream);
        if (he != hipSuccess) return (int)he;
        return kModels[model].f32_sparse(&L, stage, noise, has_bg, ws, cap);
    });
    // (negative: the launcher's own refusals, not HIP errors -- unreachable through the caller's checks, named in case a change breaks them)
    if (e == -4) return fail(5, "%s: the sparse-branch launcher refused its record workspace (%ld slots for the rings of %ld samples)", who, cap, L.P);
    if (e < 0) return fail(4, "%s: the sparse-branch launcher has no stage %d for this model", who, stage);
    return e ? hip_fail(who, e) : 0;
}

// ---- the render chain: depths -> field level 0 -> composite -> resample -> field level 1 -> composite, one body for every entry point ----
// How a level's field pass is evaluated: `shared` (xw, src, z_new given): the deformation nets are shared by the two levels and the fine
// depths contain the coarse ones, so they run once per depth -- the coarse pass writes x', w to xw, a deformation launch adds the new
// depths', and the fine pass is the radiance nets on xw through the merge permutation src; otherwise each level is the whole network.
// `ws` given: the fp32 passes that reach the radiance nets are the sparse-branch launches on that record workspace of `cap` slots.
// The callers have checked their own arguments; a chain that came here unchecked for its sample counts is refused where it always was,
// behind the coarse field launch.
struct RenderWork {
    float *xw;      // shared evaluation: (N, Sc + nf, 8) x', w; src (N, Sc + nf) and z_new (N, nf) of the merge
    int32_t *src;
    float *z_new;
    void *ws;       // sparse branches: the record workspace and its slots
    long cap;
};
static int render_chain(const char *who, int model, const void *packed, const float *frame, int precision, long N, const float *rays,
                        int ray_stride, int Sc, int nf, int lindisp, int white_background, const float *bg, const float *t_rand,
                        const float *noise_c, const float *u, const float *noise_f, float *z_c, float *z_f, float *raw, float *weights,
                        CompositeOut coarse, const CompositeOut &fine, const RenderWork &w, void *stream)
{
    const bool shared = w.xw != nullptr, sparse = w.ws != nullptr;
    const int Sf = Sc + nf, has_bg = bg != nullptr;
    const float *pk = (const float *)packed;
    hipStream_t st = (hipStream_t)stream;
    // a sparse pass of S samples per ray: stage 0 the whole network on the depths z (x', w to xw_io when given), 1 the radiance nets on w.xw
    auto sparse_pass = [&](int level, int stage, int S, const float *z, float *xw_io, int xw_row, const int32_t *src_in, const float *noise) {
        const FieldLaunch L{.packed = pk, .frame = frame, .level = level, .P = N * S, .S = S, .rays = rays, .ray_stride = ray_stride, .zvals = z,
                            .raw = raw, .xw = xw_io, .xw_row = xw_row, .src = src_in, .num_cu = num_cus(), .stream = st};
        return field_forward_sparse(who, model, L, stage, stage == 0 ? 0 : 2, noise, has_bg, w.ws, w.cap);
    };
    int e;
    if ((e = sahs_stratified_depths(N, Sc, rays, ray_stride, lindisp, t_rand, z_c, stream))) return e;
    if (sparse)
        e = sparse_pass(0, 0, Sc, z_c, w.xw, Sf, nullptr, noise_c);
    else if (shared)
        e = sahs_model_field_forward_split(model, packed, frame, precision, 0, 0, N, Sc, rays, ray_stride, z_c, raw, w.xw, Sf, 0, nullptr, stream);
    else
        e = field_forward(who, model, packed, frame, 0, N, Sc, rays, ray_stride, z_c, raw, nullptr, precision, stream);
    if (e) return e;
    REQUIRE(Sc <= 256, who);
    if (nf == 0) coarse.depth = fine.depth, coarse.w_last = fine.w_last;      // (the reference returns the last pass's depth only)
    e = composite_launch(N, Sc, raw, z_c, rays, ray_stride, noise_c, bg, white_background, weights, coarse, st);
    if (e) return hip_fail(who, e);
    if (nf == 0) return 0;
    REQUIRE(Sf <= 256, who);
    if (shared) {
        if ((e = sahs_resample_merge(N, Sc, nf, z_c, weights, u, w.z_new, z_f, w.src, stream))) return e;
        if ((e = sahs_model_field_forward_split(model, packed, frame, precision, 1, 1, N, nf, rays, ray_stride, w.z_new, nullptr, w.xw, Sf, Sc, nullptr, stream))) return e;
        e = sparse ? sparse_pass(1, 1, Sf, nullptr, w.xw, Sf, w.src, noise_f)
                   : sahs_model_field_forward_split(model, packed, frame, precision, 1, 2, N, Sf, rays, ray_stride, nullptr, raw, w.xw, Sf, 0, w.src, stream);
    } else {
        if ((e = sahs_resample(N, Sc, nf, z_c, weights, u, nullptr, z_f, nullptr, stream))) return e;
        e = sparse ? sparse_pass(1, 0, Sf, z_f, nullptr, 0, nullptr, noise_f)
                   : field_forward(who, model, packed, frame, 1, N, Sf, rays, ray_stride, z_f, raw, nullptr, precision, stream);
    }
    if (e) return e;
    e = composite_launch(N, Sf, raw, z_f, rays, ray_stride, noise_f, bg, white_background, weights, fine, st);
    return e ? hip_fail(who, e) : 0;
}

// the dense chain, each level the whole network: its own checks, then the body
static int render_rays_chain(const char *who, int model, const void *packed, const float *frame, int precision, long N,
                             const float *rays, int ray_stride, int Sc, int nf, int lindisp, int white_background, const float *bg,
                             const float *t_rand, const float *noise_c, const float *u, const float *noise_f, float *z_c, float *z_f,
                             float *raw, float *weights, const CompositeOut &coarse, const CompositeOut &fine, void *stream)
{
    if (N == 0) return 0;   // an empty ray chunk: nothing to launch (its tensors have null data pointers)
    REQUIRE(packed && frame && rays && z_c && raw && weights && coarse.rgb && coarse.disp && coarse.acc && fine.w_last && fine.depth, who);
    REQUIRE(nf == 0 || (z_f && fine.rgb && fine.disp && fine.acc), who);
    return render_chain(who, model, packed, frame, precision, N, rays, ray_stride, Sc, nf, lindisp, white_background, bg, t_rand, noise_c, u, noise_f,
                        z_c, z_f, raw, weights, coarse, fine, RenderWork{}, stream);
}

int sahs_render_rays(const void *packed, const float *frame, int precision, long N, const float *rays, int ray_stride, int Sc, int nf,
                     int lindisp, int white_background, const float *bg, const float *t_rand, const float *noise_c, const float *u,
                     const float *noise_f, float *z_c, float *z_f, float *raw, float *weights, float *rgb_c, float *disp_c,
                     float *acc_c, float *rgb_f, float *disp_f, float *acc_f, float *w_bg, float *depth_f, void *stream)
{
    return render_rays_chain("sahs_render_rays", SAHS_MODEL_AUDIO, packed, frame, precision, N, rays, ray_stride, Sc, nf, lindisp,
                             white_background, bg, t_rand, noise_c, u, noise_f, z_c, z_f, raw, weights,
                             composite_tensors(rgb_c, disp_c, acc_c, nullptr, nullptr), composite_tensors(rgb_f, disp_f, acc_f, depth_f, w_bg), stream);
}
int sahs_model_render_rays(int model, const void *packed, const float *frame, int precision, long N, const float *rays, int ray_stride,
                           int Sc, int nf, int lindisp, int white_background, const float *bg, const float *t_rand, const float *noise_c,
                           const float *u, const float *noise_f, float *z_c, float *z_f, float *raw, float *weights, float *rgb_c,
                           float *disp_c, float *acc_c, float *rgb_f, float *disp_f, float *acc_f, float *w_bg, float *depth_f, void *stream)
{
    REQUIRE_MODEL(model, "sahs_model_render_rays");
    return render_rays_chain("sahs_model_render_rays", model, packed, frame, precision, N, rays, ray_stride, Sc, nf, lindisp, white_background,
                             bg, t_rand, noise_c, u, noise_f, z_c, z_f, raw, weights, composite_tensors(rgb_c, disp_c, acc_c, nullptr, nullptr),
                             composite_tensors(rgb_f, disp_f, acc_f, depth_f, w_bg), stream);
}

int sahs_model_render_rays_rows(int model, const void *packed, const float *frame, int precision, long N, const float *rays,
                                int ray_stride, int Sc, int nf, int lindisp, int white_background, const float *bg, const float *t_rand,
                                const float *noise_c, const float *u, const float *noise_f, float *z_c, float *z_f, float *raw,
                                float *weights, float *rows, int row_ld, float *xw, int32_t *src, float *z_new, void *stream)
{
    const char *who = "sahs_model_render_rays_rows";
    REQUIRE_MODEL(model, who);
    if (N == 0) return 0;
    REQUIRE(rows && row_ld >= SAHS_ROW_COLUMNS, who);
    const Pipe *p = pipe_of(model, precision);
    const bool deform = kModels[model].deformation_nets;
    const CompositeOut coarse = composite_rows(rows, row_ld, false), fine = composite_rows(rows, row_ld, true);
    if (deform && p && p->chain != K_NONE)      // a pair that exists only as the split chain needs its workspace
        REQUIRE(xw && src && z_new && nf > 0, who);
    if (xw && src && z_new && nf > 0 && deform && p && (p->split != K_NONE || p->chain != K_NONE)) {
        REQUIRE(packed && frame && rays && z_c && z_f && raw && weights && Sc + nf <= 256, who);
        return render_chain(who, model, packed, frame, precision, N, rays, ray_stride, Sc, nf, lindisp, white_background, bg, t_rand, noise_c, u,
                            noise_f, z_c, z_f, raw, weights, coarse, fine, RenderWork{xw, src, z_new, nullptr, 0}, stream);
    }
    return render_rays_chain(who, model, packed, frame, precision, N, rays, ray_stride, Sc, nf, lindisp, white_background, bg, t_rand, noise_c,
                             u, noise_f, z_c, z_f, raw, weights, coarse, fine, stream);
}

size_t sahs_model_render_sparse_fused_workspace_bytes(int model, long samples)
{
    if (model < 0 || model > 2 || samples < 0 || samples > (1L << 30)) return 0;
    return (size_t)kModels[model].f32_sparse_ws_bytes(samples > 0 ? kModels[model].f32_sparse_ring_slots(samples, num_cus()) : 0);
}

size_t sahs_model_render_sparse_workspace_bytes(int model, long samples)
{
    if (model < 0 || model > 2 || samples < 0 || samples > (1L << 30)) return 0;
    return (size_t)kModels[model].f32_sparse_ws_bytes((samples + 127) / 128 * 128);
}

int sahs_model_render_rays_rows_sparse(int model, const void *packed, const float *frame, int precision, long N, const float *rays,
                                       int ray_stride, int Sc, int nf, int lindisp, int white_background, const float *bg, const float *t_rand,
                                       const float *noise_c, const float *u, const float *noise_f, float *z_c, float *z_f, float *raw,
                                       float *weights, float *rows, int row_ld, float *xw, int32_t *src, float *z_new, void *ws, size_t ws_bytes,
                                       void *stream)
{
    const char *who = "sahs_model_render_rays_rows_sparse";
    REQUIRE_MODEL(model, who);
    if (precision != SAHS_F32)      // the other precisions have no sparse branches: the dense chain
        return sahs_model_render_rays_rows(model, packed, frame, precision, N, rays, ray_stride, Sc, nf, lindisp, white_background, bg, t_rand, noise_c,
                                           u, noise_f, z_c, z_f, raw, weights, rows, row_ld, xw, src, z_new, stream);
    if (N == 0) return 0;
    REQUIRE(rows && row_ld >= SAHS_ROW_COLUMNS, who);
    REQUIRE(packed && frame && rays && z_c && raw && weights && N >= 0 && Sc >= 1 && nf >= 0 && Sc + nf <= 256 && ray_stride >= 8, who);
    REQUIRE(nf == 0 || z_f, who);
    REQUIRE(ws && ALIGNED16(ws) && ALIGNED16(packed) && ALIGNED16(frame) && ALIGNED16(raw) && (!xw || ALIGNED16(xw)), who);
    // refused before the first launch: a pass the rings cannot take (one size serves both passes; the fine pass has the larger rings, or equal)
    const long cap = sparse_capacity(model, ws_bytes), all = N * (long)(Sc + nf);
    if (all > (1L << 30))
        return fail(5, "%s: a pass of %ld samples is more than 2^30, and a record's header holds the sample index as an int: render fewer rays "
                       "per call (sahs_model_render_sparse_fused_workspace_bytes sizes passes up to 2^30 samples, %ld record slots; %ld given)",
                    who, all, kModels[model].f32_sparse_ring_slots(1L << 30, num_cus()), cap);
    const long need_c = kModels[model].f32_sparse_ring_slots(N * Sc, num_cus()), need_f = kModels[model].f32_sparse_ring_slots(all, num_cus());
    const long need = need_c > need_f ? need_c : need_f;
    if (cap < need)
        return fail(5, "%s: a sparse-branch workspace of %zu bytes holds %ld record slots, the rings of this render need %ld "
                       "(sahs_model_render_sparse_fused_workspace_bytes)", who, ws_bytes, cap, need);
    const bool shared = xw && src && z_new && nf > 0 && kModels[model].deformation_nets;
    return render_chain(who, model, packed, frame, precision, N, rays, ray_stride, Sc, nf, lindisp, white_background, bg, t_rand, noise_c, u, noise_f,
                        z_c, z_f, raw, weights, composite_rows(rows, row_ld, false), composite_rows(rows, row_ld, true),
                        shared ? RenderWork{xw, src, z_new, ws, cap} : RenderWork{nullptr, nullptr, nullptr, ws, cap}, stream);
}

}  // extern "C"
