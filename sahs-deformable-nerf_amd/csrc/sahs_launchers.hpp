// sahs_launchers.hpp -- the one declaration of every extern "C" function that one .hip file defines and another calls.
// Every defining file includes it: a definition whose types drift from its declaration then fails to compile (with C linkage it
// would still link, and receive garbage arguments at run time).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

// The facts of one field-forward launch, the same block for every kernel family (fp32, bf16, split-operand).  A launcher takes it with a
// mode: 0 the whole network, 1 the deformation nets only, 2 the radiance nets only.  What a mode reads:
//   every mode   packed, frame, level, P (samples), S (samples per ray), rays, ray_stride, num_cu, stream
//   zvals        modes 0, 1: the depths, P floats
//   raw          modes 0, 2: the network's output rows
//   xw           mode 0 (optional): x', w of sample s of a ray written to column xw_col0 + s of the ray's row of xw_row columns;
//                mode 1: the same, required; mode 2: read, column src[ray][s] (src null: column s); xw_col0 is not used
//   dbg          mode 0 without xw only (optional): the debug planes of the kernels that have them
//   actbuf       optional: also save the activations of the layers the launch runs (training); bits: with actbuf, their sign-bit planes
struct FieldLaunch {
    const float *packed, *frame;
    int level;
    long P;
    int S;
    const float *rays;
    int ray_stride;
    const float *zvals;
    float *raw, *dbg;
    float *xw;
    int xw_row, xw_col0;
    const int *src;
    float *actbuf;
    uint32_t *bits;
    int num_cu;
    hipStream_t stream;
};
// ... and the one place where a block is cut down to what its mode reads: the kernels get null (or 0) for everything else
inline FieldLaunch sahs_field_mode_block(FieldLaunch L, int mode)
{
    if (mode == 1) L.raw = nullptr;
    if (mode == 2) L.zvals = nullptr, L.xw_col0 = 0;
    else L.src = nullptr;
    if (mode != 0 || L.xw != nullptr) L.dbg = nullptr;
    return L;
}

extern "C" {
// render_ops.hip
int sahs_ray_bundle_launch(int H, int W, float fx, float fy, float cx, float cy, const float *c2w, int ld, float *ro, float *rd,
                           hipStream_t stream);
int sahs_stratified_depths_launch(long N, int S, const float *rays, int ray_stride, int lindisp, const float *t_rand, float *z,
                                  hipStream_t stream);
int sahs_composite_forward_launch(long N, int S, const float *raw, const float *z, const float *rays, int ray_stride, const float *noise,
                                  const float *bg, int white_bkgd, float *rgb_map, float *disp, float *acc_map, float *weights,
                                  float *depth, float *w_last, int rgb_ld, int sc_ld, hipStream_t stream);
int sahs_route_xw_grad_launch(long N, int Sc, int nf, const int *src, const float *g_fine, float *g_coarse, float *g_new, hipStream_t stream);
int sahs_resample_launch(long N, int S, int nf, int from_z, const float *z, const float *weights, const float *u, float *z_samples,
                         float *z_out, long long *inds, int *src, hipStream_t stream);
int sahs_ray_uniforms_launch(unsigned long long seed, int stream_id, long ray0, long N, int S, float *out, hipStream_t stream);
// spade_ops.hip (the tensors: float, or with bf16 set bf16 bit patterns; stats and work: float for both)
long sahs_spade_stats_words(long planes);
int sahs_spade_modulate_launch(long planes, long hw, const void *x, const void *gamma, const void *beta, float eps, float slope, void *out,
                               float *stats, int bf16, hipStream_t stream);
int sahs_spade_modulate_backward_launch(long planes, long hw, const void *x, const void *gamma, const void *out, const float *stats,
                                        const void *grad, float eps, float slope, void *dx, void *dgamma, void *dbeta, float *work, int bf16,
                                        hipStream_t stream);
// (x: (batch, channels, h, w); gamma, beta: a batch of 1 with shared set, of `batch` otherwise; with up they and out are (2h, 2w) planes)
int sahs_spade_modulate_frozen_launch(long batch, long channels, int shared, long h, long w, int up, const void *x, const void *gamma,
                                      const void *beta, float eps, float slope, void *out, float *stats, int bf16, hipStream_t stream);
// spectral_norm.hip (the tables as host arrays of device pointers, already validated: capi.hip)
int sahs_spectral_norm_forward_launch(int jobs, const float *const *W, float *const *u, float *const *v, void *const *out,
                                      float *const *saved, const int *h, const int *w, int out_bf16, int power_iteration, float eps,
                                      hipStream_t stream);
int sahs_spectral_norm_backward_launch(int jobs, const float *const *W, const float *const *saved, const void *const *grad_out,
                                       float *const *dW, const int *h, const int *w, int grad_bf16, hipStream_t stream);
// image_metrics.hip (arguments already validated: capi.hip; records: sahs_image_metrics_tiles(H, W) * B * (C + 2) doubles)
long sahs_image_metrics_tiles(int H, int W);
int sahs_image_metrics_launch(const void *a, const void *b, int is_float, long B, int H, int W, int C, const long *stride_a,
                              const long *stride_b, double ssim_data_range, double *out, double *records, hipStream_t stream);
// image_loss.hip (arguments already validated: capi.hip; records: sahs_image_loss_tiles(H, W) * B * (C + 2) doubles; grad may be null)
long sahs_image_loss_tiles(int H, int W);
int sahs_image_loss_launch(const float *pred, const float *target, long B, int H, int W, int C, const long *stride_pred,
                           const long *stride_target, double w_l2, double w_l1, double w_ssim, int clamp, double ssim_data_range,
                           float *grad, const long *stride_grad, double *out, double *records, hipStream_t stream);
// lpips.hip (arguments already validated: capi.hip; records: B * sahs_lpips_distance_tiles(jobs, hw) doubles)
// stats: null, or 3 * B * sahs_lpips_head_pixels(jobs, hw) doubles; grad_a[l]: fa[l]'s shape; clamp applies to a alone
int sahs_lpips_prepare_launch(const void *a, const void *b, int a_is_float, int b_is_float, long B, int H, int W, const long *stride_a,
                              const long *stride_b, int normalize, int clamp, float *out, hipStream_t stream);
int sahs_lpips_prepare_grad_launch(const float *pred, const float *gx, long B, int H, int W, const long *stride_pred, int normalize, int clamp,
                                   float *grad, const long *stride_grad, hipStream_t stream);
long sahs_lpips_distance_tiles(int jobs, const long *hw);
long sahs_lpips_head_pixels(int jobs, const long *hw);
int sahs_lpips_head_forward_launch(int jobs, const float *const *fa, const float *const *fb, const float *const *weights, const int *C,
                                   const long *hw, long B, double *out, double *stats, double *records, hipStream_t stream);
int sahs_lpips_head_backward_launch(int jobs, const float *const *fa, const float *const *fb, const float *const *weights, const int *C,
                                    const long *hw, long B, const void *g, int g_is_double, const double *stats, float *const *grad_a,
                                    hipStream_t stream);
// frame_products.hip (arguments already validated: capi.hip; records: B * sahs_frame_products_tiles(H, W) * 16 bytes, with disparity)
long sahs_frame_products_tiles(int H, int W);
int sahs_frame_products_launch(const float *rgb, int C, const long *stride_rgb, const float *disp, const float *w_bg, const float *intrinsics,
                               long B, int H, int W, int clean, int central_difference, uint8_t *image, uint8_t *seg, uint8_t *normals_u8,
                               float *normals_f32, uint8_t *disparity, void *records, hipStream_t stream);
// optim.hip (w1 =1 - beta1, w2 = 1 - beta2, step_size = lr / (1 - beta1^t), bc2_sqrt = sqrt(1 - beta2^t): formed in double by the caller)
int sahs_adam_step_launch(float *params, const float *grad, float *exp_avg, float *exp_avg_sq, long n, float w1, float beta2, float w2,
                          float step_size, float bc2_sqrt, float eps, float grad_scale, hipStream_t stream);
// train_bwd.hip
int sahs_composite_backward_launch(long N, int S, const float *raw, const float *z, const float *rays, int ray_stride, const float *noise,
                                   const float *bg, int white_bkgd, const float *d_rgb, const float *d_disp, const float *d_acc,
                                   const float *d_depth, const float *d_wlast, const float *d_weights, float *d_raw, const float *loss_map,
                                   const float *loss_target, int target_ld, const float *loss_mask, const float *loss_stats,
                                   const float *loss_gscale, hipStream_t stream);
int sahs_stage1_loss_forward_launch(long N, const float *map_c, const float *map_f, const float *target, int target_ld, const float *mask,
                                    const float *class_w, float *stats, hipStream_t stream);
int sahs_conditioning_backward_launch(const float *flat, const float *audio, const float *grad_cond, float *grad_flat, float *grad_audio,
                                      hipStream_t stream);

// The sources built once per model (sahs_model.hpp: SAHS_MODEL=0 no suffix, 1 suffix _nf, 2 suffix _ns).  Every model build defines every
// one of these; a forward launcher answers -2 or -3 for a mode its build does not have (and the link, -z defs, fails on a name left undefined).
#define SAHS_DECLARE_MODEL(sfx)                                                                                                          \
    /* pack.hip */                                                                                                                       \
    long sahs_layout_param_count##sfx(void);                                                                                            \
    long sahs_layout_packed_words_f32##sfx(void);                                                                                       \
    long sahs_layout_packed_words_bf16##sfx(void);                                                                                      \
    long sahs_layout_packed_words_bf16x3##sfx(void);                                                                                    \
    long sahs_layout_frame_words##sfx(void);                                                                                            \
    long sahs_layout_act_words##sfx(void);                                                                                              \
    long sahs_layout_executed_macs##sfx(int precision, int part);                                                                       \
    int sahs_pack_weights_f32_launch##sfx(const float *flat, float *packed, hipStream_t stream);                                        \
    int sahs_pack_weights_bf16_launch##sfx(const float *flat, float *packed, hipStream_t stream);                                       \
    int sahs_pack_weights_bf16x3_launch##sfx(const float *flat, float *packed, hipStream_t stream);                                     \
    int sahs_fold_conditioning_launch##sfx(const float *flat, const float *audio, const float *pose, int pose_ld, float *frame,         \
                                           hipStream_t stream);                                                                         \
    /* field_f32.hip */                                                                                                                  \
    int sahs_layout_act_part_words##sfx(int part);                                                                                      \
    int sahs_layout_act_part_col0##sfx(int part);                                                                                       \
    int sahs_layout_bits_part_words##sfx(int part);                                                                                     \
    long sahs_field_f32_sparse_ws_bytes##sfx(long cap);                                                                                 \
    long sahs_field_f32_sparse_ring_slots##sfx(long P, int num_cu);                                                                     \
    int sahs_field_f32_launch##sfx(const FieldLaunch *launch, int mode);                                                                \
    int sahs_field_f32_sparse_launch##sfx(const FieldLaunch *launch, int stage, const float *noise, int has_bg, void *ws, long cap);    \
    /* field_bf16w.hip */                                                                                                                \
    int sahs_bf16w_exact_leaky_state##sfx(int set);                                                                                     \
    int sahs_field_bf16w_launch##sfx(const FieldLaunch *launch, int mode);                                                              \
    /* field_bf16x3.hip */                                                                                                              \
    int sahs_field_bf16x3_launch##sfx(const FieldLaunch *launch, int mode);                                                             \
    /* field_bwd.hip */                                                                                                                  \
    int sahs_bwd_gemm_precision_state##sfx(int set);                                                                                    \
    long sahs_field_backward_ws_words##sfx(long P);                                                                                     \
    int sahs_field_backward_launch##sfx(const float *flat, const float *frame, int level, long P, const float *actbuf,                  \
                                        const float *d_raw, float *grad_flat, float *grad_cond, float *ws, hipStream_t stream);         \
    int sahs_field_backward_split_launch##sfx(const float *flat, const float *frame, int level, int part, long P, const float *actbuf,  \
                                              const float *d_raw, const float *xwg_in, float *xwg_out, float *grad_flat,                \
                                              float *grad_cond, float *ws, hipStream_t stream);                                         \
    long sahs_field_backward_fused_ws_words##sfx(int part, long P);                                                                     \
    int sahs_field_backward_fused_launch##sfx(const float *flat, const float *frame, int level, int part, long P, const float *actbuf,  \
                                              const uint32_t *bits, const float *d_raw, const float *xwg_in, float *xwg_out,            \
                                              float *grad_flat, float *grad_cond, float *ws, int num_cu, hipStream_t stream);           \
    /* field_bwd_chain.hip: the fused walk's data-gradient chains (split bf16 operands) */                                              \
    long sahs_bwd_chain_stream_hw##sfx(int part);                                                                                       \
    int sahs_bwd_chain_pack_launch##sfx(const float *flat, void *stream_out, int level, int part, hipStream_t stream);                  \
    int sahs_bwd_chain_rad_launch##sfx(const void *bstream, long P, const float *d_raw, const uint32_t *bits, float *dact,              \
                                       float *dgridf, float *din_a, float *din_b, int num_cu, hipStream_t stream);                      \
    int sahs_bwd_chain_def_launch##sfx(const void *bstream, long P, const float *xwg, const float *actbuf, const uint32_t *bits,        \
                                       float *dact, float *g3, float *dw4, int num_cu, hipStream_t stream);                             \
    /* field_bwd_chain_f32.hip: the same chains in exact fp32 products */                                                               \
    long sahs_bwd_chain_f32_stream_floats##sfx(int part);                                                                               \
    int sahs_bwd_chain_f32_pack_launch##sfx(const float *flat, float *stream_out, int level, int part, hipStream_t stream);             \
    int sahs_bwd_chain_f32_rad_launch##sfx(const float *bstream, long P, const float *d_raw, const uint32_t *bits, float *dact,         \
                                           float *dgridf, float *din_a, float *din_b, int num_cu, hipStream_t stream);                  \
    int sahs_bwd_chain_f32_def_launch##sfx(const float *bstream, long P, const float *xwg, const float *actbuf, const uint32_t *bits,   \
                                           float *dact, float *g3, float *dw4, int num_cu, hipStream_t stream);
SAHS_DECLARE_MODEL()
SAHS_DECLARE_MODEL(_nf)
SAHS_DECLARE_MODEL(_ns)
#undef SAHS_DECLARE_MODEL
}
