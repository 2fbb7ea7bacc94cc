/*
 * sahs_nerf.h -- C ABI of the MI355X-native deformable-NeRF volume-rendering hot path.
 *
 * The reference (jematy/SAHS-Deformable-Nerf) has no native boundary: its operator API for this
 * path is three Python seams.  Each entry point below cites the reference
 * interface it replaces; the Python side (sahs-deformable-nerf_amd/{train_utils,models,
 * volume_rendering_utils,nerf_helpers}.py) mirrors those seams one to one and calls down here.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer to fp32 unless stated; the library never allocates,
 *    never synchronises and launches only on the given stream (hipStream_t passed as void*),
 *    so a caller may capture any sequence of calls in a hipGraph;
 *  - return 0 on success; non-zero = error, text via sahs_last_error() (thread-local); a call over zero rays (N == 0)
 *    succeeds without launching anything (its buffers may be null);
 *  - "rays" is the reference's packed ray table, row = [ro3, rd3, near, far, ...] with
 *    `ray_stride` floats per row (train_utils.py:255-261 builds it with stride 20);
 *  - precision: SAHS_F32 = exact fp32 (f32 MFMA), SAHS_BF16 = bf16 MFMA operands, fp32 accumulate.
 */
#ifndef SAHS_NERF_H
#define SAHS_NERF_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SAHS_ABI_VERSION 1
#define SAHS_F32 0
#define SAHS_BF16 1
#define SAHS_BF16X3 3    /* near-fp32 on the bf16 pipe (every model): operands split into bf16 hi + lo, three MFMAs per product, fp32 accumulate,
                          * in the radiance AND (since round 3) the deformation launches; x' = x + tanh(.) and the encodings stay fp32 arithmetic.
                          * The models with deformation nets run it as the split chain only; the NeRFaceModel without them as one whole-network launch.
                          * SAHS_X3_DEFORM=f32 in the environment keeps the deformation launches on the fp32 kernel (the round-2 form) */
/* precision values 2 and 4 are reserved (A/B kernels of development builds, csrc/sahs_common.hpp; not in the shipped library) */

int sahs_abi_version(void);
const char *sahs_last_error(void);

/* Number of fp32 values in the canonical flat parameter buffer = the model's state_dict
 * (eval_stage_rays.py:299-303), tensors concatenated in state_dict order: 2,775,633. */
long sahs_param_count(void);
/* Size (in floats / 4-byte words) of the packed weight buffer and of the per-frame buffer. */
long sahs_packed_words(int precision);
long sahs_frame_words(void);

/* state_dict -> kernel layout.  Call after every parameter update (eval: once).
 * Replaces nothing in the reference (it keeps nn.Linear weights); feeds sahs_field_forward. */
int sahs_pack_weights(const float *flat_params, void *packed, int precision, void *stream);

/* Per-frame conditioning.  Replaces AudioNet (modules.py:43-73), rot_to_euler /
 * pose_to_euler_trans (models.py:482-504), encode_pose_fn (models.py:203-207) and the
 * per-point .repeat() of both (models.py:518,521), which every point-chunk of the reference
 * recomputes.  audio: (16,29); pose: 3x4 (or 4x4) row-major with row stride pose_ld.
 * frame[0:76] = driving, frame[80:116] = pose encoding, then the folded biases. */
int sahs_fold_conditioning(const float *flat_params, const float *audio, const float *pose, int pose_ld, float *frame,
                           void *stream);

/* get_ray_bundle (nerf_helpers.py:178-233). intrinsics = [fx, fy, cx, cy] (cx, cy relative);
 * c2w device pointer, row stride ld; ro, rd: (H, W, 3). */
int sahs_get_ray_bundle(int H, int W, float fx, float fy, float cx, float cy, const float *c2w, int ld, float *ro, float *rd,
                        void *stream);

/* Uniform draws in [0,1) for rays [ray0, ray0+N) x S samples -> out (N,S), as a pure function of (seed, stream_id, GLOBAL ray
 * index, sample index) (Philox4x32-10): the partition-invariant alternative to the reference's `torch.rand(z_vals.shape)`
 * (train_utils.py:110) and `torch.rand(...)` in sample_pdf_2 (nerf_helpers.py:469), whose values depend on how a frame is
 * chunked or sharded over GPUs.  stream_id separates the draws of one ray (0: t_rand, 1: u). */
int sahs_ray_uniforms(uint64_t seed, int stream_id, long ray0, long N, int S, float *out, void *stream);

/* Coarse depths (train_utils.py:93-113). t_rand (N,S) uniform draws or NULL (perturb off). z: (N,S). */
int sahs_stratified_depths(long N, int S, const float *rays, int ray_stride, int lindisp, const float *t_rand, float *z,
                           void *stream);

/* run_network + model forward (train_utils.py:9-50 -> models.py:514-528) for level 0 (coarse)
 * or 1 (fine), including pts = ro + rd*z (train_utils.py:115,168).  z: (N,S); raw: (N,S,16) =
 * [rgb3, seg12, sigma].  dbg: NULL, or N*S*88 floats receiving [N*S x 56: dx3, w2, first feature of
 * selected hidden layers][N*S x 32: grid features] (test seam). */
int sahs_field_forward(const void *packed, const float *frame, int level, long N, int S, const float *rays, int ray_stride,
                       const float *z, float *raw, float *dbg, int precision, void *stream);

/* volume_render_radiance_field (volume_rendering_utils.py:7-78) with the caller's background
 * overwrite (train_utils.py:135-136,184-185) when bg != NULL.  noise: (N,S) already scaled by
 * radiance_field_noise_std, or NULL.  Outputs rgb (N,15), disp (N), acc (N), weights (N,S), depth (N). */
int sahs_composite_forward(long N, int S, const float *raw, const float *z, const float *rays, int ray_stride,
                           const float *noise, const float *bg, int white_background, float *rgb, float *disp, float *acc,
                           float *weights, float *depth, void *stream);

/* z_vals_mid + sample_pdf_2 + cat + sort (train_utils.py:157-166, nerf_helpers.py:454-497).
 * weights: the full (N,S) composite weights (the [1:-1] slice is taken inside).  u: (N,nf) uniform
 * draws or NULL (det=True).  z_samples (N,nf) and inds (N,nf) int64 may be NULL; z_out: (N,S+nf). */
int sahs_resample(long N, int S, int nf, const float *z, const float *weights, const float *u, float *z_samples,
                  float *z_out, int64_t *inds, void *stream);

/* sample_pdf_2 alone (nerf_helpers.py:454-497): bins (N,nb), weights (N,nb-1), u (N,ns) or NULL (det=True)
 * -> samples (N,ns); inds (N,ns) int64 optional. */
int sahs_sample_pdf(long N, int nb, int ns, const float *bins, const float *weights, const float *u, float *samples,
                    int64_t *inds, void *stream);

/* predict_and_render_radiance (train_utils.py:72-206) for one ray chunk: the six launches above
 * in sequence.  Workspace (caller-owned): z_c (N,Sc), z_f (N,Sc+nf), raw (N,Sc+nf,16),
 * weights (N,Sc+nf).  Random draws in the reference's order (any may be NULL): t_rand (N,Sc),
 * noise_c (N,Sc), u (N,nf), noise_f (N,Sc+nf).  Outputs as the reference's 8-tuple:
 * rgb_c (N,15), disp_c, acc_c, rgb_f (N,15), disp_f, acc_f, w_bg (N) = weights_f[:, -1], depth_f. */
int sahs_render_rays(const void *packed, const float *frame, int precision, long N, const float *rays, int ray_stride, int Sc,
                     int nf, int lindisp, int white_background, const float *bg, const float *t_rand, const float *noise_c,
                     const float *u, const float *noise_f, float *z_c, float *z_f, float *raw, float *weights, float *rgb_c,
                     float *disp_c, float *acc_c, float *rgb_f, float *disp_f, float *acc_f, float *w_bg, float *depth_f,
                     void *stream);

/* ---- training path (BASELINE.json configs[4]: train_stage_rays_auto.py:437-499 calls loss.backward() through the path) ----
 * Gradients follow autograd of the reference graph.  fp32 only.  The backward is layer-wise over saved activations:
 * sahs_field_forward_save = sahs_field_forward that additionally writes sahs_act_words_per_sample() floats per sample (an opaque
 * buffer of N*S*words floats: one dense [N*S x width] array per layer; sahs_field_backward must be given the same P = N*S). */
long sahs_act_words_per_sample(void);
long sahs_field_backward_workspace_words(long P);
int sahs_field_forward_save(const void *packed, const float *frame, int level, long N, int S, const float *rays, int ray_stride,
                            const float *z, float *raw, float *act_out, void *stream);
/* d_raw (P,16) -> grad_flat (+=, canonical flat layout: every Linear weight/bias of warp/hyper/radiance nets and the feature
 * grid) and grad_cond (+=: [0:76] d driving, [80:116] d pose encoding).  P = N*S samples, P <= 4e6 per call. */
int sahs_field_backward(const float *flat_params, const float *frame, int level, long P, const float *act_in, const float *d_raw,
                        float *grad_flat, float *grad_cond, float *workspace, void *stream);
/* Arithmetic of the backward's dense-layer GEMMs (dW = dY^T X, dX = dY W; every model).  SAHS_BF16X3 (default): operands split into bf16
 * hi + lo on their way to the matrix pipe, three bf16 MFMAs per product, fp32 accumulation -- gradients within ~1e-5 of their scale of the
 * f32 form, far inside what two correct fp32 forwards differ by at the (leaky-)ReLU kinks; SAHS_F32: f32 MFMAs, exact
 * products (the A/B reference; SAHS_BWD_GEMM=f32 in the environment selects it at start-up).  precision < 0 queries.  Returns the
 * setting in force, -1 for an unknown value.  Process-wide. */
int sahs_backward_gemm_precision(int precision);
/* backward of sahs_composite_forward: any of d_rgb (N,15), d_disp, d_acc, d_depth, d_wlast (N: gradient of weights[:, -1], the
 * driver's 7th output), d_weights (N,S: gradient of the whole weights output, for the volume_render_radiance_field seam) may
 * be NULL -> d_raw (N,S,16). */
int sahs_composite_backward(long N, int S, const float *raw, const float *z, const float *rays, int ray_stride, const float *noise,
                            const float *bg, int white_background, const float *d_rgb, const float *d_disp, const float *d_acc,
                            const float *d_depth, const float *d_wlast, const float *d_weights, float *d_raw, void *stream);
/* The Stage-I objective of train_stage_rays_auto.py:455-468 over one ray batch, with the loss modules of nerf_helpers.py:14-62
 * (MaskMSELoss, MaskCrossEntropyLoss built with class_weights, :268-271):
 *   loss = sum over the given levels of  mean l2 + 0.02 mean ce + 0.005 sum_{c in 7,8} (masked mean_c l2 + masked mean_c ce)
 * map_coarse / map_fine (N,15) = the rendered [rgb3 | seg12] of a level (either may be NULL), target (N,target_ld >= 3), mask (N,12)
 * one-hot.  stats (64 floats): [0] loss, [1] mean l2 of the last level given (the script's psnr input), [2:14] the new sample_prob
 * (:466-468), [14:26] per-class ray counts (>= 1), [26] N.  One workgroup, fixed summation order. */
#define SAHS_LOSS_STATS_WORDS 64
int sahs_stage1_loss_forward(long N, const float *map_coarse, const float *map_fine, const float *target, int target_ld, const float *mask,
                             const float *class_weights, float *stats, void *stream);
/* sahs_composite_backward for a level whose rendered map enters that objective: the kernel forms d loss / d [rgb3 | seg12] of each ray
 * itself from (loss_map = the level's forward output, target, mask, stats of sahs_stage1_loss_forward, *loss_gscale = d objective /
 * d loss or NULL for 1) and adds it to d_rgb (may be NULL), so the (N,15) gradient never exists in memory. */
int sahs_composite_backward_loss(long N, int S, const float *raw, const float *z, const float *rays, int ray_stride, const float *noise,
                                 const float *bg, int white_background, const float *d_rgb, const float *d_disp, const float *d_acc,
                                 const float *d_depth, const float *d_wlast, const float *loss_map, const float *loss_target, int target_ld,
                                 const float *loss_mask, const float *loss_stats, const float *loss_gscale, float *d_raw, void *stream);
/* grad_cond[0:76] -> AudioNet parameter gradients in grad_flat (+=) and, optionally, grad_audio (16,29) (+=). */
int sahs_conditioning_backward(const float *flat_params, const float *audio, const float *grad_cond, float *grad_flat,
                               float *grad_audio, void *stream);

/* ---- every built architecture behind one family ----
 * The reference builds its field model with getattr(models, cfg.models.mask.type)(cfg) (eval_stage_rays.py:299,
 * train_stage_rays_auto.py:116); the same path serves
 *   SAHS_MODEL_AUDIO           AudioFaceModel, config/audio/<person>.yml (models.py:381-528) -- the functions above;
 *   SAHS_MODEL_NERFACE         NeRFaceModel, config/expression/person_2.yml / person_3.yml (models.py:189-378): warp + hyper
 *                              sheet on, 15-octave encodings, 1-D ambient coordinate, 4-layer trunk fed with the expression;
 *   SAHS_MODEL_NERFACE_STATIC  NeRFaceModel, config/expression/person_1.yml: use_warp False, use_ambient False.
 * flat_params is that model's state_dict in order (2,775,633 / 2,311,140 / 2,066,976 values); `driving` is the (16,29) audio
 * window for the AudioFaceModel and the 76-d expression vector (models.py:368 `driving.repeat`) for the NeRFaceModels;
 * rays, depths and outputs are the same, and sahs_get_ray_bundle, sahs_ray_uniforms, sahs_stratified_depths,
 * sahs_composite_forward, sahs_resample, sahs_sample_pdf are model-independent.  Training is SAHS_F32 for every model (its saving forward
 * optionally on the split-operand kernels: sahs_model_field_forward_split_save_bits_x3 / sahs_model_field_forward_save_bits_x3); rendering
 * additionally has SAHS_BF16 for all three (for SAHS_MODEL_NERFACE that means MIXED precision: deformation nets with split bf16 operands --
 * hi + lo, three MFMAs per product, as SAHS_BF16X3 -- + plain-bf16 radiance nets, see sahs_model_field_forward_split) and SAHS_BF16X3 for
 * every model (SAHS_MODEL_AUDIO and SAHS_MODEL_NERFACE: the split chain, packed [hi/lo streams | fp32 pack]; SAHS_MODEL_NERFACE_STATIC:
 * the whole network, packed as its hi/lo streams alone). */
#define SAHS_MODEL_AUDIO 0
#define SAHS_MODEL_NERFACE 1
#define SAHS_MODEL_NERFACE_STATIC 2
long sahs_model_param_count(int model);
long sahs_model_packed_words(int model, int precision);
long sahs_model_frame_words(int model);
int sahs_model_pack_weights(int model, const float *flat_params, void *packed, int precision, void *stream);
int sahs_model_fold_conditioning(int model, const float *flat_params, const float *driving, const float *pose, int pose_ld, float *frame,
                                 void *stream);
int sahs_model_field_forward(int model, const void *packed, const float *frame, int level, long N, int S, const float *rays,
                             int ray_stride, const float *z, float *raw, float *dbg, int precision, void *stream);
int sahs_model_render_rays(int model, const void *packed, const float *frame, int precision, long N, const float *rays, int ray_stride,
                           int Sc, int nf, int lindisp, int white_background, const float *bg, const float *t_rand, const float *noise_c,
                           const float *u, const float *noise_f, float *z_c, float *z_f, float *raw, float *weights, float *rgb_c,
                           float *disp_c, float *acc_c, float *rgb_f, float *disp_f, float *acc_f, float *w_bg, float *depth_f,
                           void *stream);

/* training path of any built model (fp32): the sahs_field_forward_save / sahs_field_backward pair above with a model id.
 * grad_cond: [0:76] d driving (for the NeRFaceModels this IS the gradient of the expression vector; for the AudioFaceModel
 * sahs_conditioning_backward carries it on through AudioNet), [80:116] d pose encoding. */
long sahs_model_act_words_per_sample(int model);
long sahs_model_field_backward_workspace_words(int model, long P);
int sahs_model_field_forward_save(int model, const void *packed, const float *frame, int level, long N, int S, const float *rays,
                                  int ray_stride, const float *z, float *raw, float *act_out, void *stream);
int sahs_model_field_backward(int model, const float *flat_params, const float *frame, int level, long P, const float *act_in,
                              const float *d_raw, float *grad_flat, float *grad_cond, float *workspace, void *stream);

/* Multiply-accumulates per sample evaluation that the field kernel of (model, precision) issues to the matrix pipe: the layer
 * program's zero-padded tiles and k-blocks, without the per-frame constant columns (folded into biases once per frame).  The
 * ALGORITHMIC count the roofline is quoted on is the reference's own (927,872 for AudioFaceModel). */
long sahs_model_executed_macs_per_sample(int model, int precision);
/* the same for a part of the network: 0 all of it, 1 the deformation nets, 2 the radiance net (sahs_model_field_forward_split) */
long sahs_model_executed_macs_part(int model, int precision, int part);

/* The 8-tuple of a ray side by side in one row of SAHS_ROW_COLUMNS floats -- the unit the multi-GPU all-gather of rendered
 * pixels moves and the layout run_one_iter_of_nerf's chunk loop fills in place, so no per-chunk
 * concatenation of eight tensors is needed (train_utils.py:298-319 does `torch.cat` per output). */
#define SAHS_ROW_COLUMNS 36
#define SAHS_ROW_RGB_C 0     /* 15: rgb3 + seg12 of the coarse pass */
#define SAHS_ROW_DISP_C 15
#define SAHS_ROW_ACC_C 16
#define SAHS_ROW_RGB_F 17    /* 15 */
#define SAHS_ROW_DISP_F 32
#define SAHS_ROW_ACC_F 33
#define SAHS_ROW_W_BG 34     /* weights[:, -1] of the fine pass (of the coarse pass when nf == 0) */
#define SAHS_ROW_DEPTH_F 35
/* sahs_composite_forward writing into such rows: the coarse pass (fine_pass 0) fills columns 0..16, the fine pass columns 17..35
 * (incl. w_bg = weights[:, -1] and depth); weights (N,S) stays a dense array (the resampling reads it). */
int sahs_composite_forward_rows(long N, int S, const float *raw, const float *z, const float *rays, int ray_stride, const float *noise,
                                const float *bg, int white_background, float *weights, float *rows, int row_ld, int fine_pass, void *stream);
/* z_vals_mid + sample_pdf_2 + cat + sort as sahs_resample, also returning the merge permutation: src (N,S+nf) int32, position s of the
 * sorted row holds element src[s] of cat(z, z_samples) (train_utils.py:166; equal values keep that order).
 * GUARANTEE: src[ray] is ALWAYS a permutation of 0..S+nf-1 and every slot of z_out and src is written, whatever the inputs hold: the
 * order is torch.sort's total order -- a NaN (non-finite weights make a ray's new samples NaN) follows every number, NaNs in index order. */
int sahs_resample_merge(long N, int S, int nf, const float *z, const float *weights, const float *u, float *z_samples, float *z_out,
                        int32_t *src, void *stream);

/* The field evaluated in parts.  The deformation nets (WarpFieldMLP, HyperSheetMLP: one instance for both levels, models.py:231-254)
 * map a sample point x to (x', w); the fine pass's depths are sort(cat(coarse depths, new depths)), so the reference's fine pass
 * repeats the deformation of every coarse sample.  mode 0: the whole network for (N,S) depths z, also writing [x'0 x'1 x'2 w0 w1 . . .]
 * of every sample to xw[ray][xw_col0 + s] (xw: (N, xw_row, 8) floats); mode 1: the deformation nets only (raw unused); mode 2: the
 * radiance net of `level` only, for S samples per ray whose (x', w) are xw[ray][src[ray][s]] (z unused).  Same arithmetic on the same
 * operands as sahs_model_field_forward: bit-identical raw.  SAHS_F32 for the models with deformation nets (not SAHS_MODEL_NERFACE_STATIC);
 * SAHS_BF16 for SAHS_MODEL_AUDIO (packed from sahs_pack_weights(..., SAHS_BF16, ...)) and for SAHS_MODEL_NERFACE, where it means MIXED
 * precision: mode 1 runs the deformation nets with split bf16 operands (fp32 kernel under SAHS_X3_DEFORM=f32), mode 2 the bf16 radiance nets
 * (src may then be NULL: sample s of a ray is column s of xw), mode 0 both one after the other (xw_col0 must be 0); packed =
 * sahs_model_pack_weights(SAHS_MODEL_NERFACE, ..., SAHS_BF16, ...) = [bf16 radiance stream | fp32 pack | hi/lo streams].  SAHS_BF16X3 for
 * SAHS_MODEL_AUDIO and SAHS_MODEL_NERFACE: both modes on the split-operand kernels (mode 0 one after the other, src may be NULL in mode 2),
 * packed = [hi/lo streams | fp32 pack].  SAHS_MODEL_NERFACE_STATIC has no deformation nets: its SAHS_BF16 and SAHS_BF16X3 paths are
 * sahs_model_field_forward (the whole network in one launch).
 * PRECONDITION (not checked on the device): every src[ray][s] lies in [0, xw_row) -- it indexes xw's row of that ray (a permutation from
 * sahs_resample_merge satisfies it; ops.field_forward_split validates a caller-made one). */
int sahs_model_field_forward_split(int model, const void *packed, const float *frame, int precision, int level, int mode, long N, int S, const float *rays,
                                   int ray_stride, const float *z, float *raw, float *xw, int xw_row, int xw_col0, const int32_t *src,
                                   void *stream);

/* Training through the split evaluation (autograd of the same graph, train_stage_rays_auto.py:493, with the deformation nets
 * evaluated once per depth).  sahs_model_field_forward_split_save = sahs_model_field_forward_split (fp32) that also stores the
 * activations of the layers it runs into act_out: N*S*sahs_model_act_words_part(model, mode) floats (part/mode 0: whole network, 1:
 * deformation nets, 2: radiance nets).  sahs_model_field_backward_split walks `part` of the network backwards over activations saved by
 * the forward of the same part: the seam is the gradient w.r.t. (x', w), (P,8) rows [dx'0 dx'1 dx'2 . dw0 dw1 . .]: part 2 (radiance
 * alone) takes d_raw (P,16) and writes xw_grad_out; part 1 (deformation alone) starts from xw_grad_in; part 3 (everything) takes d_raw
 * and ADDS xw_grad_in (may be NULL) at the seam.  sahs_route_xw_grad scatters the fine pass's (N,Sc+nf,8) seam gradient through the merge
 * permutation src (sahs_resample_merge) into g_coarse (N,Sc,8) -- the xw_grad_in of the coarse pass -- and g_new (N,nf,8). */
long sahs_model_act_words_part(int model, int part);
int sahs_model_field_forward_split_save(int model, const void *packed, const float *frame, int level, int mode, long N, int S, const float *rays,
                                        int ray_stride, const float *z, float *raw, float *xw, int xw_row, int xw_col0, const int32_t *src,
                                        float *act_out, void *stream);
int sahs_model_field_backward_split(int model, const float *flat_params, const float *frame, int level, int part, long P, const float *act_in,
                                    const float *d_raw, const float *xw_grad_in, float *xw_grad_out, float *grad_flat, float *grad_cond,
                                    float *workspace, void *stream);
int sahs_route_xw_grad(long N, int Sc, int nf, const int32_t *src, const float *g_fine, float *g_coarse, float *g_new, void *stream);

/* SAHS_BF16 field kernels: NeRFMLP's LeakyReLU(0.01) (modules.py:252) is by default applied to the packed bf16 bit patterns (slope 0.0095 ..
 * 0.0106 depending on the mantissa: 15 % of a launch faster, PSNR cost measured in bench.py); sahs_bf16_exact_leaky(1) selects the kernel
 * instance that computes max(v, 0.01 v) in fp32 before rounding, as the reference would in bf16 -- e.g. to A/B a real checkpoint.
 * Process-wide; enable < 0 queries; SAHS_BF16_EXACT_LEAKY=1 in the environment selects it at first use.  Returns the state in force. */
int sahs_bf16_exact_leaky(int enable);

/* The fused backward walk (every model; in the arithmetic sahs_backward_gemm_precision names: split-bf16 operands,
 * SAHS_BF16X3, or exact fp32 products, SAHS_F32 -- the reference's).  Replaces the ~38 GEMM launches sahs_model_field_backward_split makes
 * per part -- autograd of modules.py:254-295 (NeRFMLP), :371-390 (WarpFieldMLP), :444-462 (HyperSheetMLP) as driven by
 * train_stage_rays_auto.py:437-499 -- by two or three: one sample-major data-gradient chain and the weight gradients over job tables.  The (leaky-)ReLU masks come from SIGN BITS the saving forward writes beside the activations:
 * sahs_model_field_forward_split_save_bits = sahs_model_field_forward_split_save that also fills bits_out, N*S*sahs_model_bits_words_part(
 * model, mode) 32-bit words (mode 0: [deformation planes | radiance planes]).  sahs_model_field_backward_fused takes the same arguments as
 * sahs_model_field_backward_split plus bits_in (the planes of `part`; part 3: both, as written by a mode-0 save); workspace:
 * sahs_model_field_backward_fused_workspace_words(model, part, P) floats (-1: a part the model does not have).  Same results as the per-layer
 * walk up to summation order (tests/test_gpu_training.py, tests/test_gpu_nerface_fused.py).
 * Models and parts: SAHS_MODEL_AUDIO and SAHS_MODEL_NERFACE parts 1 (deformation nets), 2 (radiance nets of `level`), 3 (both);
 * SAHS_MODEL_NERFACE_STATIC part 3 only (= its radiance nets: no seam gradient, xw_grad_in / xw_grad_out unused), parts 1 and 2 fail
 * with "this model has no deformation nets".  Sign words per sample (sahs_model_bits_words_part, part 1 / 2 / 0 = 3):
 * AudioFaceModel 48 / 96 / 144, NeRFaceModel 48 / 64 / 112, NeRFaceModel without deformation -- / 64 / 64.
 * Workspace: per-sample floats times P plus a constant part (the feature grid twice, the part's transposed weight stream, scratch):
 *   AudioFaceModel  part 1: 1,256   part 2: 3,736   part 3: 5,000      NeRFaceModel  part 1: 1,288   part 2: 2,808   part 3: 4,104
 *   NeRFaceModel without deformation  part 3: 2,616
 * The static model's saving forward is the whole-network one: sahs_model_field_forward_save_bits = sahs_model_field_forward_save that also
 * fills bits_out, N*S*sahs_model_bits_words_part(model, 0) words (every model; the planes a mode-0 split save writes). */
long sahs_model_bits_words_part(int model, int part);
int sahs_model_field_forward_split_save_bits(int model, const void *packed, const float *frame, int level, int mode, long N, int S, const float *rays,
                                             int ray_stride, const float *z, float *raw, float *xw, int xw_row, int xw_col0, const int32_t *src,
                                             float *act_out, uint32_t *bits_out, void *stream);
int sahs_model_field_forward_save_bits(int model, const void *packed, const float *frame, int level, long N, int S, const float *rays,
                                       int ray_stride, const float *z, float *raw, float *act_out, uint32_t *bits_out, void *stream);
/* The same buffers written by the split-operand kernels (field_bf16x3.hip; `packed` = the SAHS_BF16X3 pack of the weights): the training
 * forward at three bf16 MFMAs per product instead of fp32 MFMAs.  Modes 1 (deformation nets) and 2 (radiance nets) of SAHS_MODEL_AUDIO and
 * SAHS_MODEL_NERFACE; the saved values are those kernels' own (within a few 1e-6 relative of the fp32 kernel's), the signs are the signs of
 * the values saved.  sahs_model_field_forward_save_bits_x3: the whole-network form, SAHS_MODEL_NERFACE_STATIC only (the other models fail
 * with a message that names the split form). */
int sahs_model_field_forward_split_save_bits_x3(int model, const void *packed, const float *frame, int level, int mode, long N, int S, const float *rays,
                                                int ray_stride, const float *z, float *raw, float *xw, int xw_row, int xw_col0, const int32_t *src,
                                                float *act_out, uint32_t *bits_out, void *stream);
int sahs_model_field_forward_save_bits_x3(int model, const void *packed, const float *frame, int level, long N, int S, const float *rays,
                                          int ray_stride, const float *z, float *raw, float *act_out, uint32_t *bits_out, void *stream);
long sahs_model_field_backward_fused_workspace_words(int model, int part, long P);
int sahs_model_field_backward_fused(int model, const float *flat_params, const float *frame, int level, int part, long P, const float *act_in,
                                    const uint32_t *bits_in, const float *d_raw, const float *xw_grad_in, float *xw_grad_out, float *grad_flat,
                                    float *grad_cond, float *workspace, void *stream);

/* sahs_model_render_rays writing rows[r * row_ld + column] instead of eight dense arrays (row_ld >= 36; columns 17..33 are
 * left untouched when nf == 0).  Workspace and draws as sahs_render_rays.  Optional extra workspace xw (N,Sc+nf,8) floats, src
 * (N,Sc+nf) int32, z_new (N,nf) floats: when all three are given (nf > 0; any model with deformation nets, any precision -- required for the mixed-precision
 * SAHS_MODEL_NERFACE + SAHS_BF16 and for SAHS_BF16X3 of those models, which exist as this chain only) the chain evaluates the deformation nets once per
 * depth (sahs_model_field_forward_split) -- 6 % less matrix work per frame, identical results. */
int sahs_model_render_rays_rows(int model, const void *packed, const float *frame, int precision, long N, const float *rays,
                                int ray_stride, int Sc, int nf, int lindisp, int white_background, const float *bg, const float *t_rand,
                                const float *noise_c, const float *u, const float *noise_f, float *z_c, float *z_f, float *raw,
                                float *weights, float *rows, int row_ld, float *xw, int32_t *src, float *z_new, void *stream);

/* sahs_model_render_rays_rows with SPARSE BRANCHES (fp32; any other precision is handed to sahs_model_render_rays_rows unchanged).  The
 * composite gives a sample whose sigma + noise is <= 0 the weight exactly 0, and with a background prior it replaces the last sample's
 * channels, so the colour and seg branches of such samples are never used.  Every radiance evaluation of the chain (both the plain chain and,
 * with xw / src / z_new, the shared-deformation one) is ONE launch per pass: every persistent workgroup runs its samples up to fc_alpha,
 * appends feat, x' and the index of every LIVE sample to a private ring of records in the workspace, and runs the branch layers itself
 * over the oldest records whenever the ring holds a tile's worth (128), then drains it.  rows, z_c, z_f and weights are bit-identical to
 * sahs_model_render_rays_rows.
 * raw: the row of a live sample is bit-identical too; of a zero-weight sample only column 15 (sigma) is a network output -- columns 0..14
 * hold the fc_rgb / fc_seg biases (the FINAL tile as fc_alpha leaves it), finite and the same in both chains, NOT the sample's logits.
 * ws, ws_bytes: the record workspace, 16-byte aligned.  It has to hold the rings of the larger pass, N * (Sc + nf) samples:
 * sahs_model_render_sparse_fused_workspace_bytes(model, samples) is the exact need on the current device (at most 512 record slots per
 * compute unit, 0.13 GiB on 256 of them), sahs_model_render_sparse_workspace_bytes(model, samples) an upper bound that does not depend on
 * the device (every sample a slot, rounded up to a tile).  A workspace that holds less, or a pass of more than 2^30 samples (a record
 * holds its sample's index as an int), is refused with code 5 before anything is launched.  No host synchronisation.  The launch probe sees
 * ONE record per pass, of the dense launch's kind and sample count.  The first two 32-bit words of the workspace afterwards hold the live
 * records of the last pass and 1 (once a sparse pass ran). */
size_t sahs_model_render_sparse_workspace_bytes(int model, long samples);
size_t sahs_model_render_sparse_fused_workspace_bytes(int model, long samples);
int sahs_model_render_rays_rows_sparse(int model, const void *packed, const float *frame, int precision, long N, const float *rays,
                                       int ray_stride, int Sc, int nf, int lindisp, int white_background, const float *bg, const float *t_rand,
                                       const float *noise_c, const float *u, const float *noise_f, float *z_c, float *z_f, float *raw,
                                       float *weights, float *rows, int row_ld, float *xw, int32_t *src, float *z_new, void *ws, size_t ws_bytes,
                                       void *stream);

/* ---- optimiser step (the training step's "Adam/LR schedule") ----
 * torch.optim.Adam with weight_decay = 0, amsgrad = False, maximize = False -- what the reference builds
 * (train_stage_rays_auto.py:201-209: getattr(torch.optim, "Adam")(params, lr=cfg.optimizer.lr)) -- as ONE launch over the n contiguous
 * fp32 values of the canonical flat buffer; params, exp_avg, exp_avg_sq are updated in place:
 *     g = grad * grad_scale                                (1 on one GPU, 1 / world after a summed all-reduce)
 *     exp_avg    += (g - exp_avg) * (1 - beta1)
 *     exp_avg_sq  = exp_avg_sq * beta2 + (1 - beta2) * g * g
 *     params     -= lr / (1 - beta1^step) * exp_avg / (sqrt(exp_avg_sq) / sqrt(1 - beta2^step) + eps)
 * step: the 1-based count of this update; both bias corrections are formed from it in double on the host.  lr, beta1, beta2 and eps are
 * read as the shortest decimal that rounds to the float given (0.999f means 0.999), so the scalars are the ones torch forms from Python
 * floats.  sqrt and the divisions are correctly rounded.  Buffers need 4-byte alignment only (16-byte accesses where all four share an
 * alignment, element by element otherwise).  Invalid: a null pointer, n < 0, step < 1, lr or eps not finite and positive, a beta outside
 * [0, 1), params / exp_avg / exp_avg_sq overlapping.  n == 0 succeeds without a launch.  A training step on this ABI is
 * sahs_model_field_backward* -> sahs_adam_step -> sahs_model_pack_weights. */
int sahs_adam_step(float *params, const float *grad, float *exp_avg, float *exp_avg_sq, long n, float lr, float beta1, float beta2,
                   float eps, long step, float grad_scale, void *stream);

/* ---- Stage-II refiner building block ----
 * The elementwise core of SPADELayer.forward followed by its SPADEBlock's LeakyReLU (nerf/_init_spade.py:130-139, :262-279):
 *   out = lrelu_slope( InstanceNorm2d(x; eps, biased variance, no affine) * (1 + gamma) + beta )
 * over `planes` = N*C contiguous planes of `hw` = H*W floats each (NCHW); gamma, beta, out have x's shape; slope 1 = no activation;
 * stats: sahs_spade_modulate_workspace_words(planes) floats of workspace (per plane: chunk sums and chunk sums of squares about the mean).  The convolutions that produce gamma / beta stay library
 * calls (MIOpen through PyTorch): sahs-deformable-nerf_amd/spade.py.  A plane is one gridDim.y slot of every launch: planes <= 65535
 * (more is refused with a non-zero return code before anything is launched). */
long sahs_spade_modulate_workspace_words(long planes);
int sahs_spade_modulate(long planes, long hw, const float *x, const float *gamma, const float *beta, float eps, float slope, float *out,
                        float *stats, void *stream);

/* Its backward (Stage-II refiner training): given grad_out = dL/d out, with mean, r = 1 / sqrt(var + eps), xh = (x - mean) * r per plane,
 *   dy = grad_out * (out > 0 ? 1 : slope)      dbeta = dy      dgamma = dy * xh
 *   dx = r * (dxh - mean(dxh) - xh * mean(dxh * xh)),   dxh = dy * (1 + gamma),   means over the plane's hw elements.
 * x, gamma, out: what sahs_spade_modulate read and wrote; stats: its workspace exactly as that call left it for this x (mean and r are
 * re-formed from it as the forward formed them).  The activation mask is taken from `out` (out > 0 exactly when the pre-activation is, for
 * slope >= 0; at 0 the factor is slope, as in ATen's leaky_relu_backward); out may be null only when slope == 1, where it is not read.
 * slope < 0 is invalid here (the forward accepts it).  Each of dx, dgamma, dbeta may be null (not wanted), not all three; work:
 * sahs_spade_modulate_backward_workspace_words(planes) floats, needed for dx.  planes <= 65535 (gridDim.y; more is an invalid argument).
 * Two launches (chunk sums, then apply), no atomics: results are bit-reproducible.  16-byte accesses where hw % 4 == 0 and every
 * pointer given is 16-byte aligned, element by element otherwise. */
long sahs_spade_modulate_backward_workspace_words(long planes);
int sahs_spade_modulate_backward(long planes, long hw, const float *x, const float *gamma, const float *out, const float *stats,
                                 const float *grad_out, float eps, float slope, float *dx, float *dgamma, float *dbeta, float *work,
                                 void *stream);

/* The same two calls with bf16 tensors (the refiner under torch.autocast, where the convolutions produce bf16): x, gamma, beta, out,
 * grad_out, dx, dgamma, dbeta hold bf16 bit patterns (2 bytes per element; 10 B of traffic per element forward and 22 B backward, half
 * of the fp32 calls').  stats and work stay fp32, with the sizes the *_workspace_words functions above return, and the stats a
 * sahs_spade_modulate_bf16 call left are what sahs_spade_modulate_backward_bf16 reads (never mix them with the fp32 calls': the
 * statistics are those of another tensor).  All arithmetic is fp32 -- operands are widened on load, the sums, mean, r and the two
 * backward means are formed as the fp32 calls form them -- and each result is rounded to bf16 once, to nearest even, on store; the
 * activation mask is out > 0 on the stored bf16 value.  Arguments and refusals as for sahs_spade_modulate_backward, in BOTH calls:
 * planes <= 65535 (more is an invalid argument whose message names the limit), and for the backward slope >= 0, out null only for
 * slope 1, at least one of dx / dgamma / dbeta, work for dx.  Access width: 16 bytes (8 bf16) per operand and thread where hw % 8 == 0
 * and every pointer given is 16-byte aligned; element by element otherwise.  Two launches each, no atomics, bit-reproducible. */
int sahs_spade_modulate_bf16(long planes, long hw, const unsigned short *x, const unsigned short *gamma, const unsigned short *beta, float eps,
                             float slope, unsigned short *out, float *stats, void *stream);
int sahs_spade_modulate_backward_bf16(long planes, long hw, const unsigned short *x, const unsigned short *gamma, const unsigned short *out,
                                      const float *stats, const unsigned short *grad_out, float eps, float slope, unsigned short *dx,
                                      unsigned short *dgamma, unsigned short *dbeta, float *work, void *stream);

/* ---- Stage-II inference: the modulation with gamma / beta frozen (sahs-deformable-nerf_amd/spade.py: freeze_identity) ----
 *   out[b,c,i,j] = lrelu_slope( (X[b,c,i,j] - mean[b,c]) * rstd[b,c] * (1 + gamma[g,c,i,j]) + beta[g,c,i,j] )
 * x is (batch, channels, h, w), out (batch, channels, H, W), gamma and beta (map_batch, channels, H, W), all contiguous NCHW.
 * map_batch == 1: ONE map shared by every frame of the batch (g = 0; it is what a frozen identity photo yields), loaded once per
 * (channel, position) and applied to all `batch` frames -- fp32 traffic per element 4 (statistics) + 8 + 8 / batch, where the
 * per-frame call moves 20.  map_batch == batch: g = b.  Any other map_batch is an invalid argument.
 * up == 0: X = x, (H, W) = (h, w).  up == 1: X[b,c,i,j] = x[b,c,i>>1,j>>1], (H, W) = (2h, 2w) -- the layer applied to the nearest-
 * neighbour 2x upsample of x, which is never formed: mean and rstd are the statistics of the SOURCE plane (every source value occurs
 * exactly four times in X, so mean and biased variance are the same), read over h * w elements.
 * The statistics passes and the per-element arithmetic are sahs_spade_modulate's own, so for up == 0 the output is bit for bit that
 * call's (with the shared map repeated), and for up == 1 each phase out[:, :, di::2, dj::2] is bit for bit that call's on x with the
 * phase of gamma and beta.  Inference only: there is no backward.  stats: sahs_spade_modulate_frozen_workspace_words(batch, channels)
 * floats.  The channel is one gridDim.y slot and the batch is a loop inside the kernel: channels <= 65535 (more is an invalid argument
 * whose message names the limit); batch * channels is NOT limited.  Access width: 16 bytes per operand and thread where the output
 * row (up == 1; the plane for up == 0) divides into groups of 4 floats and every pointer is 16-byte aligned -- with up == 1 the source
 * is read 8 bytes at a time and needs 8-byte alignment; element by element otherwise.  Three launches (more statistics launches
 * beyond 65535 planes), no atomics, bit-reproducible.
 * The _bf16 entry: x, gamma, beta, out are bf16 bit patterns, groups of 8; arithmetic, statistics and workspace stay fp32. */
long sahs_spade_modulate_frozen_workspace_words(long batch, long channels);
int sahs_spade_modulate_frozen(long batch, long channels, long h, long w, long map_batch, int up, const float *x, const float *gamma,
                               const float *beta, float eps, float slope, float *out, float *stats, void *stream);
int sahs_spade_modulate_frozen_bf16(long batch, long channels, long h, long w, long map_batch, int up, const unsigned short *x,
                                    const unsigned short *gamma, const unsigned short *beta, float eps, float slope, unsigned short *out,
                                    float *stats, void *stream);

/* ---- Stage-II refiner training: spectral norm of a table of weights, fused ----
 * torch.nn.utils.spectral_norm's SpectralNorm.compute_weight (dim 0, n_power_iterations 1) for up to SAHS_SPECTRAL_NORM_MAX_JOBS weights
 * of mixed shapes per call.  Job k is a weight viewed as a contiguous row-major h[k] x w[k] fp32 matrix W (h = out channels,
 * w = in * kh * kw) with its vectors u (h) and v (w).  W, u, v, out, saved, grad_out, dW are HOST arrays of `jobs` device pointers,
 * h and w host arrays of ints; they are read before the call returns and travel to the kernels as arguments (no device-side table, no
 * allocation, no synchronisation).
 *   power_iteration = 1 (training):  t = W^T u,  v <- t / max(|t|_2, eps);   s = W v,  u <- s / max(|s|_2, eps);   sigma = u . s
 *   power_iteration = 0 (eval):      u, v are read only,  sigma = u . (W v)
 *   out = W / sigma
 * With power_iteration = 1 the job's u and v are updated IN PLACE (they are the module's buffers).  The u, v and sigma that formed the
 * output are also written to the job's saved area, h + w + 1 floats (u, then v, then sigma), which is what the backward reads -- so a
 * second forward on the same u, v before the first one's backward disturbs nothing (torch clones them for that reason).  out_bf16 = 0:
 * out holds floats; otherwise bf16 bit patterns, the fp32 quotient rounded once, to nearest even, on store.  All arithmetic is fp32.
 * W = 0 gives sigma = 0 and a non-finite out, as in torch.
 *   backward:  dW = G / sigma - (sum(G o W) / sigma^2) u v^T      (u, v constants of the graph, as in torch)
 * G = grad_out = dL/d out, fp32 (grad_bf16 = 0) or bf16 bit patterns widened on load; W and saved as the forward read and left them;
 * dW fp32.
 * Launches, whatever `jobs`: forward two (u, v, sigma: one workgroup per job; then out = W / sigma over the chip), backward one (a
 * workgroup per job).  Every sum has a fixed order and there are no atomics: results are bit-reproducible.  16-byte accesses where
 * w % 4 == 0 (w % 8 == 0 for a bf16 out or grad_out) and the pointers -- W, out, grad_out, dW and saved + h -- are 16-byte aligned;
 * element by element otherwise, job by job.
 * Invalid, refused with a message that names it before anything is launched: jobs < 1 or > SAHS_SPECTRAL_NORM_MAX_JOBS; a null table
 * or a null pointer in one; h < 1, w < 1 or h * w >= 2^31; eps <= 0; power_iteration other than 0 or 1. */
#define SAHS_SPECTRAL_NORM_MAX_JOBS 32
int sahs_spectral_norm_forward(int jobs, const float *const *W, float *const *u, float *const *v, void *const *out, float *const *saved,
                               const int *h, const int *w, int out_bf16, int power_iteration, float eps, void *stream);
int sahs_spectral_norm_backward(int jobs, const float *const *W, const float *const *saved, const void *const *grad_out, float *const *dW,
                                const int *h, const int *w, int grad_bf16, void *stream);

/* ---- image metrics: L1, MSE and windowed SSIM of two image batches, fused (the reference scores frames with scikit-image: nerf/metrics.py) ----
 * a, b: B images of H x W pixels and C channels (1 .. 4), both SAHS_IMAGE_U8 (unsigned bytes, scored as x / 255) or both SAHS_IMAGE_F32,
 * each addressed by its own four ELEMENT strides stride[0..3] = (batch, row, column, channel), host arrays read before the call
 * returns: (H, W, C) arrays, (B, C, H, W) network outputs and cropped views are read in place.  Strides are >= 0.
 * SSIM is skimage.metrics.structural_similarity with its defaults and multichannel=True: a 7 x 7 uniform window, sample covariance
 * (the 49/48 normalisation), C1 = (0.01 R)^2, C2 = (0.03 R)^2 with R = ssim_data_range in the units of x / 255 resp. the floats, and
 * the mean over the (H - 6)(W - 6) windows that lie inside the image (its crop(S, 3).mean(), so no border mode enters), per channel,
 * then over the channels.  Values outside [0, R] are not an error.
 * out: B rows of 3 + C doubles, [mean SSIM, MSE, L1, SSIM of channel 0 .. C - 1]; MSE and L1 are means over H * W * C elements.
 * workspace: sahs_image_metrics_workspace_bytes(B, H, W, C) bytes, 8-byte aligned (one record of C + 2 doubles per image and tile of
 * SAHS_IMAGE_METRICS_TILE^2 window origins); 0 from the query means the shape is invalid.
 * Two launches whatever B is, no atomics, every sum in a fixed order: results are bit-reproducible and a batch gives the bits of its
 * single calls.  uint8: the window moments, sum |d| and sum d^2 are exact integers; fp32: the moments are centred (a shift per tile
 * and channel) and summed in float64.
 * Invalid, refused before any HIP call: a null a, b, stride array, out or workspace; B < 0 (B == 0 succeeds without a launch) or
 * B * tiles >= 2^31; H < 7 or W < 7 (skimage raises there as well) or > 32768; C outside 1 .. 4; a dtype other than the two; a
 * negative stride; ssim_data_range not finite or <= 0; a or b not aligned to its element, out or workspace not to 8 bytes;
 * workspace_bytes below the query's value. */
#define SAHS_IMAGE_U8 0
#define SAHS_IMAGE_F32 1
#define SAHS_IMAGE_METRICS_TILE 32
size_t sahs_image_metrics_workspace_bytes(long B, int H, int W, int C);
int sahs_image_metrics(const void *a, const void *b, int dtype, long B, int H, int W, int C, const long *stride_a, const long *stride_b,
                       double ssim_data_range, double *out, void *workspace, size_t workspace_bytes, void *stream);

/* ---- image loss: clamp, MSE, L1 and windowed SSIM as one differentiable objective, fused (the reference's Stage-II step trains on
 * the MSE of the clamped output and keeps the l2 + l1 variant one comment away: train_get_texture_photo_audio.py:189-191) ----
 *   loss = w_l2 MSE(x, t) + w_l1 L1(x, t) + w_ssim (1 - SSIM(x, t)),   x = clamp(pred, 0, 1) when clamp != 0, else pred.
 * pred, target: B fp32 images of H x W pixels and C channels (1 .. 4), each addressed by its own four ELEMENT strides
 * (batch, row, column, channel) as sahs_image_metrics addresses them: host arrays read before the call returns, strides >= 0.
 * MSE and L1 are means over H * W * C elements; SSIM is sahs_image_metrics' (7 x 7 uniform window, sample covariance, C1 = (0.01 R)^2,
 * C2 = (0.03 R)^2 with R = ssim_data_range, the mean over the (H - 6)(W - 6) windows inside the image, then over the channels).
 * out: 4 + 3 B doubles: [loss, MSE, L1, mean SSIM] of the batch -- the means of the rows -- then one row [MSE, L1, mean SSIM] per image.
 * grad: null, or B fp32 images addressed by stride_grad (distinct elements: every one is written once, by one thread).  It receives
 * the gradient with respect to pred of EACH IMAGE'S OWN loss, w_l2 MSE_b + w_l1 L1_b + w_ssim (1 - SSIM_b): the gradient of the
 * batch's loss under an upstream gradient g is grad * (g / B), one scaling, which is the caller's.  The clamp passes the gradient
 * where 0 <= pred <= 1, both ends included (and -0.0 with them); L1's derivative at x == t is 0.  With grad null no gradient work is
 * done, and out has the same bits.
 * workspace: sahs_image_loss_workspace_bytes(B, H, W, C) bytes, 8-byte aligned (one record of C + 2 doubles per image and tile of
 * SAHS_IMAGE_LOSS_TILE^2 pixels); 0 from the query means the shape is invalid.
 * Two launches whatever B is, no atomics, every sum in float64 and in a fixed order that does not depend on B: results are
 * bit-reproducible, and a batch gives the bits of its single calls, rows and gradient alike.  The window moments are centred (a shift
 * per tile and channel), and the gradient's window coefficients are formed in the shifted frame.
 * Invalid, refused before any HIP call: a null pred, target, stride array, out or workspace, or a grad without stride_grad; B < 0
 * (B == 0 succeeds without a launch) or B * tiles >= 2^31; H < 7 or W < 7 or > 32768; C outside 1 .. 4; a negative stride; a weight
 * that is not finite; ssim_data_range not finite or <= 0; pred, target or grad not aligned to its 4-byte element, out or workspace
 * not to 8 bytes; workspace_bytes below the query's value. */
#define SAHS_IMAGE_LOSS_TILE 32
size_t sahs_image_loss_workspace_bytes(long B, int H, int W, int C);
int sahs_image_loss(const float *pred, const float *target, long B, int H, int W, int C, const long *stride_pred, const long *stride_target,
                    double w_l2, double w_l1, double w_ssim, int clamp, double ssim_data_range, float *grad, const long *stride_grad,
                    double *out, void *workspace, size_t workspace_bytes, void *stream);

/* ---- LPIPS (net = alex, v0.1): the scaling layer and the distance head, fused (the reference scores frames with the lpips package:
 * nerf/metrics.py).  The five AlexNet feature maps between the two calls are the caller's convolutions (metrics.py: LPIPS).
 * sahs_lpips_prepare -- a, b: B images of H x W pixels and 3 channels, both SAHS_IMAGE_U8 (taken as x / 255) or both SAHS_IMAGE_F32,
 * addressed by four ELEMENT strides (batch, row, column, channel) as sahs_image_metrics addresses them.  out: ONE contiguous
 * (2B, 3, H, W) fp32 tensor, rows [0, B) from a and rows [B, 2B) from b, every element written once:
 *   x' = ((normalize ? 2x - 1 : x) - shift_c) / scale_c,   shift = (-0.030, -0.088, -0.188),  scale = (0.458, 0.448, 0.450),
 * each step one correctly rounded fp32 operation.  normalize = 0 is the reference's call (images in [0, 1] passed as they are), 1 the
 * metric's authors' (images mapped to [-1, 1] first).  One launch.
 * sahs_lpips_distance -- job l (1 .. SAHS_LPIPS_MAX_JOBS of them, one per layer) is a contiguous (2B, C[l], h, w) NCHW fp32 feature
 * tensor features[l] whose rows [0, B) belong to a and [B, 2B) to b, its C[l] channel weights weights[l] (fp32), and hw[l] = h * w.
 * features, weights, C, hw are HOST arrays read before the call returns; the table travels to the kernels as arguments.  Per pixel,
 * with na = sqrt(sum_c a_c^2) + 1e-10 and nb likewise,
 *   d = sum_c w_c (a_c / na - b_c / nb)^2 = sum w a^2 / na^2 + sum w b^2 / nb^2 - 2 sum w a b / (na nb),
 * the five channel sums in float64 (each feature value is read once); d_l is the mean of d over the layer's hw[l] pixels.
 * out: B rows of 1 + SAHS_LPIPS_MAX_JOBS doubles, [sum_l d_l, d_0, d_1, ...] (0 for layers beyond `jobs`).  Equal features give exactly
 * 0; a pixel whose features are all zero gives 0, not NaN.
 * workspace: sahs_lpips_distance_workspace_bytes(jobs, B, hw) bytes, 8-byte aligned (one double per image, layer and tile of
 * SAHS_LPIPS_TILE pixels); 0 from the query means the shapes are invalid.
 * Two launches whatever B and jobs are, no atomics, every sum in a fixed order: results are bit-reproducible and a batch gives the
 * bits of its single calls.
 * Invalid, refused with a message that names it before any HIP call: a null pointer (B == 0 succeeds without a launch); B < 0;
 * prepare: C != 3, a dtype other than the two, H or W < SAHS_LPIPS_MIN_SIDE (a smaller image leaves AlexNet's second max-pool
 * nothing) or > 32768, a negative stride, a misaligned pointer; distance: jobs outside 1 .. SAHS_LPIPS_MAX_JOBS, C[l] outside
 * 1 .. SAHS_LPIPS_MAX_CHANNELS, hw[l] outside 1 .. 2^30, B * tiles >= 2^31, a null or misaligned features[l] or weights[l],
 * workspace_bytes below the query's value. */
#define SAHS_LPIPS_TILE 256
#define SAHS_LPIPS_MAX_JOBS 5
#define SAHS_LPIPS_MAX_CHANNELS 1024
#define SAHS_LPIPS_MIN_SIDE 31
int sahs_lpips_prepare(const void *a, const void *b, int dtype, long B, int H, int W, int C, const long *stride_a, const long *stride_b,
                       int normalize, float *out, void *stream);
size_t sahs_lpips_distance_workspace_bytes(int jobs, long B, const long *hw);
int sahs_lpips_distance(int jobs, const float *const *features, const float *const *weights, const int *C, const long *hw, long B,
                        double *out, void *workspace, size_t workspace_bytes, void *stream);

/* ---- LPIPS as a training term: the same two ends, differentiable with respect to the FIRST operand (pred) only; the convolutions
 * between them, and their backward, stay the caller's.  Not twice differentiable.
 * sahs_lpips_prepare_loss -- sahs_lpips_prepare with pred fp32, target SAHS_IMAGE_U8 or SAHS_IMAGE_F32 (target_dtype), and a clamp
 * flag: clamp != 0 applies min(max(x, 0), 1) to pred alone, ahead of the optional 2x - 1 and the scaling layer (a NaN stays a NaN).
 * out: the one (2B, 3, H, W) tensor, rows [0, B) from pred.  One launch; sahs_lpips_prepare is this kernel with the flag off.
 * sahs_lpips_prepare_grad -- its backward, one launch, a thread per pixel.  gx: the contiguous (B, 3, H, W) fp32 gradient of rows
 * [0, B) of out.  grad, B images addressed by stride_grad (distinct elements, each written once), receives
 *   grad[c] = gx[c] / scale_c   (one correctly rounded fp32 division; times 2, exact, when normalize != 0),
 * and +0 where clamp != 0 and pred is not in [0, 1] (both ends pass; a NaN pred passes nothing), as torch.clamp's backward gives.
 * sahs_lpips_head_forward -- sahs_lpips_distance with each layer's two operands as two contiguous (B, C[l], h, w) tensors fa[l], fb[l];
 * out and workspace as there (sahs_lpips_distance_workspace_bytes), and the same bits: sahs_lpips_distance is this entry with
 * fb[l] = features[l] + B C[l] hw[l].  stats: null, or sahs_lpips_head_stats_bytes(jobs, B, hw) bytes, 8-byte aligned, which receive
 * what the backward needs of each pixel's five sums -- with sa = sum a^2, swa = sum w a^2, swab = sum w a b:
 *   ra = 1 / na,   rb = 1 / nb,   q = (swa / na - swab / nb) / (sqrt(sa) na),   q = 0 where sa == 0
 * -- as three planes of B * sum_l hw[l] doubles (24 bytes per pixel beside its 8 C[l] bytes of features).  It is a buffer of its own,
 * not part of the workspace, because it must live until the backward and the workspace need not.  out has the same bits either way.
 * sahs_lpips_head_backward -- one launch over all layers (the forward's job table and tile mapping, a thread per pixel walking the
 * channels; fa, fb, weights, C, hw, B and stats as the forward had them).  g: the upstream gradient of each image's LPIPS, B doubles
 * (g_is_double != 0) or B floats, widened.  grad_a[l], fa[l]'s shape, every element written once, no atomics:
 *   grad_a[c] = (float)( (2 g_i / hw) ra ( w_c (a_c ra - b_c rb) - a_c q ) ),   float64 arithmetic, rounded to fp32 once;
 * this is d/da_c of g_i * mean over pixels of sum_c w_c (a_c / na - b_c / nb)^2.  At a pixel whose a is all zero a -> a / (|a| + 1e-10)
 * has the Jacobian I / 1e-10, so q = 0 there is the derivative itself: the result is large (2 w_c b_c rb 1e10 g_i / hw) and finite, where
 * autograd of the published formula gives NaN (sqrt's derivative at 0).  Equal operands give a gradient that is exactly 0.
 * Invalid, refused with a message that names it before any HIP call: as sahs_lpips_prepare and sahs_lpips_distance refuse, for the
 * tables fa and fb alike; a null gx, grad, stride_grad, g, stats (backward) or grad_a[l]; a negative stride; a misaligned pointer
 * (g to its 4- or 8-byte element); stats_bytes below the query's value. */
int sahs_lpips_prepare_loss(const float *pred, const void *target, int target_dtype, long B, int H, int W, int C, const long *stride_pred,
                            const long *stride_target, int normalize, int clamp, float *out, void *stream);
int sahs_lpips_prepare_grad(const float *pred, const float *gx, long B, int H, int W, int C, const long *stride_pred, int normalize, int clamp,
                            float *grad, const long *stride_grad, void *stream);
size_t sahs_lpips_head_stats_bytes(int jobs, long B, const long *hw);
int sahs_lpips_head_forward(int jobs, const float *const *fa, const float *const *fb, const float *const *weights, const int *C, const long *hw,
                            long B, double *out, double *stats, size_t stats_bytes, void *workspace, size_t workspace_bytes, void *stream);
int sahs_lpips_head_backward(int jobs, const float *const *fa, const float *const *fb, const float *const *weights, const int *C, const long *hw,
                             long B, const void *g, int g_is_double, const double *stats, size_t stats_bytes, float *const *grad_a, void *stream);

/* ---- frame products: the bytes Stage-I evaluation writes for a rendered frame, fused (the reference's eval_stage_rays.py tail: image
 * and disparity casts, torch_normal_map, nerf/utils.py label2color) ----
 * For B frames of H x W pixels.  Inputs (device pointers):
 *   rgb    fp32, C = 3 or C = 15 channels per pixel ([rgb3 | seg12], as the renderer emits it), addressed by three ELEMENT strides
 *          stride_rgb[0..2] = (batch, row, column), a host array read before the call returns; the channel stride is 1.  The (H W, 15)
 *          render output, its [..., :3] view and a stacked (B, H, W, 15) are read in place.  May be null when neither image nor seg is asked for.
 *   disp   fp32 (B, H, W) contiguous, or null.     w_bg  fp32 (B, H, W) contiguous, or null; read only when clean != 0.
 *   intrinsics  HOST array [fx, fy, cx, cy], cx and cy as fractions of the width and the height, or null.
 * Outputs (device pointers, each contiguous, each optional: null = not asked for):
 *   image       u8 (B, H, W, 3): clamp(x, 0, 1) * 255 in fp32, truncated.
 *   seg         u8 (B, H, W, 3): the colour of the arg-max of the 12 scores rgb[..., 3:15]; the first maximum wins and a NaN counts as
 *               the maximum (numpy's argmax).  Needs C = 15.
 *   normals_u8  u8 (B, H - d, W - d, 3) and / or normals_f32, fp32 of the same shape; d = 2 with central_difference, else 1.  With
 *               p(r, c) = [((c - cx W) t) / fx, -((r - cy H) t) / fy, t], t = disp[r][c]:  n = cross(p(r, c + d) - p(r, c), p(r + d, c) - p(r, c)),
 *               v = (n / |n|) * 0.5 + 0.5; with clean != 0 and w_bg given, m = w_bg[r][c]: v = 1 where m > 0.22, then v = (1 - m) v + m;
 *               normals_f32 = v * 255 (not clamped), normals_u8 = clamp(v * 255, 0, 255) truncated.  RECTANGULAR maps: the column index
 *               enters x with cx * W and the row index enters y with cy * H; for square maps this is the reference's function.
 *               H <= d or W <= d: the plane is empty and nothing is written to it.  Needs disp and intrinsics.
 *   disparity   u8 (B, H, W): (t - min) / (max - min) with min and max PER FRAME, an fp32 subtraction and a correctly rounded fp32
 *               division, then clamp(., 0, 1) * 255 truncated.  Needs disp.
 * Every step is one correctly rounded fp32 operation in the order written above.
 * NaN rule: any NaN that reaches a byte conversion is stored as 0, in every plane.  min and max propagate NaN: a frame whose disparity
 * holds a NaN gets an all-zero disparity plane (the other frames of the batch are not affected), and so does a constant frame (0 / 0).
 * workspace: sahs_frame_products_workspace_bytes(B, H, W) bytes, 16-byte aligned (one record of 16 bytes per frame and tile of
 * SAHS_FRAME_PRODUCTS_TILE^2 pixels); 0 from the query means the shape is invalid (or B == 0).  Needed only with disparity.
 * At most two launches whatever B is, no atomics: bit-reproducible, and a batch gives the bits of its single calls.
 * Invalid, refused with a message that names it before any HIP call: H or W outside 1 .. 32768; B < 0 (B == 0 succeeds without a
 * launch) or B * tiles >= 2^31; C other than 3 or 15; seg with C = 3; normals without disp and intrinsics; disparity without disp;
 * image or seg without rgb or stride_rgb; a negative stride; intrinsics with fx or fy zero or not finite; a pointer not aligned to its
 * element (workspace: 16 bytes); workspace_bytes below the query's value when disparity is asked for. */
#define SAHS_FRAME_PRODUCTS_TILE 32
size_t sahs_frame_products_workspace_bytes(long B, int H, int W);
int sahs_frame_products(const float *rgb, int C, const long *stride_rgb, const float *disp, const float *w_bg, const float *intrinsics,
                        long B, int H, int W, int clean, int central_difference, unsigned char *image, unsigned char *seg,
                        unsigned char *normals_u8, float *normals_f32, unsigned char *disparity, void *workspace, size_t workspace_bytes,
                        void *stream);

/* ---- launch probe (opt-in measurement aid; the one exception to "never synchronises") ----
 * While armed on the calling thread, every FIELD-kernel launch the library makes (from any entry point above) is bracketed by two HIP
 * events recorded on the launch stream, up to `capacity` launches (further ones are counted as dropped and run unprobed).
 * sahs_probe_read(i) waits for launch i to finish and returns its duration, the number of sample evaluations it covered and
 * kind = model << 16 | level << 12 | part << 8 | precision   (part: 0 whole network, 1 deformation nets, 2 radiance nets; precision = that
 * of the KERNEL launched, e.g. SAHS_F32 for the deformation launches of a mixed-precision model).
 * bench.py times the kernels of run_one_iter_of_nerf's own call chain with it.  Events belong to the device current at arm time. */
int sahs_probe_arm(int capacity);
int sahs_probe_disarm(void);
int sahs_probe_count(void);
int sahs_probe_dropped(void);
int sahs_probe_read(int i, int *kind, long *samples, float *ms);

#ifdef __cplusplus
}
#endif
#endif /* SAHS_NERF_H */
