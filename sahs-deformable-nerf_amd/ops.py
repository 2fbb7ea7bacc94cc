"""Torch-facing ops over the C ABI: device memory and streams come from PyTorch, the arithmetic
is the HIP library's.  Every function requires CUDA(HIP) fp32 tensors and raises otherwise --
there is no eager/CPU path here.

autograd: ``RenderRaysFn`` (one ray chunk of predict_and_render_radiance) is the differentiable op.  Its forward picks one strategy -- "shared"
(split chain, activations kept), "whole" (whole-network saves kept) or "recompute" (depths only) -- and hands its backward the saved tensors
BY NAME (_save_named / _load_named; None = absent).  Its backward (_RenderBackward: composite backward, field walks, conditioning backward)
issues the same steps on one stream or, for the per-layer walks of "shared", pairwise on two, and returns gradients for the flat parameter
buffer and the driving input.  Importance resampling is not differentiated (the reference detaches it, train_utils.py:164).  The stand-alone
seams are differentiable too: ``FieldFn`` behind model(level, x, driving, pose), ``CompositeFn`` behind volume_render_radiance_field.
Stage II: ``SpadeModulateFn`` behind spade_modulate, taken only when one of its tensors needs a gradient; ``SpectralNormalizeFn`` behind
spectral_normalize (a list of weights in, their spectral-normalised forms out, one node), under the same rule.
"""
import ctypes
import os
import types

import torch

from . import _lib
from ._lib import SAHS_F32, SAHS_BF16, SAHS_BF16X3, check

PRECISIONS = {"fp32": SAHS_F32, "f32": SAHS_F32, "bf16": SAHS_BF16,
              "bf16x3": SAHS_BF16X3}    # near-fp32 on the bf16 pipe: every net with hi + lo bf16 operands (3 MFMAs per product); SAHS_X3_DEFORM=f32 keeps the deformation nets on the fp32 kernel


def is_mixed(arch, precision):
    """Precisions that exist as the split chain only (a deformation launch with split bf16 operands -- fp32 under SAHS_X3_DEFORM=f32 -- and a
    low-precision radiance launch, exchanging x', w)."""
    return (precision == SAHS_BF16 and arch == "nerface") or (precision == SAHS_BF16X3 and arch in ("audio", "nerface"))


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    """The launch stream: torch's current stream of the CURRENT device.  Every tensor handed to an op must live on that device
    (_req enforces it), so a kernel is never enqueued on another device's stream or launched without that device's attributes."""
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _req(t, name, dtype=torch.float32):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.SahsError("%s must be a GPU tensor (the HIP path has no CPU fallback)" % name)
    if t.dtype != dtype:
        raise _lib.SahsError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if t.device.index != torch.cuda.current_device():
        raise _lib.SahsError("%s lives on %s but the current device is cuda:%d: one process drives one GPU (call "
                             "torch.cuda.set_device first, as torchrun-style launchers do)" % (name, t.device, torch.cuda.current_device()))
    return t if t.is_contiguous() else t.contiguous()


ARCHS = ("audio", "nerface", "nerface_static")   # = SAHS_MODEL_AUDIO / _NERFACE / _NERFACE_STATIC of include/sahs_nerf.h


def _fn(name, arch="audio"):
    """sahs_model_<name> bound to the architecture: AudioFaceModel (config/audio) | NeRFaceModel (config/expression person_2/3)
    | NeRFaceModel without deformation (config/expression/person_1)."""
    if arch not in ARCHS:
        raise _lib.SahsError("unknown architecture %r" % (arch,))
    full = "sahs_model_" + name
    f = getattr(_lib.lib(), full)
    m = ARCHS.index(arch)
    return (lambda *a: f(m, *a)), full + "(%s)" % arch


def param_count(arch="audio"):
    return int(_fn("param_count", arch)[0]())


def executed_macs_per_sample(arch="audio", precision=SAHS_F32, part=0):
    """MACs per sample evaluation the field kernel issues to the matrix pipe (padded tiles, constants folded away); part 1 / 2: the
    deformation nets / the radiance net alone (the split evaluation)."""
    return int(_fn("executed_macs_part", arch)[0](precision, part))


def pack_weights(flat, precision=SAHS_F32, arch="audio"):
    flat = _req(flat, "flat_params")
    if flat.numel() != param_count(arch):
        raise _lib.SahsError("flat_params has %d values, expected %d" % (flat.numel(), param_count(arch)))
    words = _fn("packed_words", arch)[0](precision)
    if words <= 0:
        raise _lib.SahsError("precision %r is not built for architecture %r" % (precision, arch))
    packed = torch.empty(words, dtype=torch.float32, device=flat.device)
    f, name = _fn("pack_weights", arch)
    check(f(_p(flat), _p(packed), precision, _stream()), name)
    return packed


def fold_conditioning(flat, audio, pose, arch="audio"):
    """audio: the (16, 29) DeepSpeech window (AudioFaceModel) or the 76-d expression vector (NeRFaceModel)."""
    flat, audio = _req(flat, "flat_params"), _req(audio, "audio")
    pose = _req(pose, "pose")
    want = (16, 29) if arch == "audio" else (76,)   # NeRFaceModels: the expression vector
    if tuple(audio.shape) != want:
        raise _lib.SahsError("driving input must be %s for %r, got %s" % (want, arch, tuple(audio.shape)))
    if pose.dim() != 2 or pose.shape[0] < 3 or pose.shape[1] != 4:
        raise _lib.SahsError("pose must be (3|4, 4), got %s" % (tuple(pose.shape),))
    frame = torch.empty(_fn("frame_words", arch)[0](), dtype=torch.float32, device=flat.device)
    f, name = _fn("fold_conditioning", arch)
    check(f(_p(flat), _p(audio), _p(pose), 4, _p(frame), _stream()), name)
    return frame


def get_ray_bundle(height, width, intrinsics, c2w):
    c2w = _req(c2w, "tform_cam2world")
    fx, fy, cx, cy = [float(v) for v in intrinsics]
    ro = torch.empty(height, width, 3, dtype=torch.float32, device=c2w.device)
    rd = torch.empty_like(ro)
    check(_lib.lib().sahs_get_ray_bundle(int(height), int(width), fx, fy, cx, cy, _p(c2w), int(c2w.shape[-1]), _p(ro), _p(rd), _stream()),
          "sahs_get_ray_bundle")
    return ro, rd


def ray_uniforms(seed, stream_id, ray0, num_rays, num_samples, device):
    """(num_rays, num_samples) uniforms in [0,1) keyed by (seed, stream_id, global ray index ray0 + r, sample): the same ray
    gets the same draws however the frame is chunked or sharded."""
    out = torch.empty(int(num_rays), int(num_samples), dtype=torch.float32, device=device)
    check(_lib.lib().sahs_ray_uniforms(int(seed) & (2 ** 64 - 1), int(stream_id), int(ray0), int(num_rays), int(num_samples), _p(out), _stream()),
          "sahs_ray_uniforms")
    return out


def stratified_depths(rays, num_samples, lindisp=False, t_rand=None):
    rays, t_rand = _req(rays, "rays"), _req(t_rand, "t_rand")
    N = rays.shape[0]
    z = torch.empty(N, num_samples, dtype=torch.float32, device=rays.device)
    check(_lib.lib().sahs_stratified_depths(N, int(num_samples), _p(rays), int(rays.shape[1]), int(bool(lindisp)), _p(t_rand), _p(z),
                                             _stream()), "sahs_stratified_depths")
    return z


def field_forward(packed, frame, level, rays, z, precision=SAHS_F32, debug=False, out=None, arch="audio"):
    """raw (N,S,16) for level 0/1 at points ro + rd*z.  debug=True also returns (dx, w, grid)."""
    packed, frame, rays, z = _req(packed, "packed"), _req(frame, "frame"), _req(rays, "rays"), _req(z, "z")
    N, S = z.shape
    if rays.shape[0] != N or rays.shape[1] < 8:
        raise _lib.SahsError("rays must be (N, >=8) with N == z.shape[0]")
    raw = out if out is not None else torch.empty(N, S, 16, dtype=torch.float32, device=z.device)
    dbg = torch.zeros(N * S * 88, dtype=torch.float32, device=z.device) if debug else None
    f, name = _fn("field_forward", arch)
    check(f(_p(packed), _p(frame), int(level), N, S, _p(rays), int(rays.shape[1]), _p(z), _p(raw), _p(dbg), precision, _stream()), name)
    if debug == "full":
        return raw, dbg[: N * S * 56].view(N * S, 56), dbg[N * S * 56:].view(N * S, 32)
    if debug:
        a = dbg[: N * S * 56].view(N * S, 56)
        return raw, a[:, 0:3].reshape(N, S, 3), a[:, 3:5].reshape(N, S, 2), dbg[N * S * 56:].view(N, S, 32)
    return raw


def composite_forward(raw, z, rays, noise=None, bg=None, white_background=False):
    raw, z, rays, noise, bg = _req(raw, "radiance_field"), _req(z, "depth_values"), _req(rays, "rays"), _req(noise, "noise"), _req(bg, "background_prior")
    N, S = z.shape
    dev = z.device
    rgb = torch.empty(N, 15, dtype=torch.float32, device=dev)
    disp, acc, depth = (torch.empty(N, dtype=torch.float32, device=dev) for _ in range(3))
    weights = torch.empty(N, S, dtype=torch.float32, device=dev)
    check(_lib.lib().sahs_composite_forward(N, S, _p(raw), _p(z), _p(rays), int(rays.shape[1]), _p(noise), _p(bg), int(bool(white_background)),
                                             _p(rgb), _p(disp), _p(acc), _p(weights), _p(depth), _stream()), "sahs_composite_forward")
    return rgb, disp, acc, weights, depth


def resample(z, weights, num_fine, u=None, want_aux=False):
    z, weights, u = _req(z, "z_vals"), _req(weights, "weights"), _req(u, "u")
    N, S = z.shape
    z_out = torch.empty(N, S + num_fine, dtype=torch.float32, device=z.device)
    zs = torch.empty(N, num_fine, dtype=torch.float32, device=z.device) if want_aux else None
    inds = torch.empty(N, num_fine, dtype=torch.int64, device=z.device) if want_aux else None
    check(_lib.lib().sahs_resample(N, S, int(num_fine), _p(z), _p(weights), _p(u), _p(zs), _p(z_out), _p(inds), _stream()), "sahs_resample")
    return (z_out, zs, inds) if want_aux else z_out


def resample_merge(z, weights, num_fine, u=None):
    """resample that also returns the new samples and the merge permutation: (z_sorted (N,S+nf), z_new (N,nf), src (N,S+nf) int32)."""
    z, weights, u = _req(z, "z_vals"), _req(weights, "weights"), _req(u, "u")
    N, S = z.shape
    z_out = torch.empty(N, S + num_fine, dtype=torch.float32, device=z.device)
    z_new = torch.empty(N, num_fine, dtype=torch.float32, device=z.device)
    src = torch.empty(N, S + num_fine, dtype=torch.int32, device=z.device)
    check(_lib.lib().sahs_resample_merge(N, S, int(num_fine), _p(z), _p(weights), _p(u), _p(z_new), _p(z_out), _p(src), _stream()), "sahs_resample_merge")
    return z_out, z_new, src


FIELD_ALL, FIELD_DEFORM, FIELD_RADIANCE = 0, 1, 2


def field_forward_split(packed, frame, level, mode, rays, xw, z=None, src=None, xw_col0=0, out=None, arch="audio", precision=SAHS_F32,
                        validate_src=False):
    """The field in parts (include/sahs_nerf.h: sahs_model_field_forward_split).  xw: (N, row, 8) fp32 buffer of deformed points.
    FIELD_ALL: raw (N,S,16) for depths z, x'/w of its samples written to xw[:, xw_col0:xw_col0+S]; FIELD_DEFORM: only x'/w for depths z;
    FIELD_RADIANCE: raw for the samples xw[ray, src[ray, s]] (src (N,S) int32).  The kernel does not range-check src (precondition of the
    C ABI: 0 <= src < xw.shape[1]); validate_src=True checks a caller-made permutation here (one device reduction + sync)."""
    packed, frame, rays, z = _req(packed, "packed"), _req(frame, "frame"), _req(rays, "rays"), _req(z, "z")
    src = _req(src, "src", torch.int32)
    xw = _req(xw, "xw")
    N = rays.shape[0]
    S = src.shape[1] if mode == FIELD_RADIANCE else z.shape[1]
    if xw.dim() != 3 or xw.shape[0] != N or xw.shape[2] != 8:
        raise _lib.SahsError("xw must be (N, row, 8)")
    if src is not None and (src.dim() != 2 or src.shape[0] != N):
        raise _lib.SahsError("src must be (N, S)")
    if validate_src and src is not None and src.numel() and not (0 <= int(src.min()) and int(src.max()) < xw.shape[1]):
        raise _lib.SahsError("src indexes outside xw's %d slots per ray" % xw.shape[1])
    raw = None
    if mode != FIELD_DEFORM:
        raw = out if out is not None else torch.empty(N, S, 16, dtype=torch.float32, device=rays.device)
    f, name = _fn("field_forward_split", arch)
    check(f(_p(packed), _p(frame), int(precision), int(level), int(mode), N, int(S), _p(rays), int(rays.shape[1]), _p(z), _p(raw), _p(xw), int(xw.shape[1]), int(xw_col0),
            _p(src), _stream()), name)
    return raw


def sample_pdf(bins, weights, num_samples, u=None, want_inds=False):
    bins, weights, u = _req(bins, "bins"), _req(weights, "weights"), _req(u, "u")
    N, nb = bins.shape
    if tuple(weights.shape) != (N, nb - 1):
        raise _lib.SahsError("weights must be (N, nb-1)")
    out = torch.empty(N, num_samples, dtype=torch.float32, device=bins.device)
    inds = torch.empty(N, num_samples, dtype=torch.int64, device=bins.device) if want_inds else None
    check(_lib.lib().sahs_sample_pdf(N, nb, int(num_samples), _p(bins), _p(weights), _p(u), _p(out), _p(inds), _stream()), "sahs_sample_pdf")
    return (out, inds) if want_inds else out


def _workspace_buffer(ws, dev, name, shape, dtype=torch.float32):
    """The buffer ``name`` of a render workspace (a dict the caller keeps between calls), made anew when its shape or the device changed."""
    t = ws.get(name)
    if t is None or tuple(t.shape) != tuple(shape) or t.device != dev:
        t = ws[name] = torch.empty(*shape, dtype=dtype, device=dev)
    return t


def _req_rows(rows, N):
    if not (isinstance(rows, torch.Tensor) and rows.is_cuda and rows.dtype == torch.float32 and rows.dim() == 2 and rows.shape[0] == N
            and rows.shape[1] >= ROW_COLUMNS and rows.stride(1) == 1):
        raise _lib.SahsError("rows must be a GPU fp32 (N, >=36) tensor with unit column stride")


def render_rays(packed, frame, rays, num_coarse, num_fine, precision=SAHS_F32, lindisp=False, white_background=False, bg=None,
                t_rand=None, noise_c=None, u=None, noise_f=None, workspace=None, arch="audio"):
    """predict_and_render_radiance for one ray chunk -> the reference's 8-tuple (flat shapes)."""
    if is_mixed(arch, precision):      # mixed precision exists as the row-writing split chain only
        rows = torch.empty(rays.shape[0], ROW_COLUMNS, dtype=torch.float32, device=rays.device)
        render_rays_rows(packed, frame, rays, num_coarse, num_fine, rows, precision=precision, lindisp=lindisp, white_background=white_background,
                         bg=bg, t_rand=t_rand, noise_c=noise_c, u=u, noise_f=noise_f, workspace=workspace, arch=arch)
        return tuple(c.contiguous() for c in (rows[:, 0:15], rows[:, 15], rows[:, 16], rows[:, 17:32], rows[:, 32], rows[:, 33], rows[:, 34], rows[:, 35]))
    packed, frame, rays = _req(packed, "packed"), _req(frame, "frame"), _req(rays, "rays")
    bg, t_rand, noise_c, u, noise_f = (_req(t, n) for t, n in ((bg, "background_prior"), (t_rand, "t_rand"), (noise_c, "noise_c"),
                                                               (u, "u"), (noise_f, "noise_f")))
    N = rays.shape[0]
    dev = rays.device
    Sf = num_coarse + num_fine
    ws = workspace if workspace is not None else {}
    buf = lambda name, *shape: _workspace_buffer(ws, dev, name, shape)
    z_c, z_f = buf("z_c", N, num_coarse), buf("z_f", N, Sf)
    raw, weights = buf("raw", N, Sf, 16), buf("weights", N, Sf)
    rgb_c, rgb_f = (torch.empty(N, 15, dtype=torch.float32, device=dev) for _ in range(2))
    disp_c, acc_c, disp_f, acc_f, w_bg, depth_f = (torch.empty(N, dtype=torch.float32, device=dev) for _ in range(6))
    f, name = _fn("render_rays", arch)
    check(f(_p(packed), _p(frame), precision, N, _p(rays), int(rays.shape[1]), int(num_coarse), int(num_fine),
            int(bool(lindisp)), int(bool(white_background)), _p(bg), _p(t_rand), _p(noise_c), _p(u), _p(noise_f),
            _p(z_c), _p(z_f), _p(raw), _p(weights), _p(rgb_c), _p(disp_c), _p(acc_c), _p(rgb_f), _p(disp_f),
            _p(acc_f), _p(w_bg), _p(depth_f), _stream()), name)
    if num_fine > 0:
        return rgb_c, disp_c, acc_c, rgb_f, disp_f, acc_f, w_bg, depth_f
    return rgb_c, disp_c, acc_c, None, None, None, w_bg, depth_f


_SPARSE_BRANCHES = True
_SPARSE_MAX_SAMPLES = 1 << 30      # a record's header holds the sample index as an int: a larger pass renders dense


def sparse_branches(on=None):
    """The fp32 inference render (render_rays_rows) skips the colour and seg branches of samples the composite gives the weight exactly 0
    (sigma + noise <= 0; with a background prior also the last sample of a ray): include/sahs_nerf.h, sahs_model_render_rays_rows_sparse.
    The rendered rows are bit-identical either way; in the `raw` workspace columns 0..14 of a zero-weight sample then hold the output
    biases, not its logits.  sparse_branches(False) keeps the dense launches (the A/B reference).  None queries -> bool."""
    global _SPARSE_BRANCHES
    if on is not None:
        if not isinstance(on, (bool, int)) or on not in (0, 1, False, True):
            raise _lib.SahsError("sparse_branches: True or False, not %r" % (on,))
        _SPARSE_BRANCHES = bool(on)
    return _SPARSE_BRANCHES


def _sparse_head(workspace, who):
    rec = workspace.get("sparse") if workspace else None
    if rec is None:
        raise _lib.SahsError("%s: this workspace has not been through a sparse render" % who)
    return rec[:8].view(torch.int32)


def sparse_last_count(workspace):
    """Live records the last pass of a render_rays_rows call counted, read back from the record workspace kept in ``workspace``: a
    measurement aid -- it synchronises."""
    return int(_sparse_head(workspace, "sparse_last_count")[0].item())


def sparse_last_path(workspace):
    """1 once a sparse pass ran through ``workspace`` (the second head word of its record workspace); it synchronises."""
    return int(_sparse_head(workspace, "sparse_last_path")[1].item())


ROW_COLUMNS = 36      # SAHS_ROW_* of include/sahs_nerf.h: rgb_c 0:15, disp_c 15, acc_c 16, rgb_f 17:32, disp_f 32, acc_f 33, w_bg 34, depth_f 35


def composite_forward_rows(raw, z, rays, rows, fine_pass, noise=None, bg=None, white_background=False, weights=None):
    """composite_forward writing its ray outputs into the (N, 36) row block ``rows`` (coarse pass: columns 0..16; fine pass: 17..35);
    returns the dense (N, S) weights."""
    raw, z, rays, noise, bg = _req(raw, "radiance_field"), _req(z, "depth_values"), _req(rays, "rays"), _req(noise, "noise"), _req(bg, "background_prior")
    N, S = z.shape
    _req_rows(rows, N)
    if weights is None or tuple(weights.shape) != (N, S):
        weights = torch.empty(N, S, dtype=torch.float32, device=z.device)
    check(_lib.lib().sahs_composite_forward_rows(N, S, _p(raw), _p(z), _p(rays), int(rays.shape[1]), _p(noise), _p(bg), int(bool(white_background)),
                                                  _p(weights), _p(rows), int(rows.stride(0)), int(bool(fine_pass)), _stream()), "sahs_composite_forward_rows")
    return weights


def render_rays_rows(packed, frame, rays, num_coarse, num_fine, rows, precision=SAHS_F32, lindisp=False, white_background=False, bg=None,
                     t_rand=None, noise_c=None, u=None, noise_f=None, workspace=None, arch="audio", share_deformation=True):
    """predict_and_render_radiance for one ray chunk, written IN PLACE into ``rows`` (N, 36): the 8-tuple of every ray side by
    side (a row block of the frame's (R, 36) buffer, which is also what the multi-GPU all-gather moves), so a chunk loop needs
    no per-chunk concatenation.  Returns ``rows``.  share_deformation (fp32; bf16 for the audio model): evaluate the deformation nets once per depth -- the fine
    pass reuses the coarse samples' deformed points instead of recomputing them as the reference does; identical results."""
    packed, frame, rays = _req(packed, "packed"), _req(frame, "frame"), _req(rays, "rays")
    bg, t_rand, noise_c, u, noise_f = (_req(t, n) for t, n in ((bg, "background_prior"), (t_rand, "t_rand"), (noise_c, "noise_c"),
                                                               (u, "u"), (noise_f, "noise_f")))
    N = rays.shape[0]
    _req_rows(rows, N)
    dev = rays.device
    Sf = num_coarse + num_fine
    ws = workspace if workspace is not None else {}
    buf = lambda name, *shape: _workspace_buffer(ws, dev, name, shape)
    z_c, z_f = buf("z_c", N, num_coarse), buf("z_f", N, Sf)
    raw, weights = buf("raw", N, Sf, 16), buf("weights", N, Sf)
    xw = src = z_new = None
    mixed = is_mixed(arch, precision)      # split-operand deformation launch + low-precision radiance launch: only the split chain exists
    if mixed and not (share_deformation and num_fine > 0):
        raise _lib.SahsError("a mixed-precision model renders through the split chain (share_deformation=True, num_fine > 0)")
    if share_deformation and num_fine > 0 and arch != "nerface_static" and precision in (SAHS_F32, SAHS_BF16, SAHS_BF16X3):
        # extra workspace of the split evaluation: deformed points of every depth, the merge permutation, the new depths
        xw, z_new = buf("xw", N, Sf, 8), buf("z_new", N, num_fine)
        src = _workspace_buffer(ws, dev, "src", (N, Sf), torch.int32)
    extra = []
    if _SPARSE_BRANCHES and precision == SAHS_F32 and 0 < N * Sf <= _SPARSE_MAX_SAMPLES:
        # record workspace of the sparse branches: the workgroups' rings of the fine pass (N * Sf samples).  They cover the coarse pass
        # too: the ring slots of a pass never go down as its samples go up (csrc/field_f32.hip: sparse_ring_base)
        want = int(_fn("render_sparse_fused_workspace_bytes", arch)[0](N * Sf))
        extra = [_p(_workspace_buffer(ws, dev, "sparse", (want,), torch.uint8)), want]
    f, name = _fn("render_rays_rows_sparse" if extra else "render_rays_rows", arch)
    check(f(_p(packed), _p(frame), precision, N, _p(rays), int(rays.shape[1]), int(num_coarse), int(num_fine),
            int(bool(lindisp)), int(bool(white_background)), _p(bg), _p(t_rand), _p(noise_c), _p(u), _p(noise_f),
            _p(z_c), _p(z_f), _p(raw), _p(weights), _p(rows), int(rows.stride(0)), _p(xw), _p(src), _p(z_new), *extra, _stream()), name)
    return rows


def _spade_entry(dtype, backward=False):
    """The fp32 or the bf16 entry point of the fused modulation (include/sahs_nerf.h) -> (function, its name)."""
    name = "sahs_spade_modulate" + ("_backward" if backward else "") + ("_bf16" if dtype == torch.bfloat16 else "")
    return getattr(_lib.lib(), name), name


def _spade_modulate_forward(x, gamma, beta, eps, slope):
    """x, gamma, beta of ONE dtype, float32 or bfloat16 (spade_modulate sees to it)
    -> (x, gamma as the kernel read them (contiguous), out, the statistics workspace the launch left)."""
    dtype = x.dtype if isinstance(x, torch.Tensor) and x.dtype == torch.bfloat16 else torch.float32
    x, gamma, beta = _req(x, "x", dtype), _req(gamma, "gamma", dtype), _req(beta, "beta", dtype)
    if x.dim() != 4 or gamma.shape != x.shape or beta.shape != x.shape:
        raise _lib.SahsError("spade_modulate: x, gamma, beta must be NCHW tensors of one shape, got %s %s %s" % (tuple(x.shape), tuple(gamma.shape), tuple(beta.shape)))
    planes, hw = x.shape[0] * x.shape[1], x.shape[2] * x.shape[3]
    out = torch.empty_like(x)
    stats = torch.empty(int(_lib.lib().sahs_spade_modulate_workspace_words(planes)), dtype=torch.float32, device=x.device)
    f, name = _spade_entry(dtype)
    check(f(planes, hw, _p(x), _p(gamma), _p(beta), float(eps), float(slope), _p(out), _p(stats), _stream()), name)
    return x, gamma, out, stats


def spade_modulate(x, gamma, beta, eps=1e-5, slope=1.0):
    """lrelu_slope(InstanceNorm2d(x) * (1 + gamma) + beta) for NCHW tensors of one shape, fused (include/sahs_nerf.h: sahs_spade_modulate).
    Differentiable (SpadeModulateFn: sahs_spade_modulate_backward) when grad mode is on and one of the three tensors requires a gradient;
    with plain tensors it is the two launches of the forward alone, whatever the grad mode.
    dtype: three float32 tensors take the fp32 kernels; three bfloat16 tensors (what the convolutions hand over under
    torch.autocast) take the bf16 kernels -- fp32 arithmetic, bf16 output and gradients (sahs_spade_modulate_bf16); a mixture of the two
    is widened with .float() and takes the fp32 kernels, torch's own promotion rule.  Any other dtype is refused."""
    dtypes = [t.dtype for t in (x, gamma, beta) if isinstance(t, torch.Tensor)]
    if any(d not in (torch.float32, torch.bfloat16) for d in dtypes):
        raise _lib.SahsError("spade_modulate: x, gamma, beta must be torch.float32 or torch.bfloat16, got %s" % ", ".join(str(d) for d in dtypes))
    if len(set(dtypes)) > 1:
        x, gamma, beta = (t.float() if isinstance(t, torch.Tensor) else t for t in (x, gamma, beta))
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (x, gamma, beta)):
        return SpadeModulateFn.apply(x, gamma, beta, float(eps), float(slope))
    return _spade_modulate_forward(x, gamma, beta, eps, slope)[2]


def spade_modulate_frozen(x, gamma, beta, eps=1e-5, slope=1.0, up=False):
    """spade_modulate for inference with gamma / beta that do not depend on the frame (include/sahs_nerf.h: sahs_spade_modulate_frozen):
    x (B, C, h, w); gamma, beta (Bg, C, H, W) with Bg = 1 -- one map shared by the whole batch, read once per batch -- or Bg = B;
    up=False: (H, W) = (h, w); up=True: (H, W) = (2h, 2w) and the layer is applied to the nearest-neighbour 2x upsample of x, which is
    never formed (statistics from the source planes).  -> (B, C, H, W).  Same statistics and arithmetic as spade_modulate, bit for bit.
    There is NO backward: tensors that require a gradient are refused while grad mode is on (call it under torch.no_grad()).  dtype rule
    of spade_modulate: three float32 or three bfloat16 tensors; a mixture is widened to float32; anything else is refused."""
    dtypes = [t.dtype for t in (x, gamma, beta) if isinstance(t, torch.Tensor)]
    if any(d not in (torch.float32, torch.bfloat16) for d in dtypes):
        raise _lib.SahsError("spade_modulate_frozen: x, gamma, beta must be torch.float32 or torch.bfloat16, got %s" % ", ".join(str(d) for d in dtypes))
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (x, gamma, beta)):
        raise _lib.SahsError("spade_modulate_frozen has no backward (inference only): a tensor requires a gradient while grad mode is on; "
                             "call it under torch.no_grad(), or train through spade_modulate")
    if len(set(dtypes)) > 1:
        x, gamma, beta = (t.float() if isinstance(t, torch.Tensor) else t for t in (x, gamma, beta))
    dtype = x.dtype if isinstance(x, torch.Tensor) and x.dtype == torch.bfloat16 else torch.float32
    x, gamma, beta = _req(x, "x", dtype), _req(gamma, "gamma", dtype), _req(beta, "beta", dtype)
    shapes = "x %s, gamma %s, beta %s, up=%s" % (tuple(x.shape), tuple(gamma.shape), tuple(beta.shape), bool(up))
    if x.dim() != 4 or gamma.dim() != 4 or beta.shape != gamma.shape:
        raise _lib.SahsError("spade_modulate_frozen: x must be (B, C, h, w) and gamma, beta (1 or B, C, H, W) of one shape, got " + shapes)
    B, C, h, w = x.shape
    scale = 2 if up else 1
    if tuple(gamma.shape[1:]) != (C, scale * h, scale * w) or gamma.shape[0] not in (1, B):
        raise _lib.SahsError("spade_modulate_frozen: gamma, beta must be (1 or %d, %d, %d, %d) for this x, got %s"
                             % (B, C, scale * h, scale * w, shapes))
    out = torch.empty((B, C, scale * h, scale * w), dtype=dtype, device=x.device)
    stats = torch.empty(int(_lib.lib().sahs_spade_modulate_frozen_workspace_words(B, C)), dtype=torch.float32, device=x.device)
    name = "sahs_spade_modulate_frozen" + ("_bf16" if dtype == torch.bfloat16 else "")
    check(getattr(_lib.lib(), name)(B, C, h, w, int(gamma.shape[0]), int(bool(up)), _p(x), _p(gamma), _p(beta), float(eps), float(slope),
                                    _p(out), _p(stats), _stream()), name)
    return out


SPECTRAL_NORM_MAX_JOBS = 32      # include/sahs_nerf.h: SAHS_SPECTRAL_NORM_MAX_JOBS


def _flat_views(shapes, dtype, device):
    """One allocation cut into contiguous tensors of ``shapes``, each starting on a 32-byte boundary -> the list of views."""
    sizes = [torch.Size(s).numel() for s in shapes]
    starts, total = [], 0
    for n in sizes:
        starts.append(total)
        total += (n + 7) // 8 * 8
    flat = torch.empty(total, dtype=dtype, device=device)
    return [flat[a:a + n].view(s) for a, n, s in zip(starts, sizes, shapes)]


def _pointer_table(tensors):
    return (ctypes.c_void_p * len(tensors))(*(t.data_ptr() for t in tensors))


def _spectral_norm_dims(weights):
    return [(int(W.shape[0]), W.numel() // int(W.shape[0])) for W in weights]


def _spectral_normalize_forward(weights, us, vs, training, eps, out_dtype):
    """-> (the weights as the kernels read them, the outputs, each job's saved area: h + w + 1 floats u, v, sigma)."""
    Ws = []
    for k, (W, u, v) in enumerate(zip(weights, us, vs)):
        W = _req(W, "spectral_normalize: weights[%d]" % k)
        if W.dim() < 1 or W.numel() == 0:
            raise _lib.SahsError("spectral_normalize: weights[%d] of shape %s has no rows or no columns" % (k, tuple(W.shape)))
        h, w = _spectral_norm_dims([W])[0]
        for name, t, n in (("us", u, h), ("vs", v, w)):
            _req(t, "spectral_normalize: %s[%d]" % (name, k))
            if tuple(t.shape) != (n,) or not t.is_contiguous():
                raise _lib.SahsError("spectral_normalize: %s[%d] must be a contiguous vector of %d floats (it is updated in place), got shape %s"
                                     % (name, k, n, tuple(t.shape)))
        Ws.append(W)
    dims = _spectral_norm_dims(Ws)
    outs = _flat_views([W.shape for W in Ws], out_dtype, Ws[0].device)
    saved = _flat_views([(h + w + 1,) for h, w in dims], torch.float32, Ws[0].device)
    f = _lib.lib().sahs_spectral_norm_forward
    for a in range(0, len(Ws), SPECTRAL_NORM_MAX_JOBS):
        cut = slice(a, a + SPECTRAL_NORM_MAX_JOBS)
        hs, ws = zip(*dims[cut])
        n = len(hs)
        check(f(n, _pointer_table(Ws[cut]), _pointer_table(us[cut]), _pointer_table(vs[cut]), _pointer_table(outs[cut]),
                _pointer_table(saved[cut]), (ctypes.c_int * n)(*hs), (ctypes.c_int * n)(*ws), int(out_dtype == torch.bfloat16),
                int(bool(training)), float(eps), _stream()), "sahs_spectral_norm_forward")
    return Ws, outs, saved


def spectral_normalize(weights, us, vs, training, eps=1e-12):
    """torch.nn.utils.spectral_norm's weight computation (dim 0, one power iteration) for a LIST of weights in two launches per 32 of them
    (include/sahs_nerf.h: sahs_spectral_norm_forward): -> the list of W / sigma, each in its weight's shape.  ``us`` / ``vs``: each
    weight's u (out channels) and v (the rest) vectors; training: they take one power iteration IN PLACE, as the module's buffers do;
    otherwise they are only read.  Differentiable (SpectralNormalizeFn: one node, one backward launch per 32 weights) when grad mode
    is on and a weight requires a gradient; otherwise the forward launches alone.
    dtype: weights, us, vs float32, anything else is refused; sigma is formed in fp32 whatever autocast says, and the outputs are
    bfloat16 -- the fp32 quotient rounded once, what autocast's cast of torch's result gives -- exactly when CUDA autocast is on with
    dtype bfloat16, float32 otherwise.  The op itself runs outside autocast."""
    weights, us, vs = list(weights), list(us), list(vs)
    if not len(weights) == len(us) == len(vs):
        raise _lib.SahsError("spectral_normalize: %d weights, %d us, %d vs: the lists must be of one length" % (len(weights), len(us), len(vs)))
    if not weights:
        return []
    bf16 = torch.is_autocast_enabled("cuda") and torch.get_autocast_dtype("cuda") == torch.bfloat16
    out_dtype = torch.bfloat16 if bf16 else torch.float32
    with torch.autocast("cuda", enabled=False):
        if torch.is_grad_enabled() and any(isinstance(W, torch.Tensor) and W.requires_grad for W in weights):
            return list(SpectralNormalizeFn.apply(us, vs, bool(training), float(eps), out_dtype, *weights))
        return _spectral_normalize_forward(weights, us, vs, training, eps, out_dtype)[1]


IMAGE_METRICS_TILE = 32      # include/sahs_nerf.h: SAHS_IMAGE_METRICS_TILE
_IMAGE_DTYPES = {torch.uint8: 0, torch.float32: 1}      # SAHS_IMAGE_U8, SAHS_IMAGE_F32


def image_metrics(a, b, data_range=1.0, ssim_data_range=None, channels_last=True):
    """L1, MSE and windowed SSIM of two images or image batches in two launches (include/sahs_nerf.h: sahs_image_metrics).
    a, b: GPU tensors of ONE shape, (H, W, C) or (B, H, W, C) -- with channels_last=False (C, H, W) or (B, C, H, W) -- C = 1 .. 4,
    H, W >= 7, both torch.uint8 (scored as x / 255) or both torch.float32; any other dtype and a mixed pair are refused.  They are read
    in place through their strides: transposed or cropped views cost no copy.
    -> a float64 tensor on the device, (3 + C,) or (B, 3 + C): [mean SSIM, MSE, L1, SSIM of each channel].  SSIM is
    skimage.metrics.structural_similarity with its defaults and multichannel=True (7x7 uniform window, sample covariance, mean over the
    windows inside the image) at the data range ``ssim_data_range``, which defaults to ``data_range`` (metrics.py on why the two
    are separate arguments; PSNR, which is where ``data_range`` itself enters, is formed there).  Bit-reproducible; a batch gives the
    bits of its single calls.  No gradient."""
    for t, name in ((a, "a"), (b, "b")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.SahsError("image_metrics: %s must be a GPU tensor (the HIP path has no CPU fallback)" % name)
        if t.device.index != torch.cuda.current_device():
            raise _lib.SahsError("image_metrics: %s lives on %s but the current device is cuda:%d" % (name, t.device, torch.cuda.current_device()))
    if a.dtype != b.dtype or a.dtype not in _IMAGE_DTYPES:
        raise _lib.SahsError("image_metrics: a and b must both be torch.uint8 or both torch.float32, got %s and %s" % (a.dtype, b.dtype))
    if a.shape != b.shape or a.dim() not in (3, 4):
        raise _lib.SahsError("image_metrics: a and b must have one shape, (H, W, C) or (B, H, W, C) (channels_last=False: (C, H, W) or "
                             "(B, C, H, W)), got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    ssim_data_range = data_range if ssim_data_range is None else ssim_data_range
    if not (float(data_range) > 0.0 and float(ssim_data_range) > 0.0):
        raise _lib.SahsError("image_metrics: data_range = %r and ssim_data_range = %r must be > 0" % (data_range, ssim_data_range))
    batched = a.dim() == 4
    a, b = (a.detach(), b.detach()) if batched else (a.detach()[None], b.detach()[None])
    if not channels_last:
        a, b = a.permute(0, 2, 3, 1), b.permute(0, 2, 3, 1)      # views: the kernel reads through the strides
    B, H, W, C = a.shape
    L = _lib.lib()
    out = torch.empty(B, 3 + C, dtype=torch.float64, device=a.device)
    need = int(L.sahs_image_metrics_workspace_bytes(B, H, W, C))
    work = torch.empty(max(need, 8) // 8, dtype=torch.float64, device=a.device)
    strides = [(ctypes.c_long * 4)(*t.stride()) for t in (a, b)]
    check(L.sahs_image_metrics(_p(a), _p(b), _IMAGE_DTYPES[a.dtype], B, H, W, C, strides[0], strides[1], float(ssim_data_range), _p(out),
                               _p(work), need, _stream()), "sahs_image_metrics")
    return out if batched else out[0]


IMAGE_LOSS_TILE = 32      # include/sahs_nerf.h: SAHS_IMAGE_LOSS_TILE


def _image_loss_forward(pred, target, weights, clamp, ssim_data_range, grad):
    """pred, target, grad (or None): (B, H, W, C) views -> the float64 ``out`` of sahs_image_loss, 4 + 3 B values."""
    B, H, W, C = pred.shape
    L = _lib.lib()
    out = torch.empty(4 + 3 * B, dtype=torch.float64, device=pred.device)
    need = int(L.sahs_image_loss_workspace_bytes(B, H, W, C))
    work = torch.empty(max(need, 8) // 8, dtype=torch.float64, device=pred.device)
    strides = [None if t is None else (ctypes.c_long * 4)(*t.stride()) for t in (pred, target, grad)]
    check(L.sahs_image_loss(_p(pred), _p(target), B, H, W, C, strides[0], strides[1], weights[0], weights[1], weights[2], int(bool(clamp)),
                            float(ssim_data_range), _p(grad), strides[2], _p(out), _p(work), need, _stream()), "sahs_image_loss")
    return out


class ImageLossFn(torch.autograd.Function):
    """image_loss as ONE differentiable node: the forward's two launches also write the gradient image of each image's own loss, and the
    backward is one scaling of it by grad_out / B.  pred, target: (B, H, W, C) views.  -> (loss, rows); rows carries no gradient.
    Not twice differentiable."""

    @staticmethod
    def forward(ctx, pred, target, weights, clamp, ssim_data_range):
        grad = torch.empty_like(pred)      # (pred's strides where they are dense, so the permuted view of an NCHW tensor is written NCHW)
        out = _image_loss_forward(pred.detach(), target, weights, clamp, ssim_data_range, grad)
        _save_named(ctx, grad=grad)
        ctx.batch = pred.shape[0]
        rows = out[4:].view(-1, 3)
        ctx.mark_non_differentiable(rows)
        return out[0].float(), rows

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss, _grad_rows):
        return _load_named(ctx).grad * (grad_loss * (1.0 / ctx.batch)), None, None, None, None


def image_loss(pred, target, l2=1.0, l1=0.0, ssim=0.0, clamp=True, ssim_data_range=1.0, channels_last=False, return_terms=False):
    """The refiner's objective, fused and differentiable (include/sahs_nerf.h: sahs_image_loss; two launches whatever the batch):
        loss = l2 * MSE(x, t) + l1 * L1(x, t) + ssim * (1 - SSIM(x, t)),   x = pred.clamp(0, 1) if clamp else pred,
    MSE and L1 the means over all elements, SSIM image_metrics' (7x7 uniform window, sample covariance, at ``ssim_data_range``), averaged
    over the batch.  pred, target: float32 GPU tensors of ONE shape, (C, H, W) or (B, C, H, W) -- with channels_last=True (H, W, C) or
    (B, H, W, C) -- C = 1 .. 4, H, W >= 7, read in place through their strides.
    -> the loss, a 0-d float32 tensor; with return_terms=True (loss, rows), rows the detached float64 (B, 3) [MSE, L1, mean SSIM] of
    each image.  The gradient flows to ``pred`` only (ImageLossFn: the forward forms it, the backward scales it; it has pred's shape),
    through the clamp where 0 <= pred <= 1; ``target`` must not require one.  When pred asks for no gradient, or under no_grad, the
    kernel skips the gradient's work and returns the same bits.  Bit-reproducible; a batch gives the bits of its single calls.
    Runs outside autocast."""
    for t, name in ((pred, "pred"), (target, "target")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.SahsError("image_loss: %s must be a GPU tensor (the HIP path has no CPU fallback)" % name)
        if t.device.index != torch.cuda.current_device():
            raise _lib.SahsError("image_loss: %s lives on %s but the current device is cuda:%d" % (name, t.device, torch.cuda.current_device()))
        if t.dtype != torch.float32:
            raise _lib.SahsError("image_loss: %s must be torch.float32, got %s (under autocast: pred.float())" % (name, t.dtype))
    if target.requires_grad:
        raise _lib.SahsError("image_loss: target requires a gradient, and the gradient is formed for pred only (pass target.detach())")
    if pred.shape != target.shape or pred.dim() not in (3, 4):
        raise _lib.SahsError("image_loss: pred and target must have one shape, (C, H, W) or (B, C, H, W) (channels_last=True: (H, W, C) or "
                             "(B, H, W, C)), got %s and %s" % (tuple(pred.shape), tuple(target.shape)))
    if pred.dim() == 3:
        pred, target = pred[None], target[None]
    if not channels_last:
        pred, target = pred.permute(0, 2, 3, 1), target.permute(0, 2, 3, 1)      # views: the kernel reads through the strides
    B, H, W, C = pred.shape
    if H < 7 or W < 7:
        raise _lib.SahsError("image_loss: pred is %d x %d pixels, the 7 x 7 SSIM window needs H, W >= 7" % (H, W))
    if not 1 <= C <= 4:
        raise _lib.SahsError("image_loss: pred has C = %d channels, must be 1 .. 4 (channels_last=%r)" % (C, bool(channels_last)))
    weights = (float(l2), float(l1), float(ssim))
    with torch.autocast("cuda", enabled=False):
        if torch.is_grad_enabled() and pred.requires_grad:
            loss, rows = ImageLossFn.apply(pred, target, weights, bool(clamp), float(ssim_data_range))
        else:
            out = _image_loss_forward(pred.detach(), target, weights, clamp, ssim_data_range, None)
            loss, rows = out[0].float(), out[4:].view(-1, 3)
    return (loss, rows) if return_terms else loss


FRAME_PRODUCTS_TILE = 32      # include/sahs_nerf.h: SAHS_FRAME_PRODUCTS_TILE


def frame_products(rgb, disp=None, w_bg=None, focal=None, clean=True, central_difference=False, float_normals=False):
    """What Stage-I evaluation writes for a rendered frame, as bytes, in at most two launches whatever the batch (include/sahs_nerf.h:
    sahs_frame_products; evaluation.py's cast_to_image, label2color, normal_map and cast_to_disparity_image are its statement).
    rgb: float32 GPU tensor (H, W, C) or (B, H, W, C), C = 3 or 15 ([rgb3 | seg12], the renderer's output), read in place through
    its batch, row and column strides (channel stride 1: a [..., :3] view of the render is read in place; anything else is copied).
    disp, w_bg: float32 (H, W) or (B, H, W), optional.  focal: the intrinsics [fx, fy, cx, cy] (cx, cy as fractions), optional.
    -> dict of GPU tensors, a key present exactly when its inputs were given:
      image      uint8 (.., H, W, 3)                    always
      seg        uint8 (.., H, W, 3)                    C = 15
      disparity  uint8 (.., H, W)                       disp
      normals    uint8 (.., H - d, W - d, 3)            disp and focal (w_bg and clean: whitened and blended); d = 2 with central_difference, else 1
      normals_f32  float32, the same before the clamp   disp and focal, and float_normals (asking for it without them is refused)
    A NaN that reaches a byte is stored as 0; a frame whose disparity holds a NaN, or is constant, gets an all-zero disparity plane.
    Rectangular maps: the column index enters x with cx * W, the row index y with cy * H.  No gradient."""
    for t, name in ((rgb, "rgb"), (disp, "disp"), (w_bg, "w_bg")):
        if t is None and name != "rgb":
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.SahsError("frame_products: %s must be a GPU tensor (the HIP path has no CPU fallback)" % name)
        if t.device.index != torch.cuda.current_device():
            raise _lib.SahsError("frame_products: %s lives on %s but the current device is cuda:%d" % (name, t.device, torch.cuda.current_device()))
        if t.dtype != torch.float32:
            raise _lib.SahsError("frame_products: %s must be torch.float32, got %s" % (name, t.dtype))
    if rgb.dim() not in (3, 4):
        raise _lib.SahsError("frame_products: rgb must be (H, W, C) or (B, H, W, C), got %s" % (tuple(rgb.shape),))
    batched = rgb.dim() == 4
    rgb = rgb.detach() if batched else rgb.detach()[None]
    B, H, W, C = rgb.shape
    if rgb.stride(3) != 1 and C > 1:
        rgb = rgb.contiguous()
    planes = []
    for t, name in ((disp, "disp"), (w_bg, "w_bg")):
        if t is not None:
            if tuple(t.shape) != ((B, H, W) if batched else (H, W)):
                raise _lib.SahsError("frame_products: %s is %s, rgb is %s: needs rgb's frames and pixels" % (name, tuple(t.shape), tuple(rgb.shape)))
            t = t.detach().contiguous()
        planes.append(t)
    disp, w_bg = planes
    intr = None if focal is None else (ctypes.c_float * 4)(*[float(v) for v in focal])
    d = 2 if central_difference else 1
    dev = rgb.device
    lead = (B,) if batched else ()
    u8 = lambda *shape: torch.empty(lead + shape, dtype=torch.uint8, device=dev)      # noqa: E731
    out = {"image": u8(H, W, 3)}
    if C == 15:
        out["seg"] = u8(H, W, 3)
    if disp is not None:
        out["disparity"] = u8(H, W)
        if focal is not None:
            out["normals"] = u8(max(H - d, 0), max(W - d, 0), 3)
    if float_normals:      # asked for: without disp and focal the C side refuses, with its message
        out["normals_f32"] = torch.empty(lead + (max(H - d, 0), max(W - d, 0), 3), dtype=torch.float32, device=dev)
    L = _lib.lib()
    need = int(L.sahs_frame_products_workspace_bytes(B, H, W)) if disp is not None else 0
    work = torch.empty(max(need, 16) // 4, dtype=torch.float32, device=dev)
    strides = (ctypes.c_long * 3)(*rgb.stride()[:3])
    check(L.sahs_frame_products(_p(rgb), C, strides, _p(disp), _p(w_bg), intr, B, H, W, int(bool(clean)), int(bool(central_difference)),
                                _p(out["image"]), _p(out.get("seg")), _p(out.get("normals")), _p(out.get("normals_f32")),
                                _p(out.get("disparity")), _p(work), need, _stream()), "sahs_frame_products")
    return out


LPIPS_TILE, LPIPS_MAX_JOBS, LPIPS_MAX_CHANNELS, LPIPS_MIN_SIDE = 256, 5, 1024, 31      # include/sahs_nerf.h: SAHS_LPIPS_*


def lpips_prepare(a, b, normalize=False, channels_last=True):
    """LPIPS's input stage in one launch (include/sahs_nerf.h: sahs_lpips_prepare).  a, b: GPU tensors of ONE shape, (H, W, 3) or
    (B, H, W, 3) -- with channels_last=False (3, H, W) or (B, 3, H, W) -- H, W >= 31, both torch.uint8 (taken as x / 255) or both
    torch.float32, read in place through their strides.  -> ONE contiguous (2B, 3, H, W) float32 tensor, rows [0, B) from a and
    [B, 2B) from b, after the scaling layer (x - shift) / scale; normalize=True maps x -> 2x - 1 first (metrics.py: LPIPS on which
    is whose convention).  No gradient."""
    for t, name in ((a, "a"), (b, "b")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.SahsError("lpips_prepare: %s must be a GPU tensor (the HIP path has no CPU fallback)" % name)
        if t.device.index != torch.cuda.current_device():
            raise _lib.SahsError("lpips_prepare: %s lives on %s but the current device is cuda:%d" % (name, t.device, torch.cuda.current_device()))
    if a.dtype != b.dtype or a.dtype not in _IMAGE_DTYPES:
        raise _lib.SahsError("lpips_prepare: a and b must both be torch.uint8 or both torch.float32, got %s and %s" % (a.dtype, b.dtype))
    if a.shape != b.shape or a.dim() not in (3, 4):
        raise _lib.SahsError("lpips_prepare: a and b must have one shape, (H, W, 3) or (B, H, W, 3) (channels_last=False: (3, H, W) or "
                             "(B, 3, H, W)), got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    a, b = (a.detach(), b.detach()) if a.dim() == 4 else (a.detach()[None], b.detach()[None])
    if not channels_last:
        a, b = a.permute(0, 2, 3, 1), b.permute(0, 2, 3, 1)      # views: the kernel reads through the strides
    B, H, W, C = a.shape
    out = torch.empty(2 * B, 3, H, W, dtype=torch.float32, device=a.device)
    strides = [(ctypes.c_long * 4)(*t.stride()) for t in (a, b)]
    check(_lib.lib().sahs_lpips_prepare(_p(a), _p(b), _IMAGE_DTYPES[a.dtype], B, H, W, C, strides[0], strides[1], int(bool(normalize)),
                                        _p(out), _stream()), "sahs_lpips_prepare")
    return out


def lpips_distance(features, lin_weights):
    """LPIPS's head over up to five layers in two launches (include/sahs_nerf.h: sahs_lpips_distance).  features: a list of
    contiguous (2B, C_l, h_l, w_l) float32 GPU tensors whose rows [0, B) belong to one image batch and [B, 2B) to the other;
    lin_weights: per layer its C_l channel weights (float32, any shape with C_l elements, e.g. (1, C_l, 1, 1)).
    -> (B, 6) float64: [LPIPS, d_0 .. d_4] (d of layers not given: 0).  Bit-reproducible; a batch gives the bits of its single calls.
    A tensor that is not contiguous float32 is refused, not copied.  No gradient."""
    features, lin_weights = list(features), list(lin_weights)
    if len(features) != len(lin_weights) or not 1 <= len(features) <= LPIPS_MAX_JOBS:
        raise _lib.SahsError("lpips_distance: %d feature tensors and %d weight tensors: needs one weight tensor per layer and 1 .. %d layers"
                             % (len(features), len(lin_weights), LPIPS_MAX_JOBS))
    for l, (f, w) in enumerate(zip(features, lin_weights)):
        for t, name in ((f, "features[%d]" % l), (w, "lin_weights[%d]" % l)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise _lib.SahsError("lpips_distance: %s must be a GPU tensor (the HIP path has no CPU fallback)" % name)
            if t.device.index != torch.cuda.current_device():
                raise _lib.SahsError("lpips_distance: %s lives on %s but the current device is cuda:%d" % (name, t.device, torch.cuda.current_device()))
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise _lib.SahsError("lpips_distance: %s must be contiguous float32 (features: NCHW), got %s with strides %s"
                                     % (name, t.dtype, tuple(t.stride())))
        if f.dim() != 4 or f.shape[0] != features[0].shape[0] or f.shape[0] % 2 or w.numel() != f.shape[1]:
            raise _lib.SahsError("lpips_distance: features[%d] is %s with %d weights: needs (2B, C, h, w) with the 2B of features[0] and C weights"
                                 % (l, tuple(f.shape), w.numel()))
    n, B = len(features), features[0].shape[0] // 2
    L = _lib.lib()
    fp, wp = (ctypes.c_void_p * n)(*[f.data_ptr() for f in features]), (ctypes.c_void_p * n)(*[w.data_ptr() for w in lin_weights])
    Cs, hw = (ctypes.c_int * n)(*[f.shape[1] for f in features]), (ctypes.c_long * n)(*[f.shape[2] * f.shape[3] for f in features])
    out = torch.empty(B, 1 + LPIPS_MAX_JOBS, dtype=torch.float64, device=features[0].device)
    need = int(L.sahs_lpips_distance_workspace_bytes(n, B, hw))
    work = torch.empty(max(need, 8) // 8, dtype=torch.float64, device=out.device)
    check(L.sahs_lpips_distance(n, fp, wp, Cs, hw, B, _p(out), _p(work), need, _stream()), "sahs_lpips_distance")
    return out


def _lpips_prepare_loss_forward(pred, target, clamp, normalize):
    """pred, target: (B, H, W, 3) views -> the one (2B, 3, H, W) buffer of sahs_lpips_prepare_loss."""
    B, H, W, C = pred.shape
    out = torch.empty(2 * B, 3, H, W, dtype=torch.float32, device=pred.device)
    strides = [(ctypes.c_long * 4)(*t.stride()) for t in (pred, target)]
    check(_lib.lib().sahs_lpips_prepare_loss(_p(pred), _p(target), _IMAGE_DTYPES[target.dtype], B, H, W, C, strides[0], strides[1],
                                             int(bool(normalize)), int(bool(clamp)), _p(out), _stream()), "sahs_lpips_prepare_loss")
    return out


class LpipsPrepareLossFn(torch.autograd.Function):
    """lpips_prepare_loss as ONE differentiable node: one launch forward, one launch backward (sahs_lpips_prepare_grad: the clamp's mask is
    read from the saved pred).  pred, target: (B, H, W, 3) views.  -> (x_pred, x_target); x_target carries no gradient.  Not twice
    differentiable."""

    @staticmethod
    def forward(ctx, pred, target, clamp, normalize):
        out = _lpips_prepare_loss_forward(pred.detach(), target, clamp, normalize)
        _save_named(ctx, pred=pred.detach())
        ctx.clamp, ctx.normalize = bool(clamp), bool(normalize)
        B = pred.shape[0]
        x_pred, x_target = out[:B], out[B:]
        ctx.mark_non_differentiable(x_target)
        return x_pred, x_target

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gx, _g_target):
        pred = _load_named(ctx).pred
        B, H, W, C = pred.shape
        gx = gx.contiguous().float()
        grad = torch.empty_like(pred)      # (pred's strides where they are dense, so the permuted view of an NCHW tensor is written NCHW)
        strides = [(ctypes.c_long * 4)(*t.stride()) for t in (pred, grad)]
        check(_lib.lib().sahs_lpips_prepare_grad(_p(pred), _p(gx), B, H, W, C, strides[0], int(ctx.normalize), int(ctx.clamp), _p(grad),
                                                 strides[1], _stream()), "sahs_lpips_prepare_grad")
        return grad, None, None, None


def lpips_prepare_loss(pred, target, clamp=True, normalize=False, channels_last=False):
    """LPIPS's input stage for a training term, one launch each way (include/sahs_nerf.h: sahs_lpips_prepare_loss,
    sahs_lpips_prepare_grad).  pred: float32 GPU tensor (3, H, W) or (B, 3, H, W) -- with channels_last=True (H, W, 3) or (B, H, W, 3) --
    H, W >= 31; target: the same shape, torch.uint8 (taken as x / 255) or torch.float32.  Both are read in place through their strides.
    clamp=True applies clamp(0, 1) to pred alone, then as lpips_prepare: the optional 2x - 1 and (x - shift) / scale.
    -> (x_pred, x_target), two contiguous (B, 3, H, W) float32 views of ONE buffer, so that torch.cat is never needed.  The gradient
    flows to ``pred`` only (it has pred's shape, and pred's layout where that is dense), through the clamp where 0 <= pred <= 1;
    ``target`` must not require one.  Runs outside autocast."""
    for t, name in ((pred, "pred"), (target, "target")):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.SahsError("lpips_prepare_loss: %s must be a GPU tensor (the HIP path has no CPU fallback)" % name)
        if t.device.index != torch.cuda.current_device():
            raise _lib.SahsError("lpips_prepare_loss: %s lives on %s but the current device is cuda:%d" % (name, t.device, torch.cuda.current_device()))
    if pred.dtype != torch.float32 or target.dtype not in _IMAGE_DTYPES:
        raise _lib.SahsError("lpips_prepare_loss: pred must be torch.float32 and target torch.uint8 or torch.float32, got %s and %s "
                             "(under autocast: pred.float())" % (pred.dtype, target.dtype))
    if target.requires_grad:
        raise _lib.SahsError("lpips_prepare_loss: target requires a gradient, and the gradient is formed for pred only (pass target.detach())")
    if pred.shape != target.shape or pred.dim() not in (3, 4):
        raise _lib.SahsError("lpips_prepare_loss: pred and target must have one shape, (3, H, W) or (B, 3, H, W) (channels_last=True: "
                             "(H, W, 3) or (B, H, W, 3)), got %s and %s" % (tuple(pred.shape), tuple(target.shape)))
    if pred.dim() == 3:
        pred, target = pred[None], target[None]
    if not channels_last:
        pred, target = pred.permute(0, 2, 3, 1), target.permute(0, 2, 3, 1)      # views: the kernel reads through the strides
    B = pred.shape[0]
    with torch.autocast("cuda", enabled=False):
        if torch.is_grad_enabled() and pred.requires_grad:
            return LpipsPrepareLossFn.apply(pred, target, bool(clamp), bool(normalize))
        out = _lpips_prepare_loss_forward(pred.detach(), target, clamp, normalize)
        return out[:B], out[B:]


def _lpips_head_tables(fa, fb, lin_weights):
    n = len(fa)
    ptrs = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])      # noqa: E731
    return (n, ptrs(fa), ptrs(fb), ptrs(lin_weights), (ctypes.c_int * n)(*[f.shape[1] for f in fa]),
            (ctypes.c_long * n)(*[f.shape[2] * f.shape[3] for f in fa]), fa[0].shape[0])


def _lpips_head_forward(fa, fb, lin_weights, want_stats):
    """-> (rows (B, 6) float64, stats or None): sahs_lpips_head_forward."""
    n, pa, pb, pw, Cs, hw, B = _lpips_head_tables(fa, fb, lin_weights)
    L = _lib.lib()
    dev = fa[0].device
    out = torch.empty(B, 1 + LPIPS_MAX_JOBS, dtype=torch.float64, device=dev)
    need = int(L.sahs_lpips_distance_workspace_bytes(n, B, hw))
    work = torch.empty(max(need, 8) // 8, dtype=torch.float64, device=dev)
    need_stats = int(L.sahs_lpips_head_stats_bytes(n, B, hw)) if want_stats else 0
    stats = torch.empty(max(need_stats, 8) // 8, dtype=torch.float64, device=dev) if want_stats else None
    check(L.sahs_lpips_head_forward(n, pa, pb, pw, Cs, hw, B, _p(out), _p(stats), need_stats, _p(work), need, _stream()), "sahs_lpips_head_forward")
    return out, stats


class LpipsHeadFn(torch.autograd.Function):
    """lpips_head as ONE differentiable node: the forward's two launches also store three doubles per pixel (1 / na, 1 / nb, q), and the
    backward is one launch over all layers (include/sahs_nerf.h: sahs_lpips_head_backward).  apply(fb, lin_weights, *fa) ->
    (per_image, rows); rows carries no gradient.  Saved: the features themselves, the weights and the statistics -- no normalised copies.
    Not twice differentiable."""

    @staticmethod
    def forward(ctx, fb, lin_weights, *fa):
        fa = [f.detach() for f in fa]
        rows, stats = _lpips_head_forward(fa, fb, lin_weights, True)
        ctx.layers = len(fa)
        _save_named(ctx, stats=stats, **{"fa%d" % l: f for l, f in enumerate(fa)}, **{"fb%d" % l: f for l, f in enumerate(fb)},
                    **{"w%d" % l: w for l, w in enumerate(lin_weights)})
        ctx.mark_non_differentiable(rows)
        return rows[:, 0].float(), rows

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, _g_rows):
        s = _load_named(ctx)
        fa, fb, ws = ([getattr(s, "%s%d" % (k, l)) for l in range(ctx.layers)] for k in ("fa", "fb", "w"))
        n, pa, pb, pw, Cs, hw, B = _lpips_head_tables(fa, fb, ws)
        if g.dtype != torch.float64:
            g = g.float()
        g = g.contiguous()
        grads = [torch.empty_like(f) for f in fa]
        pg = (ctypes.c_void_p * n)(*[t.data_ptr() for t in grads])
        check(_lib.lib().sahs_lpips_head_backward(n, pa, pb, pw, Cs, hw, B, _p(g), int(g.dtype == torch.float64), _p(s.stats), s.stats.numel() * 8,
                                                  pg, _stream()), "sahs_lpips_head_backward")
        return (None, None) + tuple(gr if need else None for gr, need in zip(grads, ctx.needs_input_grad[2:]))


def lpips_head(fa, fb, lin_weights):
    """LPIPS's head as a training term (include/sahs_nerf.h: sahs_lpips_head_forward, sahs_lpips_head_backward).  fa, fb: lists of
    contiguous float32 GPU tensors (B, C_l, h_l, w_l), one pair per layer (1 .. 5), the features of pred and of target; lin_weights:
    per layer its C_l channel weights, as lpips_distance takes them.
    -> (per_image, rows): per_image (B,) float32, each image's LPIPS, differentiable with respect to ``fa`` ONLY (fb and the weights
    get no gradient, whatever they ask for); rows the detached float64 (B, 6) [LPIPS, d_0 .. d_4] of lpips_distance, the same bits.
    One autograd node, once differentiable: two launches forward, one backward.  A pixel whose features are all zero has a finite
    gradient (autograd of the published formula gives NaN there); equal operands give exactly 0 and a gradient that is exactly 0.
    Under no_grad, or when no fa[l] requires a gradient, the statistics are not stored and the result has the same bits.
    Bit-reproducible; a batch gives the bits of its single calls.  A tensor that is not contiguous float32 is refused, not copied."""
    fa, fb, lin_weights = list(fa), list(fb), list(lin_weights)
    if not (len(fa) == len(fb) == len(lin_weights)) or not 1 <= len(fa) <= LPIPS_MAX_JOBS:
        raise _lib.SahsError("lpips_head: %d fa, %d fb and %d weight tensors: needs one of each per layer and 1 .. %d layers"
                             % (len(fa), len(fb), len(lin_weights), LPIPS_MAX_JOBS))
    for l, (a, b, w) in enumerate(zip(fa, fb, lin_weights)):
        for t, name in ((a, "fa[%d]" % l), (b, "fb[%d]" % l), (w, "lin_weights[%d]" % l)):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise _lib.SahsError("lpips_head: %s must be a GPU tensor (the HIP path has no CPU fallback)" % name)
            if t.device.index != torch.cuda.current_device():
                raise _lib.SahsError("lpips_head: %s lives on %s but the current device is cuda:%d" % (name, t.device, torch.cuda.current_device()))
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise _lib.SahsError("lpips_head: %s must be contiguous float32 (features: NCHW), got %s with strides %s"
                                     % (name, t.dtype, tuple(t.stride())))
        if a.dim() != 4 or a.shape != b.shape or a.shape[0] != fa[0].shape[0] or w.numel() != a.shape[1]:
            raise _lib.SahsError("lpips_head: fa[%d] is %s, fb[%d] %s, with %d weights: needs two (B, C, h, w) of one shape with the B of fa[0] "
                                 "and C weights" % (l, tuple(a.shape), l, tuple(b.shape), w.numel()))
    fb, lin_weights = [t.detach() for t in fb], [t.detach() for t in lin_weights]
    with torch.autocast("cuda", enabled=False):
        if torch.is_grad_enabled() and any(f.requires_grad for f in fa):
            return LpipsHeadFn.apply(fb, lin_weights, *fa)
        rows, _ = _lpips_head_forward([f.detach() for f in fa], fb, lin_weights, False)
        return rows[:, 0].float(), rows


def adam_step(params, grad, exp_avg, exp_avg_sq, lr, beta1=0.9, beta2=0.999, eps=1e-8, step=1, grad_scale=1.0):
    """One torch.optim.Adam update (weight_decay 0, no amsgrad) of n contiguous fp32 values, in place on params / exp_avg / exp_avg_sq, as one
    HIP launch (include/sahs_nerf.h: sahs_adam_step).  step: the 1-based count of this update; grad is read as grad * grad_scale."""
    for t, name in ((params, "params"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        if _req(t, name) is not t:      # (updated in place: a contiguous copy would take the update with it)
            raise _lib.SahsError("adam_step: %s must be contiguous" % name)
        if t.numel() != params.numel():
            raise _lib.SahsError("adam_step: %s has %d values, params has %d" % (name, t.numel(), params.numel()))
    check(_lib.lib().sahs_adam_step(_p(params), _p(grad), _p(exp_avg), _p(exp_avg_sq), params.numel(), float(lr), float(beta1), float(beta2),
                                    float(eps), int(step), float(grad_scale), _stream()), "sahs_adam_step")
    return params


class LaunchProbe:
    """HIP events around every FIELD-kernel launch the library makes on this thread while the block is open (include/sahs_nerf.h:
    sahs_probe_*), recorded on the launch stream: per-kernel times of the product's own call chain (bench.py's roofline).
    ``records()`` -> list of dict(model, level, part (0 whole network | 1 deformation nets | 2 radiance nets), precision (of the kernel
    launched), samples, ms); it waits for the probed launches to finish."""

    def __init__(self, capacity=4096):
        self.capacity = int(capacity)

    def __enter__(self):
        check(_lib.lib().sahs_probe_arm(self.capacity), "sahs_probe_arm")
        return self

    def __exit__(self, *exc):
        _lib.lib().sahs_probe_disarm()
        return False

    @staticmethod
    def records():
        L = _lib.lib()
        if L.sahs_probe_dropped():
            raise _lib.SahsError("launch probe overflow: %d launches were not recorded" % L.sahs_probe_dropped())
        out = []
        kind, samples, ms = ctypes.c_int(), ctypes.c_long(), ctypes.c_float()
        for i in range(L.sahs_probe_count()):
            check(L.sahs_probe_read(i, ctypes.byref(kind), ctypes.byref(samples), ctypes.byref(ms)), "sahs_probe_read")
            k = kind.value
            out.append(dict(model=ARCHS[k >> 16], level=(k >> 12) & 15, part=(k >> 8) & 15, precision=k & 255, samples=samples.value, ms=ms.value))
        return out


# ---------------------------------------------------------------------------------------------------------
# training path
# ---------------------------------------------------------------------------------------------------------
def field_forward_save(packed, frame, level, rays, z, arch="audio", bits=None, precision=SAHS_F32):
    """fp32 field forward that also returns the saved activations for field_backward: ONE buffer of P * act_words floats laid out
    as a dense [P x width] plane per layer (plane c starts at float c * P; sahs_layout.hpp, namespace act) -- NOT one row per
    sample, so it can only be handed to field_backward whole, with the same P.  bits (alloc_sign_bits(P, FIELD_ALL, arch, device)):
    also filled with the sign-bit planes (sahs_model_field_forward_save_bits) -- hand both to field_backward_split(..., 3, bits=bits).
    precision SAHS_BF16X3 (the NeRFaceModel without deformation nets, bits required): the same buffers written by the split-operand
    kernel (sahs_model_field_forward_save_bits_x3); `packed` is then pack_weights(flat, SAHS_BF16X3, arch)."""
    packed, frame, rays, z = _req(packed, "packed"), _req(frame, "frame"), _req(rays, "rays"), _req(z, "z")
    N, S = z.shape
    x3 = int(precision) == SAHS_BF16X3
    if int(precision) not in (SAHS_F32, SAHS_BF16X3) or (x3 and bits is None):
        raise _lib.SahsError("field_forward_save: fp32, or SAHS_BF16X3 with the sign bits (bits=alloc_sign_bits(...))")
    raw = torch.empty(N, S, 16, dtype=torch.float32, device=z.device)
    act = torch.empty(N * S, _fn("act_words_per_sample", arch)[0](), dtype=torch.float32, device=z.device)
    if bits is not None:
        bits = _req(bits, "bits", torch.int32)
        if tuple(bits.shape) != (N * S, int(_fn("bits_words_part", arch)[0](FIELD_ALL))):
            raise _lib.SahsError("field_forward_save: bits must come from alloc_sign_bits(N * S, FIELD_ALL, arch, device)")
    f, name = _fn("field_forward_save" + ("" if bits is None else "_bits_x3" if x3 else "_bits"), arch)
    out = [_p(act)] if bits is None else [_p(act), _p(bits)]
    check(f(_p(packed), _p(frame), int(level), N, S, _p(rays), int(rays.shape[1]), _p(z), _p(raw), *out, _stream()), name)
    return raw, act


def field_backward(flat, frame, level, act, d_raw, grad_flat, grad_cond, arch="audio"):
    flat, frame, act, d_raw = _req(flat, "flat_params"), _req(frame, "frame"), _req(act, "act"), _req(d_raw, "d_raw")
    P = act.shape[0]
    ws = torch.empty(_fn("field_backward_workspace_words", arch)[0](P), dtype=torch.float32, device=act.device)
    f, name = _fn("field_backward", arch)
    check(f(_p(flat), _p(frame), int(level), P, _p(act), _p(d_raw), _p(grad_flat), _p(grad_cond), _p(ws), _stream()), name)


def alloc_sign_bits(num_samples, mode, arch, device):
    """Buffer for the sign-bit planes a saving forward of `mode` writes beside the activations (include/sahs_nerf.h:
    sahs_model_field_forward_split_save_bits) -- the derivative masks of the fused backward walk; None where the architecture's backward
    does not read them."""
    words = int(_fn("bits_words_part", arch)[0](int(mode)))
    return torch.empty(int(num_samples), words, dtype=torch.int32, device=device) if words > 0 else None


def _whole_save_part(act, bits, part, arch, P):
    """Base pointers (act, bits) of `part` (FIELD_DEFORM | FIELD_RADIANCE) inside a WHOLE-network save of P samples (bits may be None): a saved
    array of column c starts at float c * P in every save, so the deformation part starts where the save does and the radiance part behind the
    act columns in front of act::XW / behind sbits::BD_WORDS words per sample.  The kernels move 16 bytes per lane, so both byte offsets must be
    multiples of 16: in sahs_layout.hpp every act column is a multiple of 16 floats, sbits::words() of 4 words, so the guard never fires today."""
    if int(part) != FIELD_RADIANCE:
        return _p(act), _p(bits)
    words, bwords = _fn("act_words_part", arch)[0], _fn("bits_words_part", arch)[0]
    offs = 4 * (int(words(FIELD_ALL)) - int(words(FIELD_RADIANCE))) * P, 4 * int(bwords(FIELD_DEFORM)) * P
    if offs[0] % 16 or offs[1] % 16:
        raise _lib.SahsError("the radiance part of a whole-network save of N*S = %d samples starts at byte %d (activations) / %d (sign bits): "
                             "not multiples of 16" % (P, offs[0], offs[1]))
    return ctypes.c_void_p(act.data_ptr() + offs[0]), None if bits is None else ctypes.c_void_p(bits.data_ptr() + offs[1])


def field_forward_split_save(packed, frame, level, mode, rays, xw, z=None, src=None, xw_col0=0, arch="audio", bits=None, precision=SAHS_F32, whole=None):
    """field_forward_split (fp32) that also keeps the activations of the layers it runs -> (raw or None, act).  act is the part's
    own buffer, (P, act_words_part(mode)) floats as dense per-layer planes; only field_backward_split of the same part reads it.
    bits (from alloc_sign_bits, same mode): also filled -- hand it to field_backward_split with act.
    precision SAHS_BF16X3 (the models with deformation nets, modes FIELD_DEFORM / FIELD_RADIANCE, bits required): the same buffers written
    by the split-operand kernels; `packed` is then pack_weights(flat, SAHS_BF16X3, arch).
    whole=(act, bits) of a WHOLE-network save (FIELD_ALL shapes): the launch fills `mode`'s part of them instead of buffers of its own
    (a saved array of column c starts at c * P in every save), so a FIELD_DEFORM + FIELD_RADIANCE pair leaves what one FIELD_ALL launch
    leaves -> (raw or None, whole act)."""
    packed, frame, rays, z = _req(packed, "packed"), _req(frame, "frame"), _req(rays, "rays"), _req(z, "z")
    src, xw = _req(src, "src", torch.int32), _req(xw, "xw")
    N = rays.shape[0]
    S = src.shape[1] if mode == FIELD_RADIANCE else z.shape[1]
    if xw.dim() != 3 or xw.shape[0] != N or xw.shape[2] != 8:
        raise _lib.SahsError("xw must be (N, row, 8)")
    raw = None if mode == FIELD_DEFORM else torch.empty(N, S, 16, dtype=torch.float32, device=rays.device)
    words, bwords = _fn("act_words_part", arch)[0], _fn("bits_words_part", arch)[0]
    if whole is not None:
        act, bits = _req(whole[0], "whole act"), _req(whole[1], "whole bits", torch.int32)
        if int(mode) not in (FIELD_DEFORM, FIELD_RADIANCE) or tuple(act.shape) != (N * S, int(words(FIELD_ALL))) or tuple(bits.shape) != (N * S, int(bwords(FIELD_ALL))):
            raise _lib.SahsError("field_forward_split_save(whole): buffers of a FIELD_ALL save of the same samples, filled by a FIELD_DEFORM or FIELD_RADIANCE launch")
        act_ptr, bits_ptr = _whole_save_part(act, bits, mode, arch, N * S)
    else:
        act = torch.empty(N * S, words(int(mode)), dtype=torch.float32, device=rays.device)
        if bits is not None:
            bits = _req(bits, "bits", torch.int32)
            if tuple(bits.shape) != (N * S, int(bwords(int(mode)))):
                raise _lib.SahsError("field_forward_split_save: bits must come from alloc_sign_bits(N * S, mode, arch, device)")
        elif int(precision) != SAHS_F32:
            raise _lib.SahsError("field_forward_split_save: a saving forward at a precision other than fp32 needs the sign bits (bits=alloc_sign_bits(...))")
        act_ptr, bits_ptr = _p(act), _p(bits)
    f, name = _fn("field_forward_split_save" + ("" if bits is None else "_bits_x3" if int(precision) == SAHS_BF16X3 else "_bits"), arch)
    out = [act_ptr] if bits is None else [act_ptr, bits_ptr]
    check(f(_p(packed), _p(frame), int(level), int(mode), N, int(S), _p(rays), int(rays.shape[1]), _p(z), _p(raw), _p(xw), int(xw.shape[1]), int(xw_col0),
            _p(src), *out, _stream()), name)
    return raw, act


def fused_backward(enable=None):
    """The fused backward walk (one data-gradient chain launch + one or two weight-gradient launches per part: include/sahs_nerf.h,
    sahs_model_field_backward_fused) is taken whenever a backward is given sign bits -- every architecture has it: the AudioFaceModel and
    the NeRFaceModel (parts 1, 2, 3), the NeRFaceModel without deformation nets (part 3) -- in the arithmetic backward_gemm_precision()
    names, split-bf16 operands or exact fp32 products; fused_backward(False) (SAHS_BWD_FUSED=0) keeps the per-layer walk for every
    architecture (the A/B reference).  None queries."""
    global _FUSED_BACKWARD
    if enable is not None:
        _FUSED_BACKWARD = bool(enable)
    return _FUSED_BACKWARD


_FUSED_BACKWARD = os.environ.get("SAHS_BWD_FUSED", "1") != "0"


def training_forward_precision(precision=None):
    """Arithmetic of the SAVING forward launches of a training step (RenderRaysFn's kept path, every architecture): "fp32" (default: fp32
    MFMAs, the form the parity tests pin) or "bf16x3" (the split-operand kernels of the SAHS_BF16X3 frame, which then also write the saved
    activations and sign bits; values within a few 1e-6 relative of the fp32 kernel's).  The models with deformation nets save through the
    split chain (a deformation + a radiance launch), the NeRFaceModel without them through one whole-network launch.  SAHS_TRAIN_FORWARD in
    the environment selects the initial value.  None queries."""
    global _TRAIN_FORWARD
    if precision is not None:
        if precision not in ("fp32", "bf16x3"):
            raise _lib.SahsError("training_forward_precision: 'fp32' or 'bf16x3'")
        _TRAIN_FORWARD = precision
    return _TRAIN_FORWARD


_TRAIN_FORWARD = os.environ.get("SAHS_TRAIN_FORWARD", "fp32")
if _TRAIN_FORWARD not in ("fp32", "bf16x3"):
    raise _lib.SahsError("SAHS_TRAIN_FORWARD must be 'fp32' or 'bf16x3', not %r" % (_TRAIN_FORWARD,))


def field_backward_split(flat, frame, level, part, act, grad_flat, grad_cond, d_raw=None, xw_grad_in=None, arch="audio", full_act=False, bits=None):
    """Backward of `part` (FIELD_DEFORM, FIELD_RADIANCE, or 3 = everything) of the field over activations saved by the forward of that
    part.  The seam is d loss / d (x', w), (P,8): FIELD_RADIANCE returns it (the only part that writes one), FIELD_DEFORM starts from
    xw_grad_in, 3 adds xw_grad_in.  full_act: `act` was saved by a WHOLE-network forward and only `part` of it is walked (a saved array of
    column c starts at c * P in every save, so the part's arrays sit at their usual place behind the columns it does not use)."""
    flat, frame, act = _req(flat, "flat_params"), _req(frame, "frame"), _req(act, "act")
    d_raw, xw_grad_in = _req(d_raw, "d_raw"), _req(xw_grad_in, "xw_grad_in")
    P = act.shape[0]
    in_whole = bool(full_act) and int(part) in (FIELD_DEFORM, FIELD_RADIANCE)
    if act.shape[1] != _fn("act_words_part", arch)[0](3 if in_whole else int(part)):
        raise _lib.SahsError("field_backward_split(full_act): the activations were not saved by a whole-network forward" if in_whole else
                             "field_backward_split: the activations were not saved by a forward of part %d" % part)
    if xw_grad_in is not None and xw_grad_in.numel() != P * 8:
        raise _lib.SahsError("field_backward_split: xw_grad_in must hold (P,8)")
    out = torch.empty(P, 8, dtype=torch.float32, device=act.device) if part == FIELD_RADIANCE else None
    fused = bits is not None and _FUSED_BACKWARD
    bits = _req(bits, "bits", torch.int32) if fused else None      # (the per-layer walk reads none)
    if fused:
        saved_mode = 0 if (full_act or int(part) == 3) else int(part)      # part 3 takes both halves of a whole-network save, a part of it its own
        if tuple(bits.shape) != (P, int(_fn("bits_words_part", arch)[0](saved_mode))):
            raise _lib.SahsError("field_backward_split: bits were not written by the forward that saved these activations")
    act_ptr, bits_ptr = _whole_save_part(act, bits, part, arch, P) if in_whole else (_p(act), _p(bits))
    if fused:
        ws = torch.empty(int(_fn("field_backward_fused_workspace_words", arch)[0](int(part), P)), dtype=torch.float32, device=act.device)
        f, name = _fn("field_backward_fused", arch)
        check(f(_p(flat), _p(frame), int(level), int(part), P, act_ptr, bits_ptr, _p(d_raw), _p(xw_grad_in), _p(out), _p(grad_flat), _p(grad_cond), _p(ws),
                _stream()), name)
        return out
    ws = torch.empty(_fn("field_backward_workspace_words", arch)[0](P), dtype=torch.float32, device=act.device)
    f, name = _fn("field_backward_split", arch)
    check(f(_p(flat), _p(frame), int(level), int(part), P, act_ptr, _p(d_raw), _p(xw_grad_in), _p(out), _p(grad_flat), _p(grad_cond), _p(ws), _stream()), name)
    return out


_SIDE_STREAMS = {}


def _side_stream(dev):
    """One extra stream per device for the second of two independent backward walks (RenderRaysFn.backward)."""
    key = torch.device(dev).index if torch.device(dev).index is not None else torch.cuda.current_device()
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=key)
    return _SIDE_STREAMS[key]


def route_xw_grad(src, g_fine, num_coarse):
    """(N,Sf) merge permutation, (N*Sf,8) seam gradient of the fine samples -> (N*Sc,8) for the coarse samples, (N*nf,8) for the new depths."""
    src, g_fine = _req(src, "src", torch.int32), _req(g_fine, "g_fine")
    N, Sf = src.shape
    nf = Sf - int(num_coarse)
    g_c = torch.empty(N * int(num_coarse), 8, dtype=torch.float32, device=src.device)
    g_n = torch.empty(N * nf, 8, dtype=torch.float32, device=src.device)
    check(_lib.lib().sahs_route_xw_grad(N, int(num_coarse), nf, _p(src), _p(g_fine), _p(g_c), _p(g_n), _stream()), "sahs_route_xw_grad")
    return g_c, g_n


def backward_gemm_precision(precision=None):
    """Arithmetic of the backward's dense-layer GEMMs: "bf16x3" (default: split operands on the bf16 matrix pipe, ~1e-5 of scale) or "fp32"
    (f32 MFMAs, the exact A/B reference).  None queries.  Process-wide (include/sahs_nerf.h: sahs_backward_gemm_precision)."""
    names = {SAHS_F32: "fp32", SAHS_BF16X3: "bf16x3"}
    if precision is None:
        return names[_lib.lib().sahs_backward_gemm_precision(-1)]
    code = PRECISIONS[precision] if isinstance(precision, str) else int(precision)
    if _lib.lib().sahs_backward_gemm_precision(code) != code:
        raise _lib.SahsError("backward GEMM precision must be 'fp32' or 'bf16x3'")
    return names[code]


def bf16_exact_leaky(enable=None):
    """The SAHS_BF16 kernels' LeakyReLU: False (default) = packed-integer form on the bf16 bit patterns (slope 0.0095 .. 0.0106), True = the
    reference's max(v, 0.01 v) in fp32 before rounding (include/sahs_nerf.h: sahs_bf16_exact_leaky).  None queries.  Process-wide."""
    return bool(_lib.lib().sahs_bf16_exact_leaky(-1 if enable is None else int(bool(enable))))


LOSS_STATS_WORDS = 64      # include/sahs_nerf.h: [0] loss, [1] last level's mse, [2:14] new sample_prob, [14:26] class counts, [26] rays


def stage1_loss_forward(map_coarse, map_fine, target, mask, class_weights):
    """The Stage-I objective (train_stage_rays_auto.py:455-468) of one ray batch in one launch -> stats (64,) fp32 (see LOSS_STATS_WORDS).
    map_*: (N,15) rendered [rgb3 | seg12] (either may be None), target (N, >=3), mask (N,12) one-hot, class_weights (12,)."""
    mc, mf = _req(map_coarse, "map_coarse"), _req(map_fine, "map_fine")
    target, mask, cw = _req(target, "target"), _req(mask, "mask"), _req(class_weights, "class_weights")
    ref = mc if mc is not None else mf
    N = ref.shape[0]
    if any(t is not None and tuple(t.shape) != (N, 15) for t in (mc, mf)) or tuple(mask.shape) != (N, 12) or target.shape[0] != N or cw.numel() != 12:
        raise _lib.SahsError("stage1_loss_forward: maps (N,15), target (N,>=3), mask (N,12), class_weights (12,)")
    stats = torch.zeros(LOSS_STATS_WORDS, dtype=torch.float32, device=ref.device)
    check(_lib.lib().sahs_stage1_loss_forward(N, _p(mc), _p(mf), _p(target), int(target.shape[1]), _p(mask), _p(cw), _p(stats), _stream()),
          "sahs_stage1_loss_forward")
    return stats


def composite_backward(raw, z, rays, noise, bg, white_background, d_rgb, d_disp, d_acc, d_depth, d_wlast, d_weights=None, loss=None):
    """loss = (map (N,15), target, mask, stats, gscale or None): the level's share of the Stage-I objective's gradient is formed inside
    the kernel (sahs_composite_backward_loss) and added to d_rgb."""
    raw, z, rays = _req(raw, "raw"), _req(z, "z"), _req(rays, "rays")
    N, S = z.shape
    d_raw = torch.empty(N, S, 16, dtype=torch.float32, device=z.device)
    gs = [_req(g, n) for g, n in ((d_rgb, "d_rgb"), (d_disp, "d_disp"), (d_acc, "d_acc"), (d_depth, "d_depth"), (d_wlast, "d_wlast"))]
    head = (N, S, _p(raw), _p(z), _p(rays), int(rays.shape[1]), _p(_req(noise, "noise")), _p(_req(bg, "bg")), int(bool(white_background)),
            *[_p(g) for g in gs])
    if loss is None:
        check(_lib.lib().sahs_composite_backward(*head, _p(_req(d_weights, "d_weights")), _p(d_raw), _stream()), "sahs_composite_backward")
        return d_raw
    if d_weights is not None:
        raise _lib.SahsError("composite_backward: d_weights and loss together are not supported")
    lm, lt, lk, st, gsc = (_req(t, n) for t, n in zip(loss, ("loss_map", "loss_target", "loss_mask", "loss_stats", "loss_gscale")))
    if tuple(lm.shape) != (N, 15) or tuple(lk.shape) != (N, 12) or lt.shape[0] != N or st.numel() < LOSS_STATS_WORDS:
        raise _lib.SahsError("composite_backward: loss operands (N,15), (N,>=3), (N,12), stats (64,)")
    check(_lib.lib().sahs_composite_backward_loss(*head, _p(lm), _p(lt), int(lt.shape[1]), _p(lk), _p(st), _p(gsc), _p(d_raw), _stream()),
          "sahs_composite_backward_loss")
    return d_raw


def _save_named(ctx, **tensors):
    """ctx.save_for_backward under names: what a forward hands its backward is asked for by name, never by position.  None = absent."""
    ctx.saved_names = tuple(tensors)
    ctx.save_for_backward(*tensors.values())


def _load_named(ctx):
    """The tensors of _save_named as attributes (None where absent); a name that was not saved is an AttributeError."""
    return types.SimpleNamespace(**dict(zip(ctx.saved_names, ctx.saved_tensors)))


def _driving_grad(arch, flat, driving, grad_flat, grad_cond):
    """grad_cond (what the field walks left for the folded conditioning) -> the driving input's gradient; the audio net's parameters' into grad_flat."""
    if arch != "audio":      # NeRFaceModel: the driving vector is the expression itself
        return grad_cond[:76].clone()
    grad_drv = torch.zeros_like(driving)
    check(_lib.lib().sahs_conditioning_backward(_p(flat), _p(driving), _p(grad_cond), _p(grad_flat), _p(grad_drv), _stream()),
          "sahs_conditioning_backward")
    return grad_drv


class CompositeFn(torch.autograd.Function):
    """volume_render_radiance_field (volume_rendering_utils.py:7-78) as a differentiable op (seam B3): gradient w.r.t. the radiance
    field through sahs_composite_backward; depths and directions get none (the reference's callers never use those)."""

    @staticmethod
    def forward(ctx, raw, z, rays, noise, bg, white_background):
        outs = composite_forward(raw, z, rays, noise=noise, bg=bg, white_background=white_background)
        _save_named(ctx, raw=raw.detach(), z=z, rays=rays, noise=noise, bg=bg, w_last=outs[3][:, -1])
        ctx.white_background = bool(white_background)
        return outs

    @staticmethod
    def backward(ctx, g_rgb, g_disp, g_acc, g_w, g_depth):
        s = _load_named(ctx)
        c = lambda t: None if t is None else t.contiguous().float()
        d_raw = composite_backward(s.raw, s.z, s.rays, s.noise, s.bg, ctx.white_background, c(g_rgb), c(g_disp), c(g_acc), c(g_depth), None, c(g_w))
        if s.bg is not None and g_rgb is not None:     # the last sample's 15 channels are used verbatim (:28-35): d = w_last * d_rgb
            d_raw[:, -1, :15] += s.w_last[:, None] * g_rgb
        return d_raw, None, None, None, None, None


class SpadeModulateFn(torch.autograd.Function):
    """spade_modulate as a differentiable op (Stage-II refiner training): the forward's two launches, and a two-launch fused backward
    (include/sahs_nerf.h: sahs_spade_modulate_backward) in place of the six autograd nodes of the written-out formula.  Saved: x, gamma,
    the output -- the activation mask is read from it -- and the forward's statistics workspace; beta is not needed.  Gradients are
    formed only for the inputs that ask for one.  Not twice differentiable.  bfloat16 tensors: x, gamma and the output are saved as
    bf16 (half the bytes), the backward is sahs_spade_modulate_backward_bf16, and grad_out must come in the dtype of the saved x."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, slope):
        if not slope >= 0.0:
            raise _lib.SahsError("spade_modulate: the differentiable path needs slope >= 0 (the activation mask is read from the output), got %r" % (slope,))
        x, gamma, out, stats = _spade_modulate_forward(x, gamma, beta, eps, slope)
        _save_named(ctx, x=x.detach(), gamma=gamma.detach(), out=out, stats=stats)
        ctx.eps, ctx.slope = eps, slope
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_out):
        s = _load_named(ctx)
        grad_out = _req(grad_out, "grad_out", s.x.dtype)      # (contiguous: out.sum().backward() hands over a stride-0 expansion)
        if grad_out.shape != s.x.shape:
            raise _lib.SahsError("SpadeModulateFn.backward: gradient of shape %s for an output of shape %s" % (tuple(grad_out.shape), tuple(s.x.shape)))
        planes, hw = s.x.shape[0] * s.x.shape[1], s.x.shape[2] * s.x.shape[3]
        dx, dgamma, dbeta = (torch.empty_like(s.x) if need else None for need in ctx.needs_input_grad[:3])
        work = None
        if dx is not None:
            work = torch.empty(int(_lib.lib().sahs_spade_modulate_backward_workspace_words(planes)), dtype=torch.float32, device=s.x.device)
        f, name = _spade_entry(s.x.dtype, backward=True)
        check(f(planes, hw, _p(s.x), _p(s.gamma), _p(s.out), _p(s.stats), _p(grad_out), float(ctx.eps), float(ctx.slope), _p(dx), _p(dgamma),
                _p(dbeta), _p(work), _stream()), name)
        return dx, dgamma, dbeta, None, None


class SpectralNormalizeFn(torch.autograd.Function):
    """spectral_normalize as ONE differentiable node with N weights in and N normalised weights out (Stage-II refiner training), in place
    of six autograd nodes per weight: dW = G / sigma - (sum(G o W) / sigma^2) u v^T (include/sahs_nerf.h: sahs_spectral_norm_backward),
    one launch per 32 weights.  Saved: the weights as read and each job's saved area -- the u, v, sigma that formed ITS output, so the
    module's buffers may move on before the backward runs.  Gradients are formed only for the weights that ask for one and whose output
    got one; each grad_out must come in the output's dtype.  Not twice differentiable."""
    LEADING = 5      # us, vs, training, eps, out_dtype come before the weights

    @staticmethod
    def forward(ctx, us, vs, training, eps, out_dtype, *weights):
        Ws, outs, saved = _spectral_normalize_forward(weights, us, vs, training, eps, out_dtype)
        named = {"weight%d" % k: W.detach() for k, W in enumerate(Ws)}
        named.update(("saved%d" % k, s) for k, s in enumerate(saved))
        _save_named(ctx, **named)
        ctx.out_dtype = out_dtype
        ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        s = _load_named(ctx)
        lead = SpectralNormalizeFn.LEADING
        jobs = [k for k, g in enumerate(grads) if g is not None and ctx.needs_input_grad[lead + k]]
        Ws = [getattr(s, "weight%d" % k) for k in jobs]
        Gs = [_req(grads[k], "SpectralNormalizeFn.backward: grad_out[%d]" % k, ctx.out_dtype) for k in jobs]
        for k, W, G in zip(jobs, Ws, Gs):
            if G.shape != W.shape:
                raise _lib.SahsError("SpectralNormalizeFn.backward: gradient %d of shape %s for an output of shape %s" % (k, tuple(G.shape), tuple(W.shape)))
        out = [None] * len(grads)
        if jobs:
            saved, dims = [getattr(s, "saved%d" % k) for k in jobs], _spectral_norm_dims(Ws)
            dWs = _flat_views([W.shape for W in Ws], torch.float32, Ws[0].device)
            f = _lib.lib().sahs_spectral_norm_backward
            for a in range(0, len(jobs), SPECTRAL_NORM_MAX_JOBS):
                cut = slice(a, a + SPECTRAL_NORM_MAX_JOBS)
                hs, ws = zip(*dims[cut])
                n = len(hs)
                check(f(n, _pointer_table(Ws[cut]), _pointer_table(saved[cut]), _pointer_table(Gs[cut]), _pointer_table(dWs[cut]),
                        (ctypes.c_int * n)(*hs), (ctypes.c_int * n)(*ws), int(ctx.out_dtype == torch.bfloat16), _stream()),
                      "sahs_spectral_norm_backward")
            for k, dW in zip(jobs, dWs):
                out[k] = dW
        return (None,) * lead + tuple(out)


class FieldFn(torch.autograd.Function):
    """The field evaluation of seam B2, model(level, x, driving, pose) -> (P, 16), differentiable w.r.t. the parameters (as the
    canonical flat buffer) and the driving input; the sample points themselves get no gradient (no caller of the reference's asks
    for one).  fp32.  Points are passed as zero-length rays, as in the no-grad path of the seam."""

    BLOCK = 2_000_000     # samples per saved-activation block (sahs_field_backward takes at most 4e6 per call; 19 KB each)

    @staticmethod
    def forward(ctx, flat, driving, pose, rays, z, packed, level, arch):
        frame = fold_conditioning(flat.detach(), driving.detach(), pose, arch=arch)
        # the saved activations are plane-per-layer over the P of ONE forward call, so a large batch is cut into blocks HERE and
        # each block keeps its own buffer (a row slice of one big buffer would hand the backward the wrong planes)
        N = z.shape[0]
        rows = max(1, FieldFn.BLOCK // max(1, z.shape[1]))
        raws, acts = [], {}
        for s in range(0, N, rows):
            r, acts["act%d" % len(raws)] = field_forward_save(packed, frame, level, rays[s:s + rows].contiguous(), z[s:s + rows].contiguous(), arch)
            raws.append(r)
        _save_named(ctx, flat=flat.detach(), driving=driving.detach(), frame=frame, **acts)
        ctx.level, ctx.arch, ctx.block, ctx.num_blocks = level, arch, rows * z.shape[1], len(raws)
        return raws[0] if len(raws) == 1 else torch.cat(raws, dim=0)

    @staticmethod
    def backward(ctx, g_raw):
        s = _load_named(ctx)
        acts = [getattr(s, "act%d" % i) for i in range(ctx.num_blocks)]
        grad_flat = torch.zeros_like(s.flat)
        grad_cond = torch.zeros(128, dtype=torch.float32, device=s.flat.device)
        g = g_raw.contiguous().float().view(-1, 16)
        if sum(a.shape[0] for a in acts) != g.shape[0]:
            raise _lib.SahsError("FieldFn.backward: %d gradient rows for %d saved samples" % (g.shape[0], sum(a.shape[0] for a in acts)))
        for i, act in enumerate(acts):
            field_backward(s.flat, s.frame, ctx.level, act, g[i * ctx.block: i * ctx.block + act.shape[0]], grad_flat, grad_cond, ctx.arch)
        return grad_flat, _driving_grad(ctx.arch, s.flat, s.driving, grad_flat, grad_cond), None, None, None, None, None, None


class RenderRaysFn(torch.autograd.Function):
    """predict_and_render_radiance (train_utils.py:72-206) for one ray chunk, differentiable w.r.t. the model
    parameters (as the canonical flat buffer) and the audio window.
    forward, by ctx.strategy.  A chunk of at most BLOCK_RAYS rays (a training batch) keeps the field activations of both passes (19 KB per
    sample, 7.5 GB for 2048 rays x 192 samples): "shared" = the split chain, the deformation nets once per depth; "whole" = a
    whole-network save per level (SHARE_DEFORMATION = False, and the NeRFaceModel without deformation nets).  "recompute" (larger chunks,
    num_fine = 0) = render_rays: only the depths are kept and the field is run again block by block in backward.
    backward (_RenderBackward): per level -- composite backward, field walk(s) -- then the conditioning backward."""

    BLOCK_RAYS = 4096
    SHARE_DEFORMATION = True      # kept activations: deformation nets once per depth, forward AND backward (the fine pass's gradient w.r.t.
                                  # the coarse samples' (x', w) is added at the seam of the coarse pass's backward); False = the plain chain

    @staticmethod
    def forward(ctx, flat, audio, pose, rays, bg, t_rand, noise_c, u, noise_f, packed, num_coarse, num_fine, lindisp, white_background,
                arch="audio", loss_target=None, loss_mask=None, loss_weights=None, packed_x3=None):
        """With loss_target (N,>=3), loss_mask (N,12), loss_weights (12,) the op also returns (loss, stats) of the Stage-I objective
        (stage1_loss_forward) and its backward forms that loss's gradient inside the composite backward kernels.
        packed_x3 (pack_weights(flat, SAHS_BF16X3, arch); kept activations, every architecture): the saving forward launches run on the
        split-operand kernels (training_forward_precision "bf16x3") -- with deformation nets the coarse pass as a deformation + a radiance
        launch into one whole-network save, without them one whole-network launch per level."""
        frame = fold_conditioning(flat.detach(), audio.detach(), pose, arch=arch)
        N, dev, Sf = rays.shape[0], rays.device, num_coarse + num_fine
        kept = N <= RenderRaysFn.BLOCK_RAYS and num_fine > 0
        shared = kept and RenderRaysFn.SHARE_DEFORMATION and arch != "nerface_static"
        ctx.strategy = "shared" if shared else "whole" if kept else "recompute"
        ctx.arch, ctx.num_coarse, ctx.num_fine, ctx.white_background = arch, num_coarse, num_fine, bool(white_background)
        saved = dict(flat=flat.detach(), audio=audio.detach(), rays=rays, frame=frame, packed=packed, bg=bg, noise_c=noise_c, noise_f=noise_f,
                     map_c=None, map_f=None, loss_target=None, loss_mask=None, loss_stats=None)
        # sign bits of the fused walk (None: this backward reads none; of whole-network saves only the NeRFaceModel without deformation nets has one)
        sign_bits = lambda samples, mode: alloc_sign_bits(samples, mode, arch, dev) if (shared or arch == "nerface_static") else None
        bits0 = sign_bits(N * num_coarse, FIELD_ALL) if kept else None
        pk, prec = (packed_x3, SAHS_BF16X3) if (packed_x3 is not None and bits0 is not None) else (packed, SAHS_F32)
        xw = torch.empty(N, Sf, 8, dtype=torch.float32, device=dev) if shared else None      # x', w of every depth: the split chain's seam

        def level_pass(level, z, noise, z_new=None, src=None):
            # one level of a kept strategy: the saving field launch(es) (shared: as sahs_model_render_rays_rows' split evaluation, whole: as
            # sahs_render_rays), then the composite
            nonlocal xw
            if not shared:
                bits = bits0 if level == 0 else sign_bits(z.numel(), FIELD_ALL)
                raw, act = field_forward_save(pk, frame, level, rays, z, arch, bits=bits, precision=prec)
                saved.update({"act%d" % level: act, "bits%d" % level: bits})
            elif level == 0 and prec == SAHS_F32:
                raw, act = field_forward_split_save(pk, frame, 0, FIELD_ALL, rays, xw, z=z, arch=arch, bits=bits0)
                saved.update(act0=act, bits0=bits0)
            elif level == 0:      # the split-operand kernels exist per part: two launches fill one whole-network save
                whole = (torch.empty(N * num_coarse, _fn("act_words_part", arch)[0](FIELD_ALL), dtype=torch.float32, device=dev), bits0)
                field_forward_split_save(pk, frame, 0, FIELD_DEFORM, rays, xw, z=z, arch=arch, precision=prec, whole=whole)
                raw, _ = field_forward_split_save(pk, frame, 0, FIELD_RADIANCE, rays, xw, arch=arch, precision=prec, whole=whole,
                                                  src=torch.arange(num_coarse, dtype=torch.int32, device=dev).repeat(N, 1))      # (its own samples in order)
                saved.update(act0=whole[0], bits0=bits0)
            else:                 # deformation nets on the new depths only, radiance nets on every depth through the merge permutation
                bits_d, bits_r = sign_bits(N * num_fine, FIELD_DEFORM), sign_bits(N * Sf, FIELD_RADIANCE)
                _, act_d = field_forward_split_save(pk, frame, 1, FIELD_DEFORM, rays, xw, z=z_new, xw_col0=num_coarse, arch=arch, bits=bits_d, precision=prec)
                raw, act_r = field_forward_split_save(pk, frame, 1, FIELD_RADIANCE, rays, xw, src=src, arch=arch, bits=bits_r, precision=prec)
                saved.update(act_d=act_d, bits_d=bits_d, act_r=act_r, bits_r=bits_r, src=src)
                xw = None         # (freed before the fine composite)
            saved["raw%d" % level] = raw
            return composite_forward(raw, z, rays, noise, bg, white_background)

        if kept:
            z_c = stratified_depths(rays, num_coarse, lindisp, t_rand)
            rgb_c, disp_c, acc_c, w_c, _ = level_pass(0, z_c, noise_c)
            z_f, z_new, src = resample_merge(z_c, w_c, num_fine, u=u) if shared else (resample(z_c, w_c, num_fine, u), None, None)
            rgb_f, disp_f, acc_f, w_f, depth_f = level_pass(1, z_f, noise_f, z_new, src)
            saved.update(z_c=z_c, z_f=z_f)
            outs = (rgb_c, disp_c, acc_c, rgb_f, disp_f, acc_f, w_f[:, -1].contiguous(), depth_f)
        else:
            ws = {}
            outs = render_rays(packed, frame, rays, num_coarse, num_fine, precision=SAHS_F32, lindisp=lindisp, white_background=white_background,
                               bg=bg, t_rand=t_rand, noise_c=noise_c, u=u, noise_f=noise_f, workspace=ws, arch=arch)
            saved.update(z_c=ws["z_c"].clone(), z_f=ws["z_f"].clone() if num_fine > 0 else None)
        if loss_target is not None:
            tgt, msk = loss_target.detach().float().contiguous(), loss_mask.detach().float().contiguous()
            rgb_f = outs[3] if num_fine > 0 else None
            stats = stage1_loss_forward(outs[0], rgb_f, tgt, msk, loss_weights.detach().float().contiguous())
            saved.update(map_c=outs[0], map_f=rgb_f, loss_target=tgt, loss_mask=msk, loss_stats=stats)
            ctx.mark_non_differentiable(stats)
            outs = tuple(outs) + (stats[0].clone(), stats)
        _save_named(ctx, **saved)
        return outs

    @staticmethod
    def backward(ctx, g_rgb_c, g_disp_c, g_acc_c, g_rgb_f, g_disp_f, g_acc_f, g_wbg, g_depth_f, g_loss=None, g_stats=None):
        # level -> (d_rgb, d_disp, d_acc, d_depth, d_wlast); coarse only (train_utils.py:148-149): depth and weights[:, -1] are the COARSE pass's
        grads = ({1: (g_rgb_f, g_disp_f, g_acc_f, g_depth_f, g_wbg), 0: (g_rgb_c, g_disp_c, g_acc_c, None, None)} if ctx.num_fine > 0 else
                 {0: (g_rgb_c, g_disp_c, g_acc_c, g_depth_f, g_wbg)})
        bw = _RenderBackward(ctx, _load_named(ctx), grads, g_loss)
        # the fused walk is two full-chip persistent launches per part: run side by side they starve each other (measured: 14.0 ms per step on
        # two streams, 13.3 on one), so the pairwise two-stream issue is for the per-layer walks only (fused_backward(False))
        if (ctx.strategy == "shared" and not (bw.s.bits0 is not None and _FUSED_BACKWARD) and bw.has_grad[0] and bw.has_grad[1]
                and not os.environ.get("SAHS_BWD_ONE_STREAM")):
            bw.two_streams()
        else:
            bw.one_stream()
        return (bw.grad_flat, _driving_grad(ctx.arch, bw.s.flat, bw.s.audio, bw.grad_flat, bw.grad_cond)) + (None,) * 17


class _RenderBackward:
    """RenderRaysFn.backward: saved state `s`, upstream gradients per level (fine first), the buffers every walk adds into (atomically), and
    the steps that its two issue orders, one_stream and two_streams, are made of."""

    def __init__(self, ctx, s, grads, g_loss):
        self.s, self.grads, self.arch, self.strategy, self.num_coarse, self.white = s, grads, ctx.arch, ctx.strategy, ctx.num_coarse, ctx.white_background
        self.z, self.noise, self.loss_map = {0: s.z_c, 1: s.z_f}, {0: s.noise_c, 1: s.noise_f}, {0: s.map_c, 1: s.map_f}
        self.gscale = g_loss.detach().float().reshape(1).contiguous() if (s.loss_stats is not None and g_loss is not None) else None
        self.has_grad = {level: self.gscale is not None or any(g is not None for g in gs) for level, gs in grads.items()}
        self.grad_flat = torch.zeros_like(s.flat)
        self.grad_cond = torch.zeros(128, dtype=torch.float32, device=s.rays.device)

    def composite(self, level, raw, sl=slice(None)):
        """The composite backward of rays `sl` of a level, with the level's loss operands (level 0: the coarse map) -> d_raw (P,16)."""
        s = self.s
        cut = lambda t: None if t is None else t[sl].contiguous()
        loss = None if self.gscale is None else (cut(self.loss_map[level]), cut(s.loss_target), cut(s.loss_mask), s.loss_stats, self.gscale)
        return composite_backward(raw, cut(self.z[level]), cut(s.rays), cut(self.noise[level]), cut(s.bg), self.white,
                                  *[None if g is None else g[sl].contiguous().float() for g in self.grads[level]], loss=loss).view(-1, 16)

    def whole_walk(self, level, act, bits, d_raw, xw_grad_in=None):
        """A level's whole-network save walked at once: fused when sign bits were kept, else per-layer; shared level 0 adds the fine pass's seam gradient."""
        s = self.s
        if self.strategy == "shared" or bits is not None:
            field_backward_split(s.flat, s.frame, level, 3, act, self.grad_flat, self.grad_cond, d_raw=d_raw, xw_grad_in=xw_grad_in, arch=self.arch, bits=bits)
        else:
            field_backward(s.flat, s.frame, level, act, d_raw, self.grad_flat, self.grad_cond, self.arch)

    def part_walk(self, level, part, d_raw=None, xw_grad_in=None, side=None):
        """shared strategy: the walk of FIELD_RADIANCE (-> its seam gradient) or FIELD_DEFORM of a level (level 1 saved its parts apart,
        level 0 as one whole-network save); side = (stream, its grad_cond): issued there, behind everything the current stream holds so far."""
        s = self.s
        act, bits = (s.act0, s.bits0) if level == 0 else (s.act_r, s.bits_r) if part == FIELD_RADIANCE else (s.act_d, s.bits_d)
        walk = lambda grad_cond: field_backward_split(s.flat, s.frame, level, part, act, self.grad_flat, grad_cond, d_raw=d_raw, xw_grad_in=xw_grad_in,
                                                      arch=self.arch, full_act=(level == 0), bits=bits)
        if side is None:
            return walk(self.grad_cond)
        main = torch.cuda.current_stream(s.rays.device)
        side[0].wait_stream(main)
        with torch.cuda.stream(side[0]):
            out = walk(side[1])
        # (all made on the main stream: the allocator must not hand them out again before the side stream is done; the walk's result the other way round)
        for t in (s.flat, s.frame, act, bits, self.grad_flat, side[1], d_raw, xw_grad_in):
            if t is not None:
                t.record_stream(side[0])
        if out is not None:
            out.record_stream(main)
        return out

    def fine_walks(self, d_raw):
        """shared, level 1: radiance walk, seam routing through the merge permutation, deformation walk of the new depths -> the coarse samples' seam gradient."""
        g_f = self.part_walk(1, FIELD_RADIANCE, d_raw=d_raw)
        xwg_coarse, g_new = route_xw_grad(self.s.src, g_f, self.num_coarse)
        self.part_walk(1, FIELD_DEFORM, xw_grad_in=g_new)
        return xwg_coarse

    def one_stream(self):
        """BLOCK_RAYS rays at a time (a kept chunk is one block; recompute: the whole-network saving forward again per block), level by level.
        A level without upstream gradient is skipped -- but shared level 0 still runs when the fine pass left a seam gradient for its samples."""
        s, N = self.s, self.s.rays.shape[0]
        for start in range(0, N, RenderRaysFn.BLOCK_RAYS):
            sl = slice(start, min(N, start + RenderRaysFn.BLOCK_RAYS))
            xwg_coarse = None
            for level in self.grads:
                if not self.has_grad[level] and xwg_coarse is None:
                    continue
                if (self.strategy, level) == ("shared", 1):
                    xwg_coarse = self.fine_walks(self.composite(1, s.raw1, sl))
                    continue
                if self.strategy == "recompute":
                    (raw, act), bits = field_forward_save(s.packed, s.frame, level, s.rays[sl].contiguous(), self.z[level][sl].contiguous(), self.arch), None
                else:
                    raw, act, bits = getattr(s, "raw%d" % level), getattr(s, "act%d" % level), getattr(s, "bits%d" % level)
                d_raw = self.composite(level, raw, sl)
                self.whole_walk(level, act, bits, d_raw, xwg_coarse)
                del raw, act, d_raw

    def two_streams(self):
        """shared strategy, per-layer walks, both levels: the two radiance walks are independent of each other, and so are the two deformation
        walks that follow (coarse / new depths; level 0 as part 2, then part 1 of its whole-network save), so each pair runs on two streams.  A
        walk is ~75 dependent GEMM launches whose fixed costs leave most of the chip idle; the other stream's fill it."""
        s = self.s
        d_raw1, d_raw0 = self.composite(1, s.raw1), self.composite(0, s.raw0)
        side = (_side_stream(s.rays.device), torch.zeros_like(self.grad_cond))
        main = torch.cuda.current_stream(s.rays.device)
        g_c0 = self.part_walk(0, FIELD_RADIANCE, d_raw=d_raw0, side=side)
        g_f = self.part_walk(1, FIELD_RADIANCE, d_raw=d_raw1)
        xwg_coarse, g_new = route_xw_grad(s.src, g_f, self.num_coarse)
        main.wait_stream(side[0])
        xwg0 = g_c0 + xwg_coarse          # the seam gradient of the coarse samples: their own radiance walk's + the fine pass's share
        self.part_walk(0, FIELD_DEFORM, xw_grad_in=xwg0, side=side)
        self.part_walk(1, FIELD_DEFORM, xw_grad_in=g_new)
        main.wait_stream(side[0])
        self.grad_cond += side[1]
