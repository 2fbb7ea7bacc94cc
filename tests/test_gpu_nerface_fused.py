"""The fused backward walk of the NeRFaceModels (include/sahs_nerf.h: sahs_model_field_backward_fused, SAHS_MODEL_NERFACE and
SAHS_MODEL_NERFACE_STATIC; csrc/field_bwd_chain*.hip built for SAHS_MODEL 1 and 2):

  * against the per-layer walk on the SAME saved activations and upstream gradients, in both backward arithmetics, at training-step
    size and at a ragged size -- every parameter gradient, the driving and pose-encoding gradients and (radiance part) the seam;
  * against float64 autograd of the eager field at the sample counts of the tails (tests/test_gpu_backward_tails.py: its sizes, its
    yardstick and its sensitivity-floor rule), with a negative control per architecture;
  * through a NeRFaceModel training step (run_one_iter_of_nerf with the fused loss), which must take the fused walk and match the same
    step under ops.fused_backward(False)."""
import numpy as np
import pytest
import torch

from conftest import pkg
from test_gpu_backward_tails import DEV, FIELD_BOUNDS, ILL_CONDITIONED, NEGATIVE_SIZE, SIZES, _eager, _errors, _masks, _part, _sensitivity, _setup

pytestmark = pytest.mark.gpu

ARCHS = ("nerface", "nerface_static")

# fused vs per-layer walk on the same saved activations: worst |fused - per-layer| / scale per (arch, GEMM arithmetic), ~3-4x the worst
# observed over both levels, both forms and both sizes (NeRFace 1.4e-5 in f32 products, 1.9e-5 with split-bf16 operands; static 9.2e-6,
# 2.1e-5 -- fc_feat's bias, a sum over every sample, at P = 131,072), and never looser than the per-layer walk's own float64 bound
VS_LAYER_BOUNDS = {("nerface", "fp32"): 5e-5, ("nerface", "bf16x3"): 7e-5,
                   ("nerface_static", "fp32"): 4e-5, ("nerface_static", "bf16x3"): 8e-5}
VS_LAYER_ILL = {"hyper_sheep_mlp.fc_ambient.bias": 5e-2}      # ILL_CONDITIONED of the tails file: a cancelling sum behind 2^14

# fused walk vs float64 autograd: the per-layer walk's bounds (the same products in another summation order).  Observed over all sizes:
# NeRFace 1.6e-3 (the warp field's fc_final bias at P = 2,049: a cancelling sum behind the 2^14-amplified seam), static 7.9e-5 in f32
# products and 2.5e-4 with split-bf16 operands (fc_feat's bias at P = 1,023, the cancelling sum the tails file names)
FUSED_BOUNDS = {(arch, prec): FIELD_BOUNDS[(arch, "f32", "layer", prec)] for arch in ARCHS for prec in ("fp32", "bf16x3")}


def _geometry(arch, N, S, seed):
    ops, W = pkg("ops"), pkg("weights")
    gen = torch.Generator(device=DEV).manual_seed(seed)
    sd = W.hash_state_dict(0, 8.0, 30.0, model=arch)
    flat = torch.from_numpy(W.flatten_state_dict(sd, model=arch)).to(DEV)
    driving = torch.randn(76, device=DEV, generator=gen) * 0.5
    near, far, cam = 0.2, 0.8, 0.5
    pose = torch.from_numpy(np.concatenate([np.eye(3), [[0.0], [0.0], [cam]]], 1).astype(np.float32)).to(DEV)
    frame = ops.fold_conditioning(flat, driving, pose, arch=arch)
    rays = torch.zeros(N, 8, device=DEV)
    rays[:, 2] = cam
    rays[:, 3:6] = torch.randn(N, 3, device=DEV, generator=gen) * 0.15 + torch.tensor([0, 0, -1.0], device=DEV)
    rays[:, 6], rays[:, 7] = near, far
    z = torch.sort(torch.rand(N, S, device=DEV, generator=gen) * (far - near) + near, dim=1).values
    d_raw = torch.randn(N * S, 16, device=DEV, generator=gen)
    return flat, frame, rays, z, d_raw


def _save(arch, flat, frame, level, rays, z):
    """the whole-network saving forward with sign bits (sahs_model_field_forward_save_bits) -> (act, bits)"""
    ops = pkg("ops")
    bits = ops.alloc_sign_bits(z.numel(), ops.FIELD_ALL, arch, DEV)
    assert bits is not None and bits.shape[1] == (112 if arch == "nerface" else 64)
    _, act = ops.field_forward_save(ops.pack_weights(flat, arch=arch), frame, level, rays, z, arch, bits=bits)
    return act, bits


def _walk(arch, flat, frame, level, act, bits, d_raw, fused, prec, form):
    """-> {tensor name: gradient}, grad_cond, seam (form "part2+1": the radiance part's seam gradient, else None)"""
    ops = pkg("ops")
    gf, gc = torch.zeros_like(flat), torch.zeros(128, device=DEV)
    seam = None
    try:
        ops.backward_gemm_precision(prec)
        ops.fused_backward(fused)
        if form == "part3":
            ops.field_backward_split(flat, frame, level, 3, act, gf, gc, d_raw=d_raw, arch=arch, bits=bits)
        else:           # radiance part of the whole save, then its deformation part from the seam (RenderRaysFn's chain)
            seam = ops.field_backward_split(flat, frame, level, ops.FIELD_RADIANCE, act, gf, gc, d_raw=d_raw, arch=arch, full_act=True, bits=bits)
            ops.field_backward_split(flat, frame, level, ops.FIELD_DEFORM, act, gf, gc, xw_grad_in=seam, arch=arch, full_act=True, bits=bits)
        torch.cuda.synchronize()
    finally:
        ops.backward_gemm_precision("bf16x3")
        ops.fused_backward(True)
    return gf, gc, seam


def _forms(arch):
    return ("part3", "part2+1") if arch == "nerface" else ("part3",)


@pytest.mark.parametrize("N,S", [(2048, 64), (1237, 41)], ids=["step", "ragged"])
@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
@pytest.mark.parametrize("arch", ARCHS)
def test_fused_vs_per_layer_walk(arch, prec, N, S):
    """Same saved activations, same sign bits, same upstream gradients, both levels: every gradient tensor of the fused walk within
    VS_LAYER_BOUNDS of the per-layer walk's in the same arithmetic (the products agree; the summation order does not)."""
    W = pkg("weights")
    flat, frame, rays, z, d_raw = _geometry(arch, N, S, 31 + N)
    off = W.canonical_offsets(arch)
    bound = VS_LAYER_BOUNDS[(arch, prec)]
    worst, failures = {}, []
    for level in (0, 1):
        act, bits = _save(arch, flat, frame, level, rays, z)
        for form in _forms(arch):
            a = _walk(arch, flat, frame, level, act, bits, d_raw, True, prec, form)
            b = _walk(arch, flat, frame, level, act, bits, d_raw, False, prec, form)
            errs = {}
            for k, (o, shape) in off.items():
                n = int(np.prod(shape))
                ga, gb = a[0][o:o + n], b[0][o:o + n]
                sc = float(gb.abs().max())
                if sc == 0.0:
                    assert float(ga.abs().max()) == 0.0, (k, level, form)      # (the other level's net)
                    continue
                errs[k] = float((ga - gb).abs().max()) / sc
            for name, sl in (("driving", slice(0, 76)), ("pose36", slice(80, 116))):
                sc = float(b[1][sl].abs().max())
                errs[name] = float((a[1][sl] - b[1][sl]).abs().max()) / sc if sc > 0 else float(a[1][sl].abs().max())
            if b[2] is not None:
                cols = [0, 1, 2, 4]      # x', w (the 1-D ambient coordinate)
                errs["seam"] = float((a[2][:, cols] - b[2][:, cols]).abs().max()) / float(b[2][:, cols].abs().max())
            for k, e in errs.items():
                worst[(level, form, k)] = e
                if e > max(bound, VS_LAYER_ILL.get(k, 0.0)):
                    failures.append("level %d %s %s: %.3e of scale (bound %.1e)" % (level, form, k, e, bound))
        del act, bits
    top = sorted(((v, k) for k, v in worst.items() if k[2] not in VS_LAYER_ILL), reverse=True)[:4]
    print("%s %s P=%d: fused vs per-layer, worst %s" % (arch, prec, N * S, ", ".join("%s %.2e" % (k, v) for v, k in top)))
    assert bound <= FIELD_BOUNDS[(arch, "f32", "layer", prec)]
    assert not failures, "\n".join(failures)


def _fused_case(arch, N, S, zero_last=False):
    c = _setup(arch, N, S)
    P, lv = c["P"], c["level"]
    ops = pkg("ops")
    packed = ops.pack_weights(c["flat"], arch=arch)
    bits = ops.alloc_sign_bits(P, ops.FIELD_ALL, arch, DEV)
    _, act = ops.field_forward_save(packed, c["frame"], lv, c["rays"], c["z"], arch, bits=bits)
    torch.cuda.synchronize()
    masks = _masks(act, arch, P)
    ref = _eager(c, masks, 0, P)
    last = _eager(c, masks, P - 1, P)
    sens = _sensitivity(ref, last)
    d_raw = c["d_raw"]
    if zero_last:
        d_raw = d_raw.clone()
        d_raw[-1] = 0.0
    failures = []
    for prec in ("fp32", "bf16x3"):
        for form in _forms(arch):
            gf, gc, _ = _walk(arch, c["flat"], c["frame"], lv, act, bits, d_raw, True, prec, form)
            got = {k: gf[o:o + int(np.prod(shape))].view(shape) for k, (o, shape) in c["off"].items() if k in ref}
            got["driving"], got["pose36"] = gc[0:76], gc[80:116]
            errs = _errors(got, ref)
            bound = FUSED_BOUNDS[(arch, prec)]
            allow = {k: max(bound, ILL_CONDITIONED.get((arch, k), 0.0)) for k in errs}
            parts = {_part(k) for k in errs if _part(k) in ("deformation", "radiance")}
            floor = min(sens[p] for p in parts) / 2.0
            top = sorted(errs.items(), key=lambda kv: -kv[1])[:3]
            tag = "%s P=%d (%dx%d) fused/%s/%s" % (arch, P, N, S, prec, form)
            print("%s%s: worst %s  bound %.1e  sensitivity floor %.2e" % ("[last sample zeroed] " if zero_last else "", tag,
                  ", ".join("%s %.2e" % kv for kv in top), bound, floor))
            if zero_last:
                if top[0][1] <= bound:
                    failures.append("%s: the last sample's upstream rows dropped, yet worst %.2e <= bound %.1e" % (tag, top[0][1], bound))
                continue
            if bound > floor:
                failures.append("%s: bound %.1e could not see sample P-1 (half its contribution: %.2e)" % (tag, bound, floor))
            if any(errs[k] > allow[k] for k in errs):
                failures.append("%s: %s" % (tag, ", ".join("%s %.3e of scale" % kv for kv in top)))
    del act, bits, masks, ref, last
    torch.cuda.empty_cache()
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("N,S", SIZES, ids=["P%d" % (n * s) for n, s in SIZES])
@pytest.mark.parametrize("arch", ARCHS)
def test_fused_walk_vs_float64(arch, N, S):
    """Every parameter gradient of the level's field and the driving / pose-encoding gradients of the FUSED walk against float64
    autograd of the eager field on the HIP forward's side of every kink, at the tails' sample counts, upstream gradients weighted
    towards the tail and block-edge samples (tests/test_gpu_backward_tails.py)."""
    _fused_case(arch, N, S)


@pytest.mark.parametrize("arch", ARCHS)
def test_fused_walk_negative_control(arch):
    """With the upstream rows of sample P-1 zeroed, the fused walk fails the bound it is held to."""
    _fused_case(arch, *NEGATIVE_SIZE, zero_last=True)


@pytest.mark.parametrize("arch", ARCHS)
def test_train_step_takes_the_fused_walk(arch, monkeypatch):
    """A NeRFaceModel training step (run_one_iter_of_nerf with the fused Stage-I loss, as training.train_step) allocates sign bits and
    walks its backward fused; loss and every gradient match the same step under ops.fused_backward(False)."""
    sahs, ops, W, Tr = pkg(), pkg("ops"), pkg("weights"), pkg("training")
    cfg = sahs.default_config("expression" if arch == "nerface" else "expression_static")
    fw = W.flatten_state_dict(W.hash_state_dict(0, 8.0, 30.0, model=arch), model=arch)
    R = 512
    gen = torch.Generator(device=DEV).manual_seed(23)
    expr = torch.randn(76, device=DEV, generator=gen) * 0.5
    pose = torch.from_numpy(np.concatenate([np.eye(3), [[0.0], [0.0], [0.5]]], 1).astype(np.float32)).to(DEV)
    ro = torch.zeros(R, 3, device=DEV)
    ro[:, 2] = 0.5
    rd = torch.randn(R, 3, device=DEV, generator=gen) * 0.15 + torch.tensor([0, 0, -1.0], device=DEV)
    bg = torch.cat([torch.rand(R, 3, device=DEV, generator=gen), torch.ones(R, 1, device=DEV), torch.zeros(R, 11, device=DEV)], 1)
    cls = torch.randint(0, 12, (R,), device=DEV, generator=gen)
    mask = torch.nn.functional.one_hot(cls, 12).float()
    target = torch.rand(R, 3, device=DEV, generator=gen)
    cw = Tr.sample_prob_weights(DEV)

    calls = []
    real_split, real_alloc = ops.field_backward_split, ops.alloc_sign_bits

    def spy_split(*a, **k):
        calls.append(("walk", k.get("bits") is not None and ops.fused_backward()))
        return real_split(*a, **k)

    def spy_alloc(*a, **k):
        b = real_alloc(*a, **k)
        calls.append(("bits", b is not None))
        return b

    monkeypatch.setattr(ops, "field_backward_split", spy_split)
    monkeypatch.setattr(ops, "alloc_sign_bits", spy_alloc)
    res = {}
    try:
        for fused in (True, False):
            ops.fused_backward(fused)
            calls.clear()
            model = sahs.NeRFaceModel(cfg).to(DEV).load_flat(fw).train()
            e = expr.clone().requires_grad_(True)
            torch.manual_seed(7)      # the step's draws (perturbation, noise, importance samples): the same in both runs
            outs = sahs.run_one_iter_of_nerf(0, 0, None, model, ro, rd, cfg, mode="train", driving=e, pose=pose, background_prior=bg,
                                             inHead=mask, _loss=(target, mask, cw))
            outs[8].backward()
            torch.cuda.synchronize()
            walks = [v for kind, v in calls if kind == "walk"]
            assert any(v for kind, v in calls if kind == "bits"), "no sign bits were allocated"
            assert walks and all(v == fused for v in walks), calls
            res[fused] = (float(outs[8]), {k: p.grad.clone() for k, p in model.named_parameters()}, e.grad.clone())
    finally:
        ops.fused_backward(True)
    assert abs(res[True][0] - res[False][0]) <= 1e-6 * abs(res[False][0])      # the forward is the same launch sequence
    worst = {}
    for k, g in res[False][1].items():
        sc = float(g.abs().max())
        if sc > 0:
            worst[k] = float((res[True][1][k] - g).abs().max()) / sc
    worst["expression"] = float((res[True][2] - res[False][2]).abs().max()) / float(res[False][2].abs().max())
    top = sorted(worst.items(), key=lambda kv: -kv[1])[:4]
    print("%s train step, fused vs per-layer walk (bf16x3): %s" % (arch, ", ".join("%s %.2e" % kv for kv in top)))
    bound = VS_LAYER_BOUNDS[(arch, "bf16x3")]
    assert all(v <= max(bound, VS_LAYER_ILL.get(k, 0.0)) for k, v in worst.items()), top
