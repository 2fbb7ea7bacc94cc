"""The training backward against float64 autograd of the eager restatement (oracle/torch_eager.py) at the sample counts of its tails:
the field backward (fused walk, per-layer walk; every architecture) on both sides of the 16 / 32 / 128 / 1,024-sample edges of its
tiles, K-steps and item ranges, the composite backward at every block count, and the Stage-I loss kernel across its 1,024-ray stride.

Every field case checks its own sensitivity: its bound must be at most half of what sample P-1 alone contributes to at least one
gradient of every part (so that a dropped or doubled tail sample cannot pass), and once per path, at a ragged size, the HIP backward with
the last sample's upstream rows zeroed must FAIL the bound."""
import time

import numpy as np
import pytest
import torch

from conftest import pkg

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")

# P = N x S on every edge of the walks: one sample; < one f32 wave's 16 (one partial K-step); around a split-operand wave's 32; one
# 128-sample chain tile + 1; either side of the 1,024-sample range floor; the first fp32 item plan with more than one range per unit;
# 256 chain tiles + 1 (a persistent workgroup's second round holds one sample); training-step size, ragged ranges everywhere
SIZES = [(1, 1), (17, 1), (3, 11), (3, 43), (31, 33), (25, 41), (683, 3), (331, 99), (1043, 191)]
NEGATIVE_SIZE = (25, 41)
CHUNK = 32768          # samples per float64 evaluation
EDGE_GAIN = 31.0       # upstream rows of edge samples are scaled by 1 + 30

# worst |HIP - float64| / scale over the compared tensors, per (arch, saving forward, walk, GEMM arithmetic): ~3-4x the worst observed
# over all sizes and forms (audio fp32-MFMA forward 5.3e-5 in every walk; its split-operand forward 1.65e-4; 15-octave NeRFace 8.6e-4;
# static 2.6e-5 in f32 products, 2.5e-4 with split-bf16 operands -- a cancelling bias sum at P = 1,023)
FIELD_BOUNDS = {
    ("audio", "f32", "fused", "fp32"): 2e-4, ("audio", "f32", "fused", "bf16x3"): 2e-4,
    ("audio", "f32", "layer", "fp32"): 2e-4, ("audio", "f32", "layer", "bf16x3"): 2e-4,
    ("audio", "x3", "fused", "fp32"): 6e-4, ("audio", "x3", "fused", "bf16x3"): 6e-4,
    ("nerface", "f32", "layer", "fp32"): 3e-3, ("nerface", "f32", "layer", "bf16x3"): 3e-3,
    ("nerface_static", "f32", "layer", "fp32"): 1e-4, ("nerface_static", "f32", "layer", "bf16x3"): 1e-3,
}

# Held to a bound of its own, outside the path's: the NeRFaceModel's single fc_ambient bias.  Its gradient reaches the loss only through
# the 15-octave encoding of w, which multiplies the ~1e-7 round-off of the forward's w by up to 2^14, and it is a sum that cancels.
# Observed 1.6e-2 of scale at P = 17 in both GEMM arithmetics (plain fp32 autograd with its own branches: up to 31 %,
# tests/test_gpu_nerface.py::test_field_backward_seam_vs_autograd).  This bound cannot see one lost sample in this tensor; the other
# tensors of the deformation part can (the sensitivity floor of every case).
ILL_CONDITIONED = {("nerface", "hyper_sheep_mlp.fc_ambient.bias"): 5e-2}


def _paths(arch, fwd):
    """(walk, GEMM arithmetic, form) of the backward runs over one saving forward"""
    if arch != "audio":
        return [("layer", p, "whole") for p in ("fp32", "bf16x3")]
    walks = ("fused", "layer") if fwd == "f32" else ("fused",)
    return [(w, p, f) for w in walks for p in ("fp32", "bf16x3") for f in ("part3", "part2+1")]


def _edge_rows(P):
    """the samples the tails are made of: the last 16, the first and last of every 1,024 block, 128 k for a few k"""
    rows = set(range(max(0, P - 16), P))
    for b in range(0, P, 1024):
        rows |= {b, min(P, b + 1024) - 1}
    rows |= {128 * k for k in (1, 2, 3, 8, 255, 256) if 128 * k < P}
    return sorted(rows)


def _masks(act, arch, P):
    """Which side of zero every hidden unit is on, as the HIP forward saw it: the saved post-activations of a whole-network save
    (sahs::act layout, csrc/sahs_layout.hpp: one dense [P x width] array per layer, array of column c at c * P)."""
    kbx, kba, trl = {"audio": (4, 2, 8), "nerface": (6, 2, 4), "nerface_static": (4, 0, 4)}[arch]
    WH = 16 * kbx
    HH = WH + 6 * 128 + 16
    Tt = HH + 6 * 64 + 32 + 16 * kbx + 16 * kba
    C = Tt + trl * 256 + 256 + 64
    Ss = C + 512
    assert act.shape == (P, Ss + 512)
    flat_act = act.reshape(-1)
    arr = lambda c, w: flat_act[c * P:(c + w) * P].view(P, w)
    masks = {}
    for i in range(6):
        masks["warp.%d" % i] = arr(WH + 128 * i, 128) > 0
        masks["hyper.%d" % i] = arr(HH + 64 * i, 64) > 0
    for i in range(trl):
        masks["trunk.%d" % i] = arr(Tt + 256 * i, 256) > 0
    for i in range(4):
        masks["dir.%d" % i] = arr(C + 128 * i, 128) > 0
        masks["seg.%d" % i] = arr(Ss + 128 * i, 128) > 0
    return masks


def _setup(arch, N, S):
    ops, W = pkg("ops"), pkg("weights")
    gen = torch.Generator(device=DEV).manual_seed(1000 * N + S)
    if arch == "audio":
        sd_np = W.hash_state_dict(0, 2.0, 30.0, hdr=True)
        driving = torch.randn(16, 29, device=DEV, generator=gen)
        near, far, cam = 0.48, 1.08, 0.8
    else:
        sd_np = W.hash_state_dict(0, 8.0, 30.0, model=arch)
        driving = torch.randn(76, device=DEV, generator=gen) * 0.5
        near, far, cam = 0.2, 0.8, 0.5
    flat = torch.from_numpy(W.flatten_state_dict(sd_np, model=arch)).to(DEV)
    pose = torch.from_numpy(np.concatenate([np.eye(3), [[0.0], [0.0], [cam]]], 1).astype(np.float32)).to(DEV)
    frame = ops.fold_conditioning(flat, driving, pose, arch=arch)
    rays = torch.zeros(N, 8, device=DEV)
    rays[:, 2] = cam
    rays[:, 3:6] = torch.randn(N, 3, device=DEV, generator=gen) * 0.15 + torch.tensor([0, 0, -1.0], device=DEV)
    rays[:, 6], rays[:, 7] = near, far
    z = torch.sort(torch.rand(N, S, device=DEV, generator=gen) * (far - near) + near, dim=1).values
    P = N * S
    x6 = torch.cat([rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None], rays[:, None, 3:6].expand(N, S, 3)], -1).reshape(P, 6)
    gain = torch.ones(P, 1, device=DEV)
    gain[_edge_rows(P)] = EDGE_GAIN
    d_raw = (torch.randn(P, 16, device=DEV, generator=gen) * gain).contiguous()
    seam = (torch.randn(P, 8, device=DEV, generator=gen) * torch.tensor([1, 1, 1, 0, 1, 1, 0, 0.0], device=DEV) * gain).contiguous()
    return dict(arch=arch, N=N, S=S, P=P, sd_np=sd_np, flat=flat, frame=frame, rays=rays, z=z, x6=x6, d_raw=d_raw,
                seam=seam if arch == "audio" else None, level=0 if arch == "audio" else 1, off=W.canonical_offsets(arch))


def _forward(c, fwd):
    """the saving forward -> (act, bits); AudioFaceModel: the split evaluation's whole-network save (fp32 MFMAs, or the split-operand
    kernels as a deformation + a radiance launch into one whole-network save); NeRFaceModels: field_forward_save"""
    ops = pkg("ops")
    N, S, arch = c["N"], c["S"], c["arch"]
    if arch != "audio":
        packed = ops.pack_weights(c["flat"], arch=arch)
        _, act = ops.field_forward_save(packed, c["frame"], c["level"], c["rays"], c["z"], arch)
        return act, None
    xw = torch.zeros(N, S, 8, device=DEV)
    bits = ops.alloc_sign_bits(N * S, ops.FIELD_ALL, "audio", DEV)
    if fwd == "f32":
        _, act = ops.field_forward_split_save(ops.pack_weights(c["flat"]), c["frame"], c["level"], ops.FIELD_ALL, c["rays"], xw, z=c["z"], bits=bits)
    else:
        pk = ops.pack_weights(c["flat"], ops.SAHS_BF16X3)
        act = torch.zeros(N * S, int(ops._fn("act_words_part", "audio")[0](ops.FIELD_ALL)), device=DEV)
        ident = torch.arange(S, dtype=torch.int32, device=DEV).repeat(N, 1).contiguous()
        ops.field_forward_split_save(pk, c["frame"], c["level"], ops.FIELD_DEFORM, c["rays"], xw, z=c["z"], precision=ops.SAHS_BF16X3, whole=(act, bits))
        ops.field_forward_split_save(pk, c["frame"], c["level"], ops.FIELD_RADIANCE, c["rays"], xw, src=ident, precision=ops.SAHS_BF16X3, whole=(act, bits))
    torch.cuda.synchronize()
    return act, bits


def _compared(k, level):
    """the parameter tensors the field backward of `level` writes (the other level's net gets nothing; AudioNet is the conditioning
    backward's)"""
    lvl = "coarse" if level == 0 else "fine"
    return not (("nerf_mlps." in k and lvl not in k) or k.startswith("audNet_head"))


def _eager(c, masks, lo, hi, dtype=torch.float64):
    """Autograd of EagerField (float64: the yardstick) on samples [lo, hi), on the HIP forward's side of every kink, with the frame's own
    conditioning vectors as leaves: {tensor: gradient} for the parameters, "driving", "pose36" and (AudioFaceModel) "seam" = d raw-loss /
    d (x', w)."""
    from oracle import torch_eager as TE
    arch, frame = c["arch"], c["frame"]
    sd = {k: torch.from_numpy(v).to(DEV, dtype).requires_grad_(True) for k, v in c["sd_np"].items()}
    drv = frame[0:76].to(dtype).clone().requires_grad_(True)
    p36 = frame[80:116].to(dtype).clone().requires_grad_(True)
    lvl = "coarse" if c["level"] == 0 else "fine"
    seams = []
    for s in range(lo, hi, CHUNK):
        e = min(hi, s + CHUNK)
        field = TE.EagerField(sd, num_coarse=e - s, num_fine=0, arch=arch, masks={k: m[s:e] for k, m in masks.items()})
        taps = {}
        raw = field.forward(lvl, c["x6"][s:e].to(dtype), None, None, driving=drv, pose36=p36, taps=taps)
        loss = (raw * c["d_raw"][s:e].to(dtype)).sum()
        if c["seam"] is not None:
            na = taps["amb"].shape[1]
            sm = c["seam"][s:e].to(dtype)
            loss = loss + (taps["warped"] * sm[:, 0:3]).sum() + (taps["amb"] * sm[:, 4:4 + na]).sum()
            taps["warped"].retain_grad()
            taps["amb"].retain_grad()
        loss.backward()
        if c["seam"] is not None:
            g = torch.zeros(e - s, 8, dtype=dtype, device=DEV)
            g[:, 0:3] = taps["warped"].grad - sm[:, 0:3]
            g[:, 4:4 + na] = taps["amb"].grad - sm[:, 4:4 + na]
            seams.append(g)
        del raw, loss, taps, field
    out = {k: v.grad for k, v in sd.items() if _compared(k, c["level"])}
    out["driving"], out["pose36"] = drv.grad, p36.grad
    if seams:
        out["seam"] = torch.cat(seams)
    return out


def _hip(c, act, bits, walk, prec, form, zero_last):
    ops = pkg("ops")
    d_raw, seam = c["d_raw"], c["seam"]
    if zero_last:       # the negative control: the last sample's upstream rows dropped
        d_raw = d_raw.clone()
        d_raw[-1] = 0.0
        seam = None if seam is None else seam.clone()
        if seam is not None:
            seam[-1] = 0.0
    flat, frame, lv, arch = c["flat"], c["frame"], c["level"], c["arch"]
    gf, gc = torch.zeros_like(flat), torch.zeros(128, device=DEV)
    g_out = None
    try:
        ops.backward_gemm_precision(prec)
        ops.fused_backward(walk == "fused")
        if form == "whole":
            ops.field_backward(flat, frame, lv, act, d_raw, gf, gc, arch)
        elif form == "part3":
            ops.field_backward_split(flat, frame, lv, 3, act, gf, gc, d_raw=d_raw, xw_grad_in=seam, bits=bits)
        else:           # radiance part, then the deformation part from its seam gradient: RenderRaysFn's chain
            g_out = ops.field_backward_split(flat, frame, lv, ops.FIELD_RADIANCE, act, gf, gc, d_raw=d_raw, full_act=True, bits=bits)
            ops.field_backward_split(flat, frame, lv, ops.FIELD_DEFORM, act, gf, gc, xw_grad_in=g_out + seam, full_act=True, bits=bits)
        torch.cuda.synchronize()
    finally:
        ops.backward_gemm_precision("bf16x3")
        ops.fused_backward(True)
    got = {k: gf[o:o + int(np.prod(shape))].view(shape) for k, (o, shape) in c["off"].items() if _compared(k, lv)}
    got["driving"], got["pose36"] = gc[0:76], gc[80:116]
    if g_out is not None:
        got["seam"] = g_out
    return got


def _part(k):
    if k.startswith(("warp_field_mlp", "hyper_sheep_mlp")):
        return "deformation"
    if k.startswith("nerf_mlps") or k == "spatial_embeddings":
        return "radiance"
    return k        # driving / pose36 / seam


def _errors(got, ref):
    """per tensor: max |HIP - float64| / max |float64|; a tensor float64 leaves at zero must be exactly zero"""
    errs = {}
    for k, r in ref.items():
        if k not in got:
            continue
        if got[k] is None and r is None:
            continue
        g = got[k].double()
        if k == "seam":
            g, r = g[:, [0, 1, 2, 4, 5]], r[:, [0, 1, 2, 4, 5]]
        if r is None:
            errs[k] = 0.0 if float(g.abs().max()) == 0.0 else float("inf")
            continue
        sc = float(r.abs().max())
        errs[k] = float((g - r).abs().max()) / sc if sc > 0 else (0.0 if float(g.abs().max()) == 0.0 else float("inf"))
    return errs


def _sensitivity(ref, last):
    """per part: the largest entry of sample P-1's own contribution, relative to the tensor's scale, over the part's tensors"""
    best = {}
    for k, r in ref.items():
        if r is None or last.get(k) is None or k in ("driving", "pose36"):
            continue
        lr = last[k][-1:] if k == "seam" else last[k]
        sc = float(r.abs().max())
        if sc > 0:
            best[_part(k)] = max(best.get(_part(k), 0.0), float(lr.abs().max()) / sc)
    return best


def _field_case(arch, N, S, zero_last=False):
    t0 = time.time()
    c = _setup(arch, N, S)
    P = c["P"]
    failures = []
    for fwd in (("f32", "x3") if arch == "audio" else ("f32",)):
        act, bits = _forward(c, fwd)
        masks = _masks(act, arch, P)
        ref = _eager(c, masks, 0, P)
        last = _eager(c, masks, P - 1, P)
        if "seam" in last:
            last["seam"] = torch.cat([torch.zeros(P - 1, 8, dtype=torch.float64, device=DEV), last["seam"]])
        sens = _sensitivity(ref, last)
        for walk, prec, form in _paths(arch, fwd):
            bound = FIELD_BOUNDS[(arch, fwd, walk, prec)]
            got = _hip(c, act, bits, walk, prec, form, zero_last)
            errs = _errors(got, ref)
            allow = {k: max(bound, ILL_CONDITIONED.get((arch, k), 0.0)) for k in errs}
            over = ["%s %.2e (own bound %.1e)" % (k, errs[k], allow[k]) for k in errs if errs[k] > bound and errs[k] <= allow[k]]
            parts = {_part(k) for k in errs if _part(k) in ("deformation", "radiance")} | ({"seam"} if "seam" in got else set())
            floor = min(sens[p] for p in parts) / 2.0
            top = sorted(errs.items(), key=lambda kv: -kv[1])[:3]
            tag = "%s P=%d (%dx%d) %s-forward %s/%s/%s" % (arch, P, N, S, fwd, walk, prec, form)
            print("%s%s: worst %s  bound %.1e  sensitivity floor %.2e%s" % ("[last sample zeroed] " if zero_last else "", tag,
                  ", ".join("%s %.2e" % kv for kv in top), bound, floor, ("  ill-conditioned: " + ", ".join(over)) if over else ""))
            if zero_last:
                if top[0][1] <= bound:
                    failures.append("%s: the last sample's upstream rows dropped, yet worst %.2e <= bound %.1e" % (tag, top[0][1], bound))
                continue
            if bound > floor:
                failures.append("%s: bound %.1e could not see sample P-1 (half its contribution: %.2e; per part %s)" % (tag, bound, floor, sens))
            if any(errs[k] > allow[k] for k in errs):
                failures.append("%s: %s" % (tag, ", ".join("%s %.3e of scale" % kv for kv in top)))
        del act, bits, masks, ref, last
    torch.cuda.empty_cache()
    print("%s P=%d: %.1f s" % (arch, P, time.time() - t0))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("N,S", SIZES, ids=["P%d" % (n * s) for n, s in SIZES])
@pytest.mark.parametrize("arch", ["audio", "nerface", "nerface_static"])
def test_field_backward_vs_float64(arch, N, S):
    """Every parameter gradient of the level's field, the driving and pose-encoding gradients (grad_cond[0:76], [80:116]) and, for
    the radiance part, the returned seam gradient d (x', w), against float64 autograd of the eager field on the HIP forward's side of
    every kink; upstream gradients weighted towards the tail and block-edge samples."""
    _field_case(arch, N, S)


@pytest.mark.parametrize("arch", ["audio", "nerface", "nerface_static"])
def test_field_backward_negative_control(arch):
    """Each path, with the upstream rows of sample P-1 zeroed, fails the bound it is held to (the bounds can see one lost sample)."""
    _field_case(arch, *NEGATIVE_SIZE, zero_last=True)


# ---------------------------------------------------------------------------------------------------------------------------------
# composite backward (composite_backward_kernel: one wave per ray, S <= 256 in up to 4 blocks of 64 samples)
# ---------------------------------------------------------------------------------------------------------------------------------
COMPOSITE_BOUND = 3e-6      # max |HIP - float64| / scale of d raw (observed: 8.8e-7)
COMPOSITE_S = [1, 2, 63, 64, 65, 128, 129, 192, 193, 256]
COMPOSITE_OPTS = [(True, False, True), (False, True, False), (False, False, True), (True, True, False)]


def _composite_inputs(S, use_bg, noise_on, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    N = 257
    raw = torch.randn(N, S, 16, device=DEV, generator=gen) * 1.5
    raw[..., 15] = raw[..., 15] * 6 + 1.0
    z = torch.sort(torch.rand(N, S, device=DEV, generator=gen) * 0.6 + 0.48, dim=1).values
    rays = torch.zeros(N, 8, device=DEV)
    rays[:, 3:6] = torch.randn(N, 3, device=DEV, generator=gen) * 0.2 + torch.tensor([0, 0, -1.0], device=DEV)
    bg = torch.rand(N, 15, device=DEV, generator=gen) if use_bg else None
    noise = torch.randn(N, S, device=DEV, generator=gen) * 0.1 if noise_on else None
    return gen, N, raw, z, rays, bg, noise


def _render64(raw, z, rays, noise, bg, white):
    from oracle import torch_eager as TE
    x = raw.double().clone().requires_grad_(True)
    xin = x
    if bg is not None:
        xin = torch.cat((x[:, :-1], torch.cat((bg.double(), x[:, -1, -1:]), dim=-1).unsqueeze(1)), dim=1)
    outs = TE.volume_render(xin, z.double(), rays[:, 3:6].double(), None if noise is None else noise.double(), white, bg is not None)
    return x, outs


def _check_composite(d_raw, ref, what):
    assert torch.isfinite(d_raw).all(), what
    scale = float(ref.abs().max())
    if scale == 0.0:      # (S = 1 behind a background prior: the one sample's colour is the prior's, its alpha saturated at 1)
        print("%s: float64 gradient is zero, HIP max |d raw| %.2e" % (what, float(d_raw.abs().max())))
        assert float(d_raw.abs().max()) == 0.0, what
        return
    err = float((d_raw.double() - ref).abs().max()) / scale
    print("%s: %.2e of scale (bound %.1e)" % (what, err, COMPOSITE_BOUND))
    assert err <= COMPOSITE_BOUND, (what, err, scale)


@pytest.mark.parametrize("use_bg,white,noise_on", COMPOSITE_OPTS, ids=["bg-noise", "white", "noise", "bg-white"])
@pytest.mark.parametrize("S", COMPOSITE_S)
def test_composite_backward_vs_float64(S, use_bg, white, noise_on):
    """sahs_composite_backward with every upstream gradient (rgb, disp, acc, depth, weights[:, -1], the whole weights) against float64
    autograd of the eager compositing (volume_rendering_utils.py:7-78)."""
    ops = pkg("ops")
    gen, N, raw, z, rays, bg, noise = _composite_inputs(S, use_bg, noise_on, 7 * S + 2 * use_bg + white)
    gr = [torch.randn(N, 15, device=DEV, generator=gen)] + [torch.randn(N, device=DEV, generator=gen) for _ in range(4)]
    gw = torch.randn(N, S, device=DEV, generator=gen)
    gr[1] = gr[1] * 1e-3
    x, (rgb, disp, acc, w, depth) = _render64(raw, z, rays, noise, bg, white)
    loss = ((rgb * gr[0].double()).sum() + (disp * gr[1].double()).sum() + (acc * gr[2].double()).sum() + (depth * gr[3].double()).sum()
            + (w[:, -1] * gr[4].double()).sum() + (w * gw.double()).sum())
    loss.backward()
    d_raw = ops.composite_backward(raw, z, rays, noise, bg, white, gr[0], gr[1], gr[2], gr[3], gr[4], gw)
    _check_composite(d_raw, x.grad, "composite backward S=%d bg=%d white=%d noise=%d" % (S, use_bg, white, noise_on))


def _loss_inputs(gen, N, target_cols=5):
    cls = torch.randint(0, 12, (N,), device=DEV, generator=gen)
    cls[cls == 5] = 4          # an empty class
    cls[cls == 11] = 10
    cls[N // 2] = 11           # a one-ray class
    mask = torch.nn.functional.one_hot(cls, 12).float()
    target = torch.rand(N, target_cols, device=DEV, generator=gen)       # target_ld > 3: the kernel must read only the first 3 columns
    return target, mask


@pytest.mark.parametrize("use_bg,white,noise_on", COMPOSITE_OPTS[:2], ids=["bg-noise", "white"])
@pytest.mark.parametrize("S", COMPOSITE_S)
def test_composite_backward_loss_form_vs_float64(S, use_bg, white, noise_on):
    """sahs_composite_backward_loss (the Stage-I objective's gradient formed inside the kernel, LossGrad) as RenderRaysFn drives it --
    this level's rendered map, the stats of both levels, d objective / d loss as loss_gscale, other upstream gradients beside it --
    against float64 autograd of gscale * training.stage1_loss + those terms, for either level's place in the objective."""
    ops, Tr = pkg("ops"), pkg("training")
    gen, N, raw, z, rays, bg, noise = _composite_inputs(S, use_bg, noise_on, 11 * S + use_bg)
    target, mask = _loss_inputs(gen, N)
    cw = Tr.sample_prob_weights(DEV)
    other = torch.cat([torch.rand(N, 3, device=DEV, generator=gen), torch.softmax(torch.randn(N, 12, device=DEV, generator=gen) * 2, -1)], 1)
    gr = [torch.randn(N, 15, device=DEV, generator=gen) * 0.1, torch.randn(N, device=DEV, generator=gen) * 1e-4,
          torch.randn(N, device=DEV, generator=gen) * 0.1, torch.randn(N, device=DEV, generator=gen) * 0.1, torch.randn(N, device=DEV, generator=gen) * 0.1]
    gscale = torch.tensor([2.5], device=DEV)
    rgb32 = ops.composite_forward(raw, z, rays, noise=noise, bg=bg, white_background=white)[0].contiguous()
    for this_level in (0, 1):
        maps = (rgb32, other) if this_level == 0 else (other, rgb32)
        st = ops.stage1_loss_forward(maps[0], maps[1], target, mask, cw)
        d_raw = ops.composite_backward(raw, z, rays, noise, bg, white, *gr, loss=(rgb32, target, mask, st, gscale))
        x, (rgb, disp, acc, w, depth) = _render64(raw, z, rays, noise, bg, white)
        m64 = (rgb, other.double()) if this_level == 0 else (other.double(), rgb)
        obj = Tr.stage1_loss(m64[0], m64[1], target.double(), mask.double())[0] * float(gscale)
        loss = (obj + (rgb * gr[0].double()).sum() + (disp * gr[1].double()).sum() + (acc * gr[2].double()).sum()
                + (depth * gr[3].double()).sum() + (w[:, -1] * gr[4].double()).sum())
        loss.backward()
        _check_composite(d_raw, x.grad, "composite backward, loss form, level %d, S=%d bg=%d white=%d" % (this_level, S, use_bg, white))


# ---------------------------------------------------------------------------------------------------------------------------------
# Stage-I loss kernel (one 1,024-thread workgroup: thread t takes rays t, t + 1024, ...)
# ---------------------------------------------------------------------------------------------------------------------------------
LOSS_REL_BOUND = 5e-7       # loss and mse, relative (observed: 1.2e-7)
PROB_BOUND = 1e-7           # sample_prob, absolute (they sum to 1; observed: 2.4e-8)


@pytest.mark.parametrize("both", [True, False], ids=["both-levels", "coarse-only"])
@pytest.mark.parametrize("N", [1, 1023, 1024, 1025, 2048, 4097])
def test_stage1_loss_forward_vs_float64(N, both):
    """Every stats word of sahs_stage1_loss_forward -- loss, the last level's mse, the 12 new sample_prob, the class counts (>= 1), the
    ray count -- against float64 of training.stage1_loss on the same inputs, across the workgroup's stride; an empty and a one-ray
    class, target with 5 columns.  The bound is held below the share of the last ray (a ray the strided loop skipped would fail)."""
    ops, Tr = pkg("ops"), pkg("training")
    gen = torch.Generator(device=DEV).manual_seed(N + 7 * both)
    target, mask = _loss_inputs(gen, N)
    cw = Tr.sample_prob_weights(DEV)
    maps = [torch.cat([torch.rand(N, 3, device=DEV, generator=gen), torch.softmax(torch.randn(N, 12, device=DEV, generator=gen) * 2, -1)], 1)
            for _ in range(2)]
    mc, mf = maps[0], maps[1] if both else None
    st = ops.stage1_loss_forward(mc, mf, target, mask, cw).double()
    d = lambda t: None if t is None else t.double()
    loss, prob, mse = Tr.stage1_loss(d(mc), d(mf), target.double(), mask.double())
    counts = mask.double().sum(0).clamp(min=1.0)
    res = dict(loss=abs(float(st[0]) - float(loss)) / abs(float(loss)), mse=abs(float(st[1]) - float(mse)) / abs(float(mse)),
               prob=float((st[2:14] - prob).abs().max()))
    print("stage-1 loss N=%d %s: %s" % (N, "both levels" if both else "coarse only", ", ".join("%s %.2e" % kv for kv in res.items())))
    assert res["loss"] <= LOSS_REL_BOUND and res["mse"] <= LOSS_REL_BOUND and res["prob"] <= PROB_BOUND, res
    assert torch.equal(st[14:26], counts) and float(st[26]) == N
    assert float(st[14 + 5]) == 1.0 and float(st[14 + 11]) == 1.0      # the empty class counts as 1; the one-ray class is 1
    if N > 1:     # sensitivity: without its last ray the loss moves by more than the bound
        cut = lambda t: None if t is None else t[:-1].double()
        l2 = Tr.stage1_loss(cut(mc), cut(mf), target[:-1].double(), mask[:-1].double())[0]
        assert abs(float(l2) - float(loss)) / abs(float(loss)) > 2 * LOSS_REL_BOUND
