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

from backward_reference import DEV, EDGE_GAIN, FIELD_BOUNDS, ILL_CONDITIONED, _edge_rows, _eager, _errors, _forward, _hip, _masks, _part, _paths
from conftest import pkg

pytestmark = pytest.mark.gpu

# P = N x S on every edge of the walks: one sample; < one f32 wave's 16 (one partial K-step); around a split-operand wave's 32; one
# 128-sample chain tile + 1; either side of the 1,024-sample range floor; the first fp32 item plan with more than one range per unit;
# 256 chain tiles + 1 (a persistent workgroup's second round holds one sample); training-step size, ragged ranges everywhere
SIZES = [(1, 1), (17, 1), (3, 11), (3, 43), (31, 33), (25, 41), (683, 3), (331, 99), (1043, 191)]
NEGATIVE_SIZE = (25, 41)


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
