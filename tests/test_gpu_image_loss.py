"""The fused image objective on the GPU (include/sahs_nerf.h: sahs_image_loss; ops.image_loss; spade.RefineLoss) against the float64
references of tests/image_loss_reference.py, at the smallest shapes that can break the kernel: with T the pixel-tile edge, (H, W) =
(7,7), (7,8), (8,7), (13,13), (T,T), (T+1,T), (T,T+1), (T-1,2T+1), (2T+7,T+6) and 45 x 71; C = 1, 3 and 4; the four weightings; clamp on
and off; every image of a shape in one batch.  tests/test_image_loss_reference_host.py shows on the CPU that a dropped gamma term, a
dropped row of window origins at a tile seam, an exclusive clamp mask, sign(0) = 1 and the wrong normalisation each move E by more than 100
times the tolerance used here.

Tolerances.  Gradient: E = max |g - g64| / max(max |g64|, sum |w| / N) per image, and with E_torch the E of torch's fp32 autograd through
its own formulation (avg_pool2d moment planes, raw-moment variances, clamp, mse_loss, l1_loss) on the same GPU and inputs,
E_fused <= max(4 E_torch, 2^-20) -- tests/test_gpu_metrics.py's rule -- and on the flat bright pair E_fused < E_torch wherever SSIM is
weighted.  Loss rows [MSE, L1, SSIM]: that file's fp32 rule as it stands, absolute for SSIM and relative for MSE and L1.  Under MSE alone
the gradient is 2 (x - t) / N with at most three fp32 roundings on either side (the fused op: the float64 quotient rounded once, and the
backward's product with the rounded 1 / B; torch: the difference, the product with 2 / N): within 4 ulp of torch's, with the same zeros.
Every E is printed (pytest -s).

On the flat bright pair the strict E_fused < E_torch is asked wherever SSIM is weighted, which is where centring decides anything.
Under MSE or L1 alone both sides are a closed form with two or three fp32 roundings, and torch's L1 gradient, fl(1 / N), is the
correctly rounded value: no implementation can come out strictly below it (measured there: E_fused 1.2e-8 .. 1.2e-7, E_torch
4.0e-9 .. 1.0e-7, both far below the rule's floor, which does apply).

The refiner-step test holds the gradients of the first and the last convolution weight to tests/test_gpu_spade_backward.py's rule for
two fp32 steps: relative L2 error against the float64 step of tests/spade_reference.py (computed once per session and shared with
that file), G_fused <= 4 G_none with G_none <= 1e-4.

Measured on an MI355X: worst E_fused 1.3e-7 (0.14 of its bound) over every shape, channel count, weighting, clamp and content, worst
E_torch 6.8e-4; flat bright with SSIM weighted E_fused <= 1.1e-7 against E_torch 2.7e-5 .. 6.8e-4; rows within 4.5e-16 (MSE, relative),
0 (L1) and 2.2e-16 (SSIM) of float64; MSE alone within 3 ulp of torch's gradient; refine_step loss=None 0.267020077, RefineLoss(l2=1)
0.267020047, G_fused 5.9e-6 / 1.3e-6 against G_none 5.9e-6 / 1.3e-6; RefineLoss(1, 1, 1) 1.677 -> 0.564 in five steps.  Wall time: the
accuracy cases 0.06 .. 1.1 s each (the first pays the start-up), the refiner step 7 s cold with the shared float64 step, the rest
under 0.3 s.
"""
import copy
import functools

import numpy as np
import pytest
import torch

import image_loss_reference as R
import metrics_reference as M
from conftest import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = R.TILE
SHAPES = R.gpu_shapes()


@functools.lru_cache(maxsize=None)
def cases(H, W, C):
    """-> names, pred (N, H, W, C), target, {clamp: (terms (N, 3), grads (N, 3, H, W, C))} in float64, computed once per shape."""
    items = R.inputs(H, W, C)
    refs = {}
    for clamp in (True, False):
        both = [R.closed_terms(p, t, clamp) for _, p, t in items]
        refs[clamp] = np.stack([a for a, _ in both]), np.stack([b for _, b in both])
    return [n for n, _, _ in items], np.stack([p for _, p, _ in items]), np.stack([t for _, _, t in items]), refs


def nchw(a):
    return torch.from_numpy(a).to(DEV).permute(0, 3, 1, 2).contiguous()


def fused(pred, target, w, clamp=True, channels_last=False, rng=1.0):
    """ops.image_loss with a gradient -> loss (0-d), rows (B, 3), the gradient in pred's own layout."""
    pred = pred.detach().requires_grad_(True)
    loss, rows = pkg("ops").image_loss(pred, target, *w, clamp=clamp, ssim_data_range=rng, channels_last=channels_last, return_terms=True)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and rows.dtype == torch.float64 and not rows.requires_grad
    loss.backward()
    assert pred.grad.shape == pred.shape
    return loss.detach(), rows, pred.grad


def hwc(g):
    return g.permute(0, 2, 3, 1).double().cpu().numpy()


def rel(got, ref):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ref == 0, np.where(got == 0, 0.0, np.inf), np.abs(got - ref) / np.abs(ref))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_gradient_and_terms_against_float64(shape):
    for C in (1, 3, 4):
        names, pred, target, refs = cases(*shape, C)
        B = len(names)
        tp, tt = nchw(pred), nchw(target)
        for clamp in (True, False):
            terms64, grads64 = refs[clamp]
            x = tp.clamp(0, 1) if clamp else tp
            rows_torch = M.torch_formulation(x, tt).double().cpu().numpy()[:, [1, 2, 0]]      # -> [MSE, L1, SSIM]
            want_rows = np.stack([terms64[:, 0], terms64[:, 1], 1.0 - terms64[:, 2]], axis=1)
            for w in R.WEIGHTS:
                loss, rows, g = fused(tp, tt, w, clamp)
                leaf = tp.detach().requires_grad_(True)
                R.torch_composition(leaf, tt, w, clamp).backward()
                g, g_torch, rows = hwc(g), hwc(leaf.grad), rows.cpu().numpy()
                for k, name in enumerate(names):
                    g64 = R.combine(terms64[k], grads64[k], w)[1] / B
                    e, e_torch = R.grad_error(g[k], g64, w, B), R.grad_error(g_torch[k], g64, w, B)
                    print("%s C=%d clamp=%d w=%s %-15s E_fused %.2e  E_torch %.2e" % (shape, C, clamp, w, name, e, e_torch))
                    assert e <= max(4.0 * e_torch, R.FLOOR), (shape, C, clamp, w, name, e, e_torch)
                    if name == "flat_bright" and w[2] != 0.0:
                        assert e < e_torch, (shape, C, clamp, w, "the shifted frame no better than raw moments", e, e_torch)
                # the loss terms: test_gpu_metrics.py's fp32 rule, and the loss is the weighted mean of the rows, rounded once
                e_rows = np.stack([rel(rows[:, 0], want_rows[:, 0]), rel(rows[:, 1], want_rows[:, 1]), np.abs(rows[:, 2] - want_rows[:, 2])])
                e_rows_torch = np.stack([rel(rows_torch[:, 0], want_rows[:, 0]), rel(rows_torch[:, 1], want_rows[:, 1]), np.abs(rows_torch[:, 2] - want_rows[:, 2])])
                for k, name in enumerate(names):
                    assert np.all(e_rows[:, k] <= np.maximum(4.0 * e_rows_torch[:, k], R.FLOOR)), (shape, C, clamp, name, e_rows[:, k], e_rows_torch[:, k])
                    if name == "flat_bright":
                        assert e_rows[2, k] < e_rows_torch[2, k], (shape, C, clamp, e_rows[2, k], e_rows_torch[2, k])
                m = [rows[:, j].cumsum()[-1] / B for j in range(3)]      # (the finalize step's order: image by image)
                assert float(loss) == np.float32(w[0] * m[0] + w[1] * m[1] + w[2] * (1.0 - m[2])), (shape, C, clamp, w)
            print("%s C=%d clamp=%d rows: MSE rel %.2e  L1 rel %.2e  SSIM %.2e" % (shape, C, clamp, *e_rows.max(1)))


@pytest.mark.parametrize("shape", [(13, 13), (T - 1, 2 * T + 1), (45, 71)], ids=lambda s: "%dx%d" % s)
def test_exact_zeros_and_the_clamps_ends(shape):
    for C in (1, 3, 4):
        names, pred, target, _ = cases(*shape, C)
        tp, tt = nchw(pred), nchw(target)
        outside = (pred < 0) | (pred > 1)
        for w in R.WEIGHTS:
            _, _, g = fused(tp, tt, w, True)
            g = g.permute(0, 2, 3, 1).cpu().numpy()
            assert outside.any() and not g[outside].any(), (shape, C, w)
            k = names.index("planted_edges")
            for flat, _ in R.PLANTED_EDGES:
                assert g[k].reshape(-1)[flat] != 0.0, (shape, C, w, flat)
        _, _, g = fused(tp, tt, (1.0, 0.0, 0.0), True)
        assert not g[names.index("identical_exact")].any()
        _, _, g = fused(tp, tt, (0.0, 1.0, 0.0), True)      # L1's derivative at x == t is 0: only the mean's share of the weight elsewhere
        k, g = names.index("planted_equal"), g.permute(0, 2, 3, 1).cpu().numpy()
        for flat in R.PLANTED_EQUAL:
            assert g[k].reshape(-1)[flat] == 0.0
        inside = ~outside[k]
        inside.reshape(-1)[list(R.PLANTED_EQUAL)] = False
        assert np.all(np.abs(g[k][inside]) == np.float32(np.float32(1.0 / pred[k].size) * np.float32(1.0 / len(names))))


@pytest.mark.parametrize("shape", [(7, 8), (T + 1, T), (45, 71)], ids=lambda s: "%dx%d" % s)
def test_mse_alone_is_torchs_gradient_within_4_ulp(shape):
    for C in (1, 3, 4):
        _, pred, target, _ = cases(*shape, C)
        tp, tt = nchw(pred), nchw(target)
        loss, _, g = fused(tp, tt, (1.0, 0.0, 0.0), True)
        leaf = tp.detach().requires_grad_(True)
        want = torch.nn.functional.mse_loss(leaf.clamp(0, 1), tt)
        want.backward()
        assert abs(float(loss) - float(want.detach())) <= 1e-6 * float(want.detach())
        assert torch.equal(g == 0, leaf.grad == 0)
        got, ref = g.cpu().numpy(), leaf.grad.cpu().numpy()
        worst = float((np.abs(got.astype(np.float64) - ref) / np.spacing(np.abs(ref))).max())
        print("%s C=%d: MSE gradient within %.1f ulp of torch's" % (shape, C, worst))
        assert worst <= 4.0


def test_layouts_give_the_same_bits():
    """(B, C, H, W), (B, H, W, C), a cropped view of a larger tensor (pred and target with different strides), and a single (C, H, W)."""
    H, W, C = 45, 71, 3
    _, pred, target, _ = cases(H, W, C)
    w = R.WEIGHTS[3]
    loss, rows, g = fused(nchw(pred), nchw(target), w)
    g = g.permute(0, 2, 3, 1)
    loss_l, rows_l, g_l = fused(torch.from_numpy(pred).to(DEV), torch.from_numpy(target).to(DEV), w, channels_last=True)
    assert torch.equal(loss, loss_l) and torch.equal(rows.view(torch.int64), rows_l.view(torch.int64)) and torch.equal(g, g_l)
    big = torch.full((len(pred), H + 5, W + 9, C), 77.0, device=DEV)      # (anything read outside the crop shows in every figure)
    big[:, 2:2 + H, 3:3 + W] = torch.from_numpy(pred).to(DEV)
    view = big[:, 2:2 + H, 3:3 + W]
    assert not view.is_contiguous() and view.stride(1) > W * C
    loss_v, rows_v, g_v = fused(view, torch.from_numpy(target).to(DEV), w, channels_last=True)
    assert torch.equal(loss, loss_v) and torch.equal(rows.view(torch.int64), rows_v.view(torch.int64)) and torch.equal(g, g_v)
    # the gradient of a view lands in the view's elements of its base, and nowhere else
    base = big.clone().requires_grad_(True)
    pkg("ops").image_loss(base[:, 2:2 + H, 3:3 + W], torch.from_numpy(target).to(DEV), *w, channels_last=True).backward()
    assert torch.equal(base.grad[:, 2:2 + H, 3:3 + W], g)
    base.grad[:, 2:2 + H, 3:3 + W] = 0
    assert not base.grad.any()
    single = nchw(pred)[2].detach().requires_grad_(True)      # no batch dimension
    loss_s, rows_s = pkg("ops").image_loss(single, nchw(target)[2], *w, return_terms=True)
    loss_s.backward()
    assert rows_s.shape == (1, 3) and single.grad.shape == (C, H, W)


def test_batch_gives_the_bits_of_its_single_calls_and_runs_repeat():
    ops = pkg("ops")
    _, pred, target, _ = cases(T - 1, 2 * T + 1, 3)
    tp, tt = nchw(pred)[:3].contiguous(), nchw(target)[:3].contiguous()
    for w in (R.WEIGHTS[3], R.WEIGHTS[2]):
        loss, rows, g = fused(tp, tt, w)
        again = fused(tp, tt, w)
        assert torch.equal(loss, again[0]) and torch.equal(rows.view(torch.int64), again[1].view(torch.int64)) and torch.equal(g, again[2])
        # the three single calls, averaged the way the batch is: each backward scales its gradient image by 1 / 3
        leaves = [tp[i:i + 1].detach().requires_grad_(True) for i in range(3)]
        singles = [ops.image_loss(leaf, tt[i:i + 1], *w, return_terms=True) for i, leaf in enumerate(leaves)]
        ((singles[0][0] + singles[1][0] + singles[2][0]) / 3).backward()
        assert torch.equal(torch.cat([r for _, r in singles]).view(torch.int64), rows.view(torch.int64))
        assert torch.equal(torch.cat([leaf.grad for leaf in leaves]), g)
        # B = 1: the batch row is the image's row, and the loss its weighted sum
        r = singles[0][1][0].cpu().numpy()
        assert float(singles[0][0].detach()) == np.float32(w[0] * r[0] + w[1] * r[1] + w[2] * (1.0 - r[2]))


def test_incoming_gradient_scales_and_no_grad_returns_the_same_bits():
    ops = pkg("ops")
    _, pred, target, _ = cases(T + 1, T, 3)
    tp, tt = nchw(pred), nchw(target)
    w = R.WEIGHTS[3]
    for n in (1, 4):      # (1 / B a power of two: the backward's one product is the only rounding after the gradient image's own)
        _, _, g = fused(tp[:n], tt[:n], w)
        leaf = tp[:n].detach().requires_grad_(True)
        (ops.image_loss(leaf, tt[:n], *w) * 2.5).backward()
        assert torch.equal(leaf.grad, (g.double() * 2.5).float()), n      # 2.5 x the gradient, rounded once
    loss, rows, g = fused(tp, tt, w)
    plain = ops.image_loss(tp, tt, *w, return_terms=True)      # pred asks for no gradient
    assert plain[0].grad_fn is None and torch.equal(plain[0], loss) and torch.equal(plain[1].view(torch.int64), rows.view(torch.int64))
    with torch.no_grad():
        held = ops.image_loss(tp.detach().requires_grad_(True), tt, *w, return_terms=True)
    assert held[0].grad_fn is None and torch.equal(held[0], loss) and torch.equal(held[1].view(torch.int64), rows.view(torch.int64))
    with torch.autocast("cuda", dtype=torch.bfloat16):      # the op runs outside autocast
        cast = ops.image_loss(tp, tt, *w)
    assert cast.dtype == torch.float32 and torch.equal(cast, loss)


def test_refusals_by_name():
    ops, lib = pkg("ops"), pkg("_lib")
    f = torch.rand(2, 3, 9, 9, device=DEV)
    for match, call in (("target requires a gradient", lambda: ops.image_loss(f, f.clone().requires_grad_(True))),
                        ("pred must be torch.float32", lambda: ops.image_loss(f.bfloat16(), f)),
                        ("target must be torch.float32", lambda: ops.image_loss(f, f.double())),
                        ("pred must be torch.float32", lambda: ops.image_loss((f * 255).to(torch.uint8), f)),
                        ("target must be a GPU tensor", lambda: ops.image_loss(f, f.cpu())),
                        ("pred must be a GPU tensor", lambda: ops.image_loss(f.cpu(), f)),
                        ("pred and target must have one shape", lambda: ops.image_loss(f, f[:, :, :8])),
                        ("pred and target must have one shape", lambda: ops.image_loss(f[0, 0], f[0, 0])),
                        ("H, W >= 7", lambda: ops.image_loss(f[:, :, :6], f[:, :, :6])),
                        ("H, W >= 7", lambda: ops.image_loss(f[:, :, :, :6], f[:, :, :, :6])),
                        ("C = 5 channels", lambda: ops.image_loss(torch.zeros(1, 5, 9, 9, device=DEV), torch.zeros(1, 5, 9, 9, device=DEV))),
                        ("C = 9 channels", lambda: ops.image_loss(f.new_zeros(1, 9, 9, 9), f.new_zeros(1, 9, 9, 9), channels_last=True)),
                        ("must be finite", lambda: ops.image_loss(f, f, l1=float("nan"))),
                        ("ssim_data_range = 0", lambda: ops.image_loss(f, f, ssim_data_range=0.0))):
        with pytest.raises(lib.SahsError, match=match):
            call()


def _conv_weights(G):
    names = [k for k, p in G.named_parameters() if p.dim() == 4]
    return names[0], names[-1]


def test_refine_step_with_the_fused_mse_is_the_step():
    """refine_step(loss=RefineLoss(l2=1)) against refine_step(loss=None) on two copies of the seeded Generator, on the fixture's inputs
    (the size tests/test_gpu_spade_backward.py steps at).  That file's rule for two fp32 steps that differ in one op: the global relative
    L2 error against the float64 yardstick, G <= 4 G_other, with G_other <= 1e-4 -- here over the first and the last convolution weight."""
    import spade_reference as SR
    S = pkg("spade")
    G = SR.seeded("generator").to(DEV)
    twin = copy.deepcopy(G)
    inputs = SR.step_inputs("generator", DEV)[:3]
    adam = lambda m: torch.optim.Adam(m.parameters(), lr=2e-4, betas=(0.5, 0.999))      # noqa: E731
    loss_none = float(S.refine_step(twin, adam(twin), *inputs))
    loss_fused = float(S.refine_step(G, adam(G), *inputs, loss=S.RefineLoss(l2=1.0)))
    print("refine_step: loss=None %.9g  RefineLoss(l2=1) %.9g" % (loss_none, loss_fused))
    assert abs(loss_fused - loss_none) <= 1e-6 * loss_none
    grads64 = SR.cpu_step("generator")["grads64"]
    first, last = _conv_weights(G)
    assert first != last and first in grads64 and last in grads64
    for k in (first, last):
        ref = {k: grads64[k]}
        g_fused = SR.global_rel_l2({k: dict(G.named_parameters())[k].grad}, ref)
        g_none = SR.global_rel_l2({k: dict(twin.named_parameters())[k].grad}, ref)
        print("  %s: G_fused %.3e  G_none %.3e" % (k, g_fused, g_none))
        assert g_none <= 1e-4 and g_fused <= 4.0 * g_none, (k, g_fused, g_none)


def test_refine_loss_trains():
    import spade_reference as SR
    S = pkg("spade")
    G = SR.seeded("generator").to(DEV)
    inputs = SR.step_inputs("generator", DEV)[:3]
    opt = torch.optim.Adam(G.parameters(), lr=2e-4, betas=(0.5, 0.999))
    loss = S.RefineLoss(1, 1, 1)
    steps = [float(S.refine_step(G, opt, *inputs, loss=loss)) for _ in range(6)]      # (a step returns the loss BEFORE its update)
    print("RefineLoss(1, 1, 1): the loss before each of six steps %s" % " ".join("%.6f" % s for s in steps))
    assert steps[5] < steps[0]
    fake = inputs[0].bfloat16().requires_grad_(True)      # what the generator hands over under autocast: widened first, the gradient comes back in bf16
    with torch.autocast("cuda", dtype=torch.bfloat16):
        cast = loss(fake, inputs[2])
    cast.backward()
    want = pkg("ops").image_loss(fake.detach().float(), inputs[2], 1.0, 1.0, 1.0)
    assert cast.dtype == torch.float32 and torch.equal(cast.detach(), want) and fake.grad.dtype == torch.bfloat16 and bool(fake.grad.any())
