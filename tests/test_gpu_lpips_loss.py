"""LPIPS as a training term on the GPU (include/sahs_nerf.h: sahs_lpips_prepare_loss, sahs_lpips_prepare_grad, sahs_lpips_head_forward,
sahs_lpips_head_backward; ops.lpips_prepare_loss, ops.lpips_head; metrics.LPIPS.loss; spade.RefineLoss(lpips=...)) against the float64
references of tests/lpips_grad_reference.py, which tests/test_lpips_grad_reference_host.py holds to autograd and to a central difference.

Head gradient, on synthetic fp32 features against the closed form in float64 on the same values: layer pixel counts 1, 3, 49, T - 16, T,
T + 16 (T = 256), C = 5 (the 4-unrolled loop's tail), 64 and 384, B = 2, a non-uniform upstream gradient, pixels that are all zero in one
operand or both.  Rule, per element: |got - ref| <= 2^-23 |ref| + 2^-40 m, m the pixel's largest |ref| (lpips_grad_reference.head_rule),
and finite everywhere.  All five layers of mixed sizes in one call; equal operands: rows == 0 and a gradient with no non-zero element;
the same bits on a second call, a batch the bits of its single calls, rows the bits of ops.lpips_distance.

Prepare backward: bit-equal to torch autograd of the one-operation-per-step formula (clamp, 2x - 1, (x - shift) / scale with tensor
divisors) at 31 x 31 and 45 x 71, for NCHW, NHWC and a cropped view, with pred values exactly 0, exactly 1, out of range and NaN.

Whole chain (LPIPS.from_seed(0), the fp32 pairs of lpips_reference.content as one batch, 31 x 31 and 45 x 71, both ``normalize``): the
loss against the float64 chain by E <= max(4 E_torch, 2^-20); the gradient per image by E = ||g - g64|| / ||g64||, E_fused <= 4 E_torch,
E_torch being torch's fp32 autograd of the same objective (the safe-sqrt head) through the same convolutions on the same GPU.  The
identical pair gives loss == 0 and an all-zero gradient.  With every bias replaced by -(|b| + 1) the features have all-zero pixels: the
torch composition of the published head then has NaN in its gradient (at the feature maps; the ReLUs behind them mask it on the way
to the image: test_dead_pixels_in_the_real_chain), the fused one is finite and within the same rule.
Every E is printed (pytest -s).

Measured on an MI355X: head gradient worst 0.499 of its rule over every pixel count, C and layer list (one fp32 rounding is 0.5).
Whole chain, gradient: worst E_fused 6.6e-6 against E_torch 6.6e-6 for the textured, noisy and constant pairs (E_fused / E_torch between
0.99 and 1.02: both are the convolutions' error, the head's own being float64's); the one-pixel pair 3.1e-4 .. 4.3e-3 against 3.1e-4 ..
4.3e-3 at gradient norms 6e-8 .. 2.5e-6; the identical pair exactly 0 for both.  Loss: E_fused 5e-9 .. 3.1e-7 (the one-pixel pair 1.8e-5
.. 1.9e-4, E_torch 2.1e-5 .. 2.0e-4).  Dead pixels: the GPU's features have 100, 12, 1, 3, 3 of them, as float64 has; 6400, 2304, 384,
768, 768 NaN elements in the torch head's feature gradients, none in the fused head's; gradient E_fused 1.19e-6 against E_torch 1.18e-6.
RefineLoss(l2=1, lpips=1): 0.2797 -> 0.0734 over six steps.  Wall time: 5.1 s for the refiner step (seven steps and a twin), 3.6 s for
the first whole-chain case (it pays the vendor library's start-up), under 0.8 s for every other case.
"""
import copy
import functools

import numpy as np
import pytest
import torch

import lpips_grad_reference as G
import lpips_reference as R
from conftest import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = R.TILE
HEAD_TOL = 1e-12      # tests/test_gpu_lpips.py: the forward head's rule, |fused - ref| <= 1e-12 * sum_l max_c w_lc
PIXELS = [(1, 1), (1, 3), (7, 7), (15, 16), (16, 16), (16, 17)]
assert [h * w for h, w in PIXELS] == [1, 3, 49, T - 16, T, T + 16]
UPSTREAM = np.array([0.7, -1.3, 0.4], np.float32)      # widened exactly by the kernel


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


@functools.lru_cache(maxsize=None)
def head_case(B, C, h, w, seed):
    """-> (fa, fb, weights, closed-form gradient under UPSTREAM[:B], float64 d per image), computed once."""
    fa, fb, lw = G.head_case(B, C, h, w, seed)
    return fa, fb, lw, G.closed_head_grad(fa, fb, lw, UPSTREAM[:B].astype(np.float64)), R.head_rows([np.concatenate([fa, fb])], [lw])[:, 1]


def fused_head(fas, fbs, lws, upstream=UPSTREAM):
    """ops.lpips_head with a backward under ``upstream`` -> (per_image, rows, [gradient per layer])."""
    leaves = [dev(f).requires_grad_(True) for f in fas]
    per_image, rows = pkg("ops").lpips_head(leaves, [dev(f) for f in fbs], [dev(w) for w in lws])
    B = fas[0].shape[0]
    assert per_image.shape == (B,) and per_image.dtype == torch.float32 and per_image.requires_grad
    assert rows.shape == (B, 6) and rows.dtype == torch.float64 and not rows.requires_grad
    assert torch.equal(per_image.detach(), rows[:, 0].float())
    (per_image * dev(np.asarray(upstream)[:B])).sum().backward()
    assert all(leaf.grad.shape == leaf.shape and leaf.grad.dtype == torch.float32 and leaf.grad.is_contiguous() for leaf in leaves)
    return per_image.detach(), rows, [leaf.grad for leaf in leaves]


@pytest.mark.parametrize("C", [5, 64, 384])
@pytest.mark.parametrize("hw", PIXELS, ids=lambda s: "%dx%d" % s)
def test_head_gradient_against_the_closed_form(hw, C):
    fa, fb, lw, ref, d = head_case(2, C, *hw, 40)
    dead_a, dead_b = G.dead_pixels(fa), G.dead_pixels(fb)
    assert dead_a.any() and (hw == (1, 1) or (dead_a & ~dead_b).any()) and G.separation(fa, fb) >= 2.0 ** -10
    _, rows, (got,) = fused_head([fa], [fb], [lw])
    got = got.cpu().numpy()
    worst = G.head_rule(got, ref)
    print("head gradient %s C=%d: worst error %.3f of the rule, largest |g| %.3e, %d dead pixels" % (hw, C, worst, np.abs(ref).max(), dead_a.sum()))
    assert np.all(np.isfinite(got)) and worst <= 1.0, (hw, C, worst)
    assert np.abs(rows.cpu().numpy()[:, 1] - d).max() <= HEAD_TOL * float(lw.max())


def test_head_all_five_layers_mixed_sizes():
    shapes = [(64, 7, 9), (192, 16, 17), (384, 1, 1), (256, 31, 31), (5, 1, 3)]
    cases = [head_case(3, C, h, w, 50 + l) for l, (C, h, w) in enumerate(shapes)]
    fas, fbs, lws = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    _, rows, grads = fused_head(fas, fbs, lws)
    for l, (got, case) in enumerate(zip(grads, cases)):      # LPIPS is the sum of the layers: each layer's upstream gradient is the image's
        worst = G.head_rule(got.cpu().numpy(), case[3])
        print("five layers, layer %d %s: worst error %.3f of the rule" % (l, shapes[l], worst))
        assert worst <= 1.0, (l, worst)
    ref = R.head_rows([np.concatenate([a, b]) for a, b in zip(fas, fbs)], lws)
    assert np.abs(rows.cpu().numpy() - ref).max() <= HEAD_TOL * sum(float(w.max()) for w in lws)
    # fewer layers: the layers given keep their bits
    _, part, part_grads = fused_head(fas[1:4], fbs[1:4], lws[1:4])
    assert torch.equal(bits(part[:, 1:4]), bits(rows[:, 2:5])) and not part[:, 4:].any()
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(part_grads, grads[1:4]))


def test_equal_operands_give_zero_rows_and_a_zero_gradient():
    shapes = [(384, 16, 17), (64, 7, 7), (5, 1, 3)]
    fas = [head_case(3, C, h, w, 60 + l)[0] for l, (C, h, w) in enumerate(shapes)]
    lws = [head_case(3, C, h, w, 60 + l)[2] for l, (C, h, w) in enumerate(shapes)]
    assert all(G.dead_pixels(f).any() for f in fas)
    per_image, rows, grads = fused_head(fas, [f.copy() for f in fas], lws)
    assert not rows.any() and not per_image.any() and not any(bool(g.any()) for g in grads)


def test_same_bits_every_call_batch_equals_singles_and_the_scaling():
    ops = pkg("ops")
    shapes = [(64, 16, 17), (384, 31, 31), (256, 1, 1)]
    cases = [head_case(3, C, h, w, 70 + l) for l, (C, h, w) in enumerate(shapes)]
    fas, fbs, lws = [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]
    per_image, rows, grads = fused_head(fas, fbs, lws)
    again = fused_head(fas, fbs, lws)
    assert torch.equal(bits(rows), bits(again[1])) and all(torch.equal(bits(a), bits(b)) for a, b in zip(grads, again[2]))
    for i in range(3):
        _, r, g = fused_head([f[i:i + 1] for f in fas], [f[i:i + 1] for f in fbs], lws, UPSTREAM[i:i + 1])
        assert torch.equal(bits(r), bits(rows[i:i + 1])) and all(torch.equal(bits(a), bits(b[i:i + 1])) for a, b in zip(g, grads))
    # without a gradient (no_grad, or no fa that asks for one) the statistics are skipped and the rows are the same bits; they are
    # ops.lpips_distance's bits on the concatenated operands
    tensors = [dev(f) for f in fas], [dev(f) for f in fbs], [dev(w) for w in lws]
    plain = ops.lpips_head(*tensors)
    with torch.no_grad():
        quiet = ops.lpips_head([t.clone().requires_grad_(True) for t in tensors[0]], tensors[1], tensors[2])
    old = ops.lpips_distance([torch.cat([a, b]) for a, b in zip(tensors[0], tensors[1])], tensors[2])
    for per, r in (plain, quiet):
        assert not per.requires_grad and torch.equal(bits(r), bits(rows)) and torch.equal(bits(r), bits(old)) and torch.equal(per, per_image)
    # an upstream gradient scaled by 3 scales the gradient as the formula says: the closed form under 3 g, by the same rule
    _, _, tripled = fused_head(fas, fbs, lws, UPSTREAM * np.float32(3.0))
    for l, (got, case) in enumerate(zip(tripled, cases)):
        ref = G.closed_head_grad(case[0], case[1], case[2], (UPSTREAM * np.float32(3.0)).astype(np.float64))
        assert G.head_rule(got.cpu().numpy(), ref) <= 1.0, l
    # the C entry takes the upstream gradient as doubles too (autograd hands this node float32, per_image's dtype): the same bits
    import ctypes
    _, stats = ops._lpips_head_forward(*tensors, True)
    n, pa, pb, pw, Cs, hw, B = ops._lpips_head_tables(*tensors)
    out = [torch.full_like(t, 7.0) for t in tensors[0]]
    pg, g64 = (ctypes.c_void_p * n)(*[t.data_ptr() for t in out]), dev(UPSTREAM.astype(np.float64))
    code = pkg("_lib").lib().sahs_lpips_head_backward(n, pa, pb, pw, Cs, hw, B, ctypes.c_void_p(g64.data_ptr()), 1, ctypes.c_void_p(stats.data_ptr()),
                                                      stats.numel() * 8, pg, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert code == 0 and all(torch.equal(bits(a), bits(b)) for a, b in zip(out, grads))


def prepare_inputs(H, W, seed=7):
    """-> pred (B, H, W, 3) float32 with values below 0, above 1, exactly 0 (and -0), exactly 1 and NaN planted; target; upstream weights."""
    rng = np.random.default_rng(seed)
    pred = rng.uniform(-0.3, 1.3, (3, H, W, 3)).astype(np.float32)
    flat = pred.reshape(-1)
    for k, v in ((5, 0.0), (11, 1.0), (17, -0.0), (23, np.nan), (H * W * 3 + 2, 1.0), (2 * H * W * 3 - 1, np.nan), (3 * H * W * 3 - 1, 0.0)):
        flat[k] = v
    target = rng.uniform(0.0, 1.0, (3, H, W, 3)).astype(np.float32)
    return pred, target, rng.normal(0.0, 1.0, (3, 3, H, W)).astype(np.float32)


@pytest.mark.parametrize("shape", [(31, 31), (45, 71)], ids=lambda s: "%dx%d" % s)
def test_prepare_backward_is_torch_autograd_of_the_formula(shape):
    ops = pkg("ops")
    H, W = shape
    pred, target, weight = prepare_inputs(H, W)
    assert np.isnan(pred).sum() == 2 and (pred == 0).sum() >= 3 and (pred == 1).sum() >= 2 and (pred < 0).any() and (pred > 1).any()
    wt, t_nhwc = dev(weight), dev(target)
    t_nchw = t_nhwc.permute(0, 3, 1, 2).contiguous()
    for normalize in (False, True):
        for clamp in (True, False):
            p = dev(pred).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
            want_x, want_t = G.scaling_steps(p, t_nchw, normalize, clamp)
            (want_x * wt).sum().backward()
            want = p.grad
            assert bool(((want == 0).sum() > 0) == clamp)

            def run(leaf, view, target, channels_last):
                x_pred, x_target = ops.lpips_prepare_loss(view, target, clamp=clamp, normalize=normalize, channels_last=channels_last)
                assert x_pred.shape == x_target.shape == (3, 3, H, W) and x_pred.is_contiguous() and x_target.is_contiguous()
                assert x_pred.requires_grad and not x_target.requires_grad and x_pred.dtype == torch.float32
                assert x_pred.data_ptr() + x_pred.numel() * 4 == x_target.data_ptr()      # two views of the one buffer
                assert torch.equal(x_pred.detach().nan_to_num(7.0), want_x.detach().nan_to_num(7.0)) and torch.equal(x_target, want_t)
                (x_pred * wt).sum().backward()
                return leaf.grad

            nchw = dev(pred).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
            g = run(nchw, nchw, t_nchw, False)
            assert g.is_contiguous() and torch.equal(g, want) and not g.isnan().any()
            nhwc = dev(pred).requires_grad_(True)
            assert torch.equal(run(nhwc, nhwc, t_nhwc, True).permute(0, 3, 1, 2), want)
            base = torch.full((3, 3, H + 5, W + 9), 0.5, device=DEV)      # a cropped view: the gradient lands in its elements only
            base[:, :, 2:2 + H, 3:3 + W] = nchw.detach()
            base.requires_grad_(True)
            g = run(base, base[:, :, 2:2 + H, 3:3 + W], t_nchw, False)
            assert torch.equal(g[:, :, 2:2 + H, 3:3 + W], want)
            g[:, :, 2:2 + H, 3:3 + W] = 0
            assert not g.any()
    # a uint8 target is taken as x / 255, as ops.lpips_prepare takes it; without a gradient the same bits, no autograd node
    u8 = (t_nhwc * 255).to(torch.uint8)
    with torch.no_grad():
        x_pred, x_target = ops.lpips_prepare_loss(dev(pred), u8, clamp=False, channels_last=True)
    assert torch.equal(x_target, ops.lpips_prepare(u8, u8)[3:]) and not x_pred.requires_grad
    assert torch.equal(x_pred.nan_to_num(7.0), ops.lpips_prepare(dev(pred), t_nhwc)[:3].nan_to_num(7.0))
    single = dev(pred)[0].permute(2, 0, 1).contiguous().requires_grad_(True)      # no batch dimension
    ops.lpips_prepare_loss(single, t_nchw[0])[0].nan_to_num(0.0).sum().backward()
    assert single.grad.shape == (3, H, W)


def nchw(a):
    return dev(a).permute(0, 3, 1, 2).contiguous()


def hwc(g):
    return g.permute(0, 2, 3, 1).double().cpu().numpy()


class deterministic_convolutions:
    """The vendor library's deterministic mode, for a backward(): metrics.LPIPS.loss sets it for its forward only."""

    def __enter__(self):
        self.before = torch.backends.cudnn.deterministic
        torch.backends.cudnn.deterministic = True

    def __exit__(self, *exc):
        torch.backends.cudnn.deterministic = self.before


def fused_chain(model, a, b):
    """metrics.LPIPS.loss with a backward -> (loss, rows (B, 6), gradient (B, H, W, 3) float64)."""
    p = nchw(a).requires_grad_(True)
    loss, rows = model.loss(p, nchw(b), clamp=True, return_rows=True)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and rows.dtype == torch.float64 and not rows.requires_grad
    with deterministic_convolutions():
        loss.backward()
    assert p.grad.shape == p.shape and p.grad.is_contiguous()
    return float(loss.detach().double()), rows.cpu().numpy(), hwc(p.grad)


def torch_chain(model, a, b, head=G.safe_head):
    """The same objective composed in torch, fp32, through the same convolutions -> (loss, per-image LPIPS, gradient)."""
    convs, lins = model.device_weights(torch.device(DEV))
    p = nchw(a).requires_grad_(True)
    with deterministic_convolutions():
        loss, per_image = G.chain(p, nchw(b), convs, lins, model.normalize, True, head, pkg("metrics").alexnet_features)
        loss.backward()
    return float(loss.detach().double()), per_image.detach().double().cpu().numpy(), hwc(p.grad)


@functools.lru_cache(maxsize=None)
def whole_case(H, W, normalize):
    """-> (names, a (N, H, W, 3) float32, b, float64 loss, per-image LPIPS, gradient), the reference computed once."""
    model = pkg("metrics").LPIPS.from_seed(0)
    items = R.content(H, W, np.float32)
    a, b = np.stack([x for _, x, _ in items]), np.stack([y for _, _, y in items])
    loss, per_image, grad, _ = G.chain64(a, b, model, normalize)
    return [n for n, _, _ in items], a, b, loss, per_image, grad


def check_chain(tag, names, fused, composed, ref):
    """The rules of the whole chain; fused, composed, ref: (loss, per-image LPIPS, gradient).  -> the worst E_fused of the gradient."""
    e, e_torch = G.rel(fused[0], ref[0]), G.rel(composed[0], ref[0])
    print("%s loss %.6e  E_fused %.2e  E_torch %.2e" % (tag, ref[0], e, e_torch))
    assert e <= max(4.0 * e_torch, G.FLOOR), (tag, e, e_torch)
    ei, ei_torch = G.rel(fused[1], ref[1]), G.rel(composed[1], ref[1])
    eg, eg_torch = G.grad_error(fused[2], ref[2]), G.grad_error(composed[2], ref[2])
    for k, name in enumerate(names):
        print("%s %-9s LPIPS %.6e  E_fused %.2e  E_torch %.2e   gradient norm %.3e  E_fused %.2e  E_torch %.2e"
              % (tag, name, ref[1][k], ei[k], ei_torch[k], np.sqrt((ref[2][k] ** 2).sum()), eg[k], eg_torch[k]))
        assert ei[k] <= max(4.0 * ei_torch[k], G.FLOOR), (tag, name, ei[k], ei_torch[k])
        assert np.all(np.isfinite(fused[2][k])) and eg[k] <= 4.0 * eg_torch[k], (tag, name, eg[k], eg_torch[k])
    return float(eg.max())


@pytest.mark.parametrize("shape", [(31, 31), (45, 71)], ids=lambda s: "%dx%d" % s)
def test_whole_chain_error_rule(shape):
    M = pkg("metrics")
    for normalize in (False, True):
        names, a, b, loss64, per64, grad64 = whole_case(*shape, normalize)
        model = M.LPIPS.from_seed(0, normalize=normalize)
        loss, rows, grad = fused_chain(model, a, b)
        composed = torch_chain(model, a, b)
        worst = check_chain("chain %s normalize=%s" % (shape, normalize), names, (loss, rows[:, 0], grad), composed, (loss64, per64, grad64))
        print("chain %s normalize=%s: worst E_fused of the gradient %.2e" % (shape, normalize, worst))
        k = names.index("identical")
        assert rows[k, 0] == 0.0 and not rows[k].any() and not grad[k].any()
        assert abs(loss - rows[:, 0].mean()) <= 2.0 ** -21 * rows[:, 0].mean()      # (five fp32 roundings and an fp32 mean of them)
        # the forward is the scoring call's bits, every time
        with torch.no_grad():
            again, rows_again = model.loss(nchw(a), nchw(b), return_rows=True)
        assert float(again.double()) == loss and np.array_equal(rows_again.cpu().numpy(), rows)
    one = M.LPIPS.from_seed(0).loss(nchw(a)[0], nchw(b)[0])      # one pair, no batch dimension
    assert one.shape == () and float(one) == float(M.LPIPS.from_seed(0).loss(nchw(a)[:1], nchw(b)[:1]))


def feature_gradients(model, a, b, head):
    """The chain's gradient with respect to its five pred feature maps, which autograd forms before it reaches the ReLUs.  head: a
    function (fa, fb, lins) -> per-image LPIPS.  -> ([features], [their gradients])."""
    convs, lins = model.device_weights(torch.device(DEV))
    x_pred, x_target = pkg("ops").lpips_prepare_loss(nchw(a).requires_grad_(True), nchw(b), normalize=model.normalize)
    with deterministic_convolutions():
        fa = pkg("metrics").alexnet_features(x_pred, convs)
        with torch.no_grad():
            fb = pkg("metrics").alexnet_features(x_target, convs)
        for f in fa:
            f.retain_grad()
        head(fa, fb, lins).mean().backward()
    return [f.detach() for f in fa], [f.grad for f in fa]


def test_dead_pixels_in_the_real_chain():
    """Every bias replaced by -(|b| + 1): on the 45 x 71 constant-region pair ReLU leaves whole pixels zero in every layer (float64 on the
    CPU: 100, 12, 1, 3, 3 of 170, 32, 3, 3, 3).  The torch composition of the published head has NaN in its gradient there: in every
    channel of every all-zero pixel of every feature map.  (That is where it is asserted.  In THIS chain the NaN does not reach the image:
    the op behind each feature map is a ReLU, whose backward writes 0 wherever its output is 0, NaN or not -- measured on the CPU in
    float32 and float64 and on the GPU: 6400, 2304, 384, 768, 768 NaN elements in the five feature gradients, none in the image's.  A
    feature extractor that ends in anything else, or a head applied to given features, has no such mask.)  The fused head's gradient is
    finite in every element, and the fused chain is within the whole chain's rule against the safe float64 chain."""
    M, ops = pkg("metrics"), pkg("ops")
    seeded = M.LPIPS.from_seed(0)
    model = G.with_convs(seeded, G.negative_bias_convs(seeded))
    name, a, b = R.content(45, 71, np.float32)[4]
    assert name == "constant"
    a, b = a[None], b[None]
    loss64, per64, grad64, maps64 = G.chain64(a, b, seeded, False, conv_weights=G.negative_bias_convs(seeded))
    naive_maps, naive_grads = feature_gradients(model, a, b, lambda fa, fb, lins: sum(G.naive_head(x, y, w) for x, y, w in zip(fa, fb, lins)))
    fused_maps, fused_grads = feature_gradients(model, a, b, lambda fa, fb, lins: ops.lpips_head(fa, fb, lins)[0])
    dead = [G.dead_pixels(f.cpu().numpy()) for f in fused_maps]
    print("dead pixels per layer: the GPU's features %s, float64 %s" % ([int(d.sum()) for d in dead], [int(G.dead_pixels(m).sum()) for m in maps64]))
    assert sum(int(d.sum()) for d in dead) >= 1 and all(torch.equal(x, y) for x, y in zip(naive_maps, fused_maps))
    for l, (d, g_naive, g_fused) in enumerate(zip(dead, naive_grads, fused_grads)):
        nan = np.isnan(g_naive.cpu().numpy())
        print("  layer %d: %d NaN elements in the torch head's feature gradient, %d in the fused head's" % (l, nan.sum(), int(g_fused.isnan().sum())))
        assert np.array_equal(nan, np.broadcast_to(d[:, None], nan.shape)) and bool(torch.isfinite(g_fused).all())
    assert any(bool(g.isnan().any()) for g in naive_grads), "the torch composition of the published head was expected to give NaN here"
    loss, rows, grad = fused_chain(model, a, b)
    assert np.all(np.isfinite(grad)) and np.isfinite(loss)
    check_chain("dead pixels 45x71", [name], (loss, rows[:, 0], grad), torch_chain(model, a, b), (loss64, per64, grad64))


def test_refiner_step_with_the_lpips_term():
    import spade_reference as SR
    S, M = pkg("spade"), pkg("metrics")
    model = M.LPIPS.from_seed(0)
    inputs = SR.step_inputs("generator", DEV)[:3]
    assert inputs[2].shape[-2:] == (32, 32)
    adam = lambda m: torch.optim.Adam(m.parameters(), lr=2e-4, betas=(0.5, 0.999))      # noqa: E731
    G0 = SR.seeded("generator").to(DEV)
    twin = copy.deepcopy(G0)
    S.refine_step(twin, adam(twin), *inputs, loss=S.RefineLoss(l2=1.0))
    reached = sorted(k for k, p in twin.named_parameters() if p.grad is not None)
    loss = S.RefineLoss(1, 0, 0, lpips=1.0, lpips_model=model)
    opt = adam(G0)
    steps = [float(S.refine_step(G0, opt, *inputs, loss=loss))]      # (a step returns the loss BEFORE its update)
    grads = {k: p.grad for k, p in G0.named_parameters() if p.grad is not None}
    assert sorted(grads) == reached and len(reached) > 10
    assert all(bool(torch.isfinite(g).all()) for g in grads.values()) and any(bool(g.any()) for g in grads.values())
    steps += [float(S.refine_step(G0, opt, *inputs, loss=loss)) for _ in range(5)]
    print("RefineLoss(l2=1, lpips=1): the loss before each of six steps %s" % " ".join("%.6f" % s for s in steps))
    assert steps[5] < steps[0]
    # lpips = 0: the bits of the objective without the term, loss and gradient
    fake = inputs[0].detach().clone()
    results = []
    for objective in (S.RefineLoss(l2=1.0), S.RefineLoss(l2=1.0, lpips=0.0), S.RefineLoss(l2=1.0, lpips=0.0, lpips_model=model)):
        leaf = fake.clone().requires_grad_(True)
        value = objective(leaf, inputs[2])
        value.backward()
        results.append((value.detach(), leaf.grad))
    assert all(torch.equal(bits(v), bits(results[0][0])) and torch.equal(bits(g), bits(results[0][1])) for v, g in results[1:])
    # with the term: the sum of its parts, and more than the MSE alone
    with torch.no_grad():
        both, mse, term = loss(fake, inputs[2]), S.RefineLoss(l2=1.0)(fake, inputs[2]), model.loss(fake, inputs[2])
    assert torch.equal(both, mse + 1.0 * term) and float(term) > 0.0


def test_refusals_by_name():
    M, ops, lib = pkg("metrics"), pkg("ops"), pkg("_lib")
    f = torch.zeros(1, 3, 64, 64, device=DEV)
    with pytest.raises(lib.SahsError, match="pred must be a GPU tensor"):
        ops.lpips_prepare_loss(f.cpu(), f)
    with pytest.raises(lib.SahsError, match="target must be a GPU tensor"):
        ops.lpips_prepare_loss(f, f.cpu())
    with pytest.raises(lib.SahsError, match="pred must be torch.float32 and target torch.uint8 or torch.float32, got torch.float64 and torch.float32"):
        ops.lpips_prepare_loss(f.double(), f)
    with pytest.raises(lib.SahsError, match="got torch.uint8 and torch.uint8"):
        ops.lpips_prepare_loss(f.to(torch.uint8), f.to(torch.uint8))
    with pytest.raises(lib.SahsError, match="got torch.float32 and torch.float16"):
        ops.lpips_prepare_loss(f, f.half())
    with pytest.raises(lib.SahsError, match="target requires a gradient"):
        ops.lpips_prepare_loss(f, f.clone().requires_grad_(True))
    with pytest.raises(lib.SahsError, match="target requires a gradient"):
        M.LPIPS.from_seed(0).loss(f, f.clone().requires_grad_(True))
    with pytest.raises(lib.SahsError, match=r"one shape.*got \(1, 3, 64, 64\) and \(1, 3, 64, 63\)"):
        ops.lpips_prepare_loss(f, f[..., :63])
    with pytest.raises(lib.SahsError, match="30 x 64 pixels"):
        ops.lpips_prepare_loss(f[:, :, :30], f[:, :, :30])
    with pytest.raises(lib.SahsError, match="64 x 30 pixels"):
        M.LPIPS.from_seed(0).loss(f[..., :30].requires_grad_(True), f[..., :30])
    with pytest.raises(lib.SahsError, match="C = 4 channels"):
        ops.lpips_prepare_loss(torch.zeros(1, 4, 64, 64, device=DEV), torch.zeros(1, 4, 64, 64, device=DEV))
    feat, w = torch.zeros(2, 64, 7, 7, device=DEV), torch.zeros(64, device=DEV)
    with pytest.raises(lib.SahsError, match=r"fa\[0\] must be a GPU tensor"):
        ops.lpips_head([feat.cpu()], [feat], [w])
    with pytest.raises(lib.SahsError, match=r"fb\[0\] must be contiguous float32 .* got torch.float64"):
        ops.lpips_head([feat], [feat.double()], [w])
    with pytest.raises(lib.SahsError, match=r"fa\[0\] must be contiguous float32"):
        ops.lpips_head([feat.permute(0, 1, 3, 2)[:, :, :, :5]], [feat[:, :, :, :5].contiguous()], [w])
    with pytest.raises(lib.SahsError, match="2 fa, 1 fb and 2 weight tensors"):
        ops.lpips_head([feat, feat], [feat], [w, w])
    with pytest.raises(lib.SahsError, match="1 .. 5 layers"):
        ops.lpips_head([feat] * 6, [feat] * 6, [w] * 6)
    with pytest.raises(lib.SahsError, match=r"fa\[0\] is \(2, 64, 7, 7\), fb\[0\] \(2, 64, 7, 6\)"):
        ops.lpips_head([feat], [feat[..., :6].contiguous()], [w])
    with pytest.raises(lib.SahsError, match=r"with 63 weights"):
        ops.lpips_head([feat], [feat], [w[:63]])
    with pytest.raises(lib.SahsError, match="job 0 has C = 1025"):
        ops.lpips_head([torch.zeros(2, 1025, 1, 1, device=DEV)], [torch.zeros(2, 1025, 1, 1, device=DEV)], [torch.zeros(1025, device=DEV)])
    torch.cuda.synchronize()
