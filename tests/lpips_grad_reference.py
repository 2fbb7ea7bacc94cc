"""float64 references for LPIPS as a training term (metrics.LPIPS.loss, ops.lpips_prepare_loss, ops.lpips_head) and what its tests share.
tests/lpips_reference.py holds the forward's; this module adds the gradient with respect to the first operand.

The head, per layer and pixel, with na = sqrt(sum a^2) + 1e-10, a^ = a / na (b likewise) and d = sum_c w_c (a^_c - b^_c)^2:
    dd/da_k = (2 / na) [ w_k (a^_k - b^_k) - a_k q ],   q = S / (sqrt(sa) na),   S = sum_c w_c (a^_c - b^_c) a_c,   q = 0 where sa == 0.
It is written three ways:
  ``closed_head_grad``   the closed form above, numpy float64, from the definition of S (not from the kernel's expansion of it);
  ``safe_head``          the head in torch with sqrt taken only where sa > 0 -- at an all-zero pixel a -> a / (|a| + 1e-10) is
                         differentiable with Jacobian I / 1e-10, and this statement lets autograd see that; THE yardstick;
  ``naive_head``         the published formula as torch writes it, whose autograd is NaN at such a pixel (sqrt's derivative at 0 is
                         inf, and 0 * inf behind it): why the yardstick is the safe statement.
``chain`` is clamp -> scaling layer -> lpips_reference.feature_maps -> a head -> mean over the batch, in the dtype and on the device of
its inputs, each step one torch operation with tensor divisors: in float64 on the CPU the whole objective's reference (``chain64``), in
float32 on the GPU the composition a user would write (E_torch of the GPU tests).
"""
import numpy as np
import torch

import lpips_reference as R

EPS = R.EPS
FLOOR = 2.0 ** -20      # tests/test_gpu_lpips.py: FLOOR, the project's floor for E of a whole-metric value


def closed_head_grad(fa, fb, w, g):
    """fa, fb: (B, C, h, w) arrays, w: (C,), g: (B,) upstream gradients of each image's d_l -> float64 (B, C, h, w), the gradient with
    respect to fa of sum_i g_i * mean over pixels of d."""
    fa, fb, g = np.asarray(fa, np.float64), np.asarray(fb, np.float64), np.asarray(g, np.float64)
    w = np.asarray(w, np.float64).reshape(1, -1, 1, 1)
    sa = (fa * fa).sum(1, keepdims=True)
    na, nb = np.sqrt(sa) + EPS, np.sqrt((fb * fb).sum(1, keepdims=True)) + EPS
    diff = fa / na - fb / nb
    S = (w * diff * fa).sum(1, keepdims=True)
    q = np.where(sa > 0, S / np.where(sa > 0, np.sqrt(sa) * na, 1.0), 0.0)
    hw = fa.shape[2] * fa.shape[3]
    return (2.0 * g.reshape(-1, 1, 1, 1) / hw) / na * (w * diff - fa * q)


def kernel_order_head_grad(fa, fb, w, g):
    """The gradient in the kernel's evaluation order (csrc/lpips.hip), float64 rounded to float32 once: the five sums give ra = 1 / na,
    rb = 1 / nb and q = (swa / na - swab / nb) / (sqrt(sa) na), then (2 g / hw) ra (w (a ra - b rb) - a q).  numpy's sums are pairwise
    where the kernel's are sequential, so this is the kernel up to the sums' rounding."""
    fa, fb, g = np.asarray(fa, np.float64), np.asarray(fb, np.float64), np.asarray(g, np.float64)
    w = np.asarray(w, np.float64).reshape(1, -1, 1, 1)
    sa, sb = (fa * fa).sum(1, keepdims=True), (fb * fb).sum(1, keepdims=True)
    swa, swab = (w * (fa * fa)).sum(1, keepdims=True), (w * (fa * fb)).sum(1, keepdims=True)
    na, nb = np.sqrt(sa) + EPS, np.sqrt(sb) + EPS
    ra, rb = 1.0 / na, 1.0 / nb
    q = np.where(sa == 0, 0.0, (swa / na - swab / nb) / np.where(sa == 0, 1.0, np.sqrt(sa) * na))
    k = (2.0 * g.reshape(-1, 1, 1, 1) / (fa.shape[2] * fa.shape[3])) * ra
    return (k * (w * (fa * ra - fb * rb) - fa * q)).astype(np.float32)


def _safe_norm(f):
    s = (f * f).sum(1, keepdim=True)
    alive = s > 0
    return torch.where(alive, torch.sqrt(torch.where(alive, s, torch.ones_like(s))), torch.zeros_like(s)) + EPS


def safe_head(fa, fb, w):
    """fa, fb: (B, C, h, w) tensors, w: C weights -> (B,) d_l; sqrt only where sum a^2 > 0."""
    d = (fa / _safe_norm(fa) - fb / _safe_norm(fb)) ** 2
    return (d * w.reshape(1, -1, 1, 1)).sum(1).mean(dim=(1, 2))


def naive_head(fa, fb, w):
    """The published head (lpips_reference.torch_head) on two operands -> (B,)."""
    na = fa / (torch.sqrt(torch.sum(fa * fa, dim=1, keepdim=True)) + EPS)
    nb = fb / (torch.sqrt(torch.sum(fb * fb, dim=1, keepdim=True)) + EPS)
    return (((na - nb) ** 2) * w.reshape(1, -1, 1, 1)).sum(1).mean(dim=(1, 2))


def autograd_head_grad(fa, fb, w, g, head=safe_head):
    """float64 autograd of ``head`` -> (B, C, h, w) array."""
    a = torch.from_numpy(np.asarray(fa, np.float64)).requires_grad_(True)
    d = head(a, torch.from_numpy(np.asarray(fb, np.float64)), torch.from_numpy(np.asarray(w, np.float64)))
    (d * torch.from_numpy(np.asarray(g, np.float64))).sum().backward()
    return a.grad.numpy()


def head_case(B, C, h, w, seed):
    """-> (fa, fb (B, C, h, w) float32, weights (C,) float32): lpips_reference.synthetic_features split into its operands, with, where the
    layer has the pixels, one pixel dead in fa alone (the last of image 0) next to the ones synthetic_features plants (pixel 0 of image
    0: dead in both).
    No pixel is left with a^ = b^ to rounding.  synthetic_features copies fb = 1.01 fa element by element with probability 1/2, so at
    C = 5 one pixel in 32 has fb = 1.01 fa in every channel; there a^_c - b^_c = O(1e-12) is the difference of two values near 1 that
    float64 holds to 1e-16 each: the whole pixel's gradient is known to 1e-4 of itself in ANY float64 evaluation, this module's
    included, and no comparison to 2^-23 says anything.  (The gradient there is 1e-12 of its neighbours'.)  The same holds for a live
    pixel of fa with ONE non-zero channel: a^ = e_k (1 - 1e-10 / a_k) is saturated, its derivative is 1e-10 of a usual one, and the
    bracket w_k a^_k (1 - a^_k) is a difference that float64 holds to 2e-7 of itself.  So channels 1 and 2 of fa and channel 0 of fb
    are lifted at their live pixels: every live pixel of fa has two non-zero channels, and the two directions differ (``separation``
    measures it)."""
    f, lw = R.synthetic_features(B, C, h, w, seed)
    fa, fb = f[:B].copy(), f[B:].copy()
    fa[:, 1] = np.where(dead_pixels(fa), 0.0, fa[:, 1] + np.float32(0.2))
    fa[:, 2] = np.where(dead_pixels(fa), 0.0, fa[:, 2] + np.float32(0.1))
    fb[:, 0] = np.where(dead_pixels(fb), 0.0, fb[:, 0] + np.float32(0.3))
    if h * w > 1:
        fa[0, :, -1, -1] = 0.0
        fb[0, :, -1, -1] = np.maximum(fb[0, :, -1, -1], 0.25)
    return fa, fb, lw


def dead_pixels(f):
    """(B, C, h, w) -> (B, h, w) bool: every channel zero."""
    return ~np.asarray(f).any(axis=1)


def separation(fa, fb):
    """The least max_c |a^_c - b^_c| over the pixels that are not all zero in both operands: how far the head's differences are from
    pure cancellation (see head_case)."""
    fa, fb = np.asarray(fa, np.float64), np.asarray(fb, np.float64)
    diff = np.abs(fa / (np.sqrt((fa * fa).sum(1, keepdims=True)) + EPS) - fb / (np.sqrt((fb * fb).sum(1, keepdims=True)) + EPS)).max(1)
    return float(diff[~(dead_pixels(fa) & dead_pixels(fb))].min())


def head_rule(got, ref):
    """The GPU head's rule, per element: |got - ref| <= 2^-23 |ref| + 2^-40 m, m the pixel's largest |ref| -- one fp32 rounding with a
    factor 2 of slack, and 8x the float64 accumulation bound C 2^-53 at C = 1024 for elements whose two bracket terms cancel.
    -> the worst ratio of error to tolerance (<= 1 passes; 0 / 0 counts as 0)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    tol = 2.0 ** -23 * np.abs(ref) + 2.0 ** -40 * np.abs(ref).max(axis=1, keepdims=True)
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(err == 0, 0.0, err / tol).max())      # (a NaN or an error at tolerance 0 does not pass)


# ---- the whole objective ----
def scaling_steps(pred, target, normalize, clamp):
    """pred, target: (B, 3, H, W) tensors of one dtype and device -> (x_pred, x_target), one torch operation per step, true divisions
    (the divisors are tensors); the clamp on pred alone."""
    shift = torch.tensor(R.SHIFT, dtype=pred.dtype, device=pred.device).reshape(1, 3, 1, 1)
    scale = torch.tensor(R.SCALE, dtype=pred.dtype, device=pred.device).reshape(1, 3, 1, 1)
    out = []
    for x, c in ((pred, clamp), (target, False)):
        if c:
            x = x.clamp(0.0, 1.0)
        if normalize:
            x = 2.0 * x - 1.0
        out.append((x - shift) / scale)
    return out


def chain(pred, target, convs, lins, normalize, clamp=True, head=safe_head, features=R.feature_maps):
    """-> (loss 0-d, per-image LPIPS (B,)): mean over the batch of sum_l head(features_l(pred), features_l(target)).  pred may require a
    gradient; the target side is evaluated under no_grad, as the product evaluates it."""
    xa, xb = scaling_steps(pred, target, normalize, clamp)
    fa = features(xa, convs)
    with torch.no_grad():
        fb = features(xb, convs)
    per_image = sum(head(a, b, w) for a, b, w in zip(fa, fb, lins))
    return per_image.mean(), per_image


def chain64(pred, target, model, normalize, clamp=True, conv_weights=None):
    """pred, target: (B, H, W, 3) float arrays -> (loss, per-image LPIPS (B,), gradient (B, H, W, 3), the five pred feature maps), all
    float64 on the CPU; the gradient is autograd's of the safe head."""
    convs, lins = R.float64_weights(model)
    if conv_weights is not None:
        convs = [(w.double(), b.double()) for w, b in conv_weights]
    p = torch.from_numpy(np.asarray(pred, np.float64)).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    t = torch.from_numpy(np.asarray(target, np.float64)).permute(0, 3, 1, 2).contiguous()
    kept = []

    def features(x, cw):
        maps = R.feature_maps(x, cw)
        kept.append(maps)
        return maps

    loss, per_image = chain(p, t, convs, [torch.from_numpy(w) for w in lins], normalize, clamp, safe_head, features)
    loss.backward()
    return float(loss.detach()), per_image.detach().numpy(), p.grad.permute(0, 2, 3, 1).numpy(), [m.detach().numpy() for m in kept[0]]


def negative_bias_convs(model):
    """The model's convolutions with every bias replaced by -(|b| + 1.0): ReLU then leaves whole pixels zero wherever the input is
    constant.  -> [(weight, bias)] * 5, float32 CPU tensors."""
    return [(w, -(b.abs() + 1.0)) for w, b in model.conv_weights()]


def with_convs(model, convs):
    """A metrics.LPIPS like ``model`` (its class, its channel weights, its ``normalize``) on other convolutions."""
    alexnet, linear = {}, {k: v for k, v in model.state.items() if k.startswith("lin")}
    keys = [k for k in model.state if k.startswith("features.") and k.endswith(".weight")]
    for key, (w, b) in zip(keys, convs):
        alexnet[key], alexnet[key.replace(".weight", ".bias")] = w, b
    return type(model)(alexnet, linear, normalize=model.normalize)


def grad_error(g, g64):
    """Per image: ||g - g64||_2 / ||g64||_2 (the absolute norm where g64 is all zero).  g, g64: (B, ...) -> (B,)."""
    g, g64 = np.asarray(g, np.float64).reshape(len(g64), -1), np.asarray(g64, np.float64).reshape(len(g64), -1)
    num, den = np.sqrt(((g - g64) ** 2).sum(1)), np.sqrt((g64 ** 2).sum(1))
    return np.where(den == 0, num, num / np.where(den == 0, 1.0, den))


def rel(got, ref):
    """|got - ref| / |ref|, absolute where ref == 0."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return np.where(ref == 0, np.abs(got - ref), np.abs(got - ref) / np.where(ref == 0, 1.0, np.abs(ref)))
