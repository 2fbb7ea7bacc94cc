"""float64 references for the fused image objective (ops.image_loss, include/sahs_nerf.h: sahs_image_loss) and the inputs its tests share.

    loss = w_l2 MSE(x, t) + w_l1 L1(x, t) + w_ssim (1 - SSIM(x, t)),   x = clamp(pred, 0, 1) or pred,

for ONE image (H, W, C); a batch's loss is the mean of its images' and its gradient theirs over B.  Loss and gradient are stated twice and
independently:
  (a) ``autograd_terms``: torch float64 autograd through a centred two-pass window statement (``unfold``; mean, then deviations), torch's
      own clamp, ``abs`` and ``pow`` rules;
  (b) ``closed_terms``: numpy, no autograd: per window dS/dx_p = alpha_w + beta_w x_p + gamma_w y_p, the pixel's gradient the 7x7 box sums
      of the three coefficient planes over the window origins in [p - 6, p]^2, the mask and sign written out.
tests/test_image_loss_reference_host.py holds them to 1e-11 of the gradient's scale of each other.  Both return the three TERMS
[MSE, L1, 1 - SSIM] and their three gradients, so that any weighting is one dot product (the objective is linear in its weights).
``closed_terms`` takes a ``fault`` for the sensitivity tests: what a kernel that got one thing wrong would compute.
"""
import functools

import numpy as np

import metrics_reference as M

TILE = 32      # include/sahs_nerf.h: SAHS_IMAGE_LOSS_TILE (tests/test_image_loss_reference_host.py checks the two agree)
WIN = 7
WEIGHTS = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (1.0, 0.5, 0.25)]
FLOOR = 2.0 ** -20
FAULTS = ("drop_gamma", "seam_row", "exclusive_clamp", "sign0_is_1", "norm_hw")


def gpu_shapes(T=TILE):
    """(H, W) of the GPU tests: one window, one more in each direction, less than a tile, exactly one, one pixel / row / column more, two
    tiles and a pixel, tiles whose halo of origins crosses the image's last windows, and one odd shape."""
    return [(7, 7), (7, 8), (8, 7), (13, 13), (T, T), (T + 1, T), (T, T + 1), (T - 1, 2 * T + 1), (2 * T + 7, T + 6), (45, 71)]


# ---- inputs ----
PLANTED_EDGES = ((3, 0.0), (17, 1.0), (31, -0.0))      # (flat index, value): elements exactly on the clamp's ends, which pass the gradient
PLANTED_EQUAL = (5, 20, 40)      # flat indices where pred == target: L1 contributes 0 there


@functools.lru_cache(maxsize=None)
def inputs(H, W, C):
    """-> [(name, pred, target)], float32 (H, W, C): every pair of metrics_reference.content with pred = a + 0.15 N(0, 1) (1 - 45 % of
    its elements leave [0, 1], so the clamp's mask is exercised), the untouched identical pair, and the two planted cases."""
    rng = np.random.default_rng(20240)
    out, generic = [], None
    for name, a, b in M.content(H, W, C, np.float32):
        pred = (a.astype(np.float64) + 0.15 * rng.standard_normal(a.shape)).astype(np.float32)
        out.append((name, pred, b))
        if name == "identical":
            same = (a, b)
        if name == "noise0.03":
            generic = (pred, b)
    out.append(("identical_exact", same[0], same[1].copy()))
    pred = generic[0].copy()
    for k, v in PLANTED_EDGES:
        pred.flat[k] = np.float32(v)
    assert np.signbit(pred.flat[PLANTED_EDGES[2][0]]) and all(generic[1].flat[k] not in (0.0, 1.0) for k, _ in PLANTED_EDGES)
    out.append(("planted_edges", pred, generic[1]))
    pred = generic[0].copy()
    for k in PLANTED_EQUAL:
        pred.flat[k] = generic[1].flat[k]
    out.append(("planted_equal", pred, generic[1]))
    return out


# ---- (b) the closed form ----
def _box(plane):
    """7x7 sums over the origins in [p - 6, p]^2: (H - 6, W - 6) -> (H, W)."""
    padded = np.pad(plane, WIN - 1)
    return np.lib.stride_tricks.sliding_window_view(padded, (WIN, WIN)).sum((-1, -2))


def _ssim_closed(x, y, data_range, fault):
    """x, y: (H, W) float64 -> mean S over the windows, and its gradient with respect to x."""
    H, W = x.shape
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    m_x, m_y = x.mean(), y.mean()      # the frame alpha is formed in: any shift is valid, a close one keeps alpha + beta x + gamma y from cancelling
    wx = np.lib.stride_tricks.sliding_window_view(x, (WIN, WIN)).reshape(H - 6, W - 6, 49)
    wy = np.lib.stride_tricks.sliding_window_view(y, (WIN, WIN)).reshape(H - 6, W - 6, 49)
    ux, uy = wx.mean(-1), wy.mean(-1)
    dx, dy = wx - ux[..., None], wy - uy[..., None]
    vx, vy, vxy = (dx * dx).sum(-1) / 48.0, (dy * dy).sum(-1) / 48.0, (dx * dy).sum(-1) / 48.0
    A1, A2, B1, B2 = 2 * ux * uy + C1, 2 * vxy + C2, ux * ux + uy * uy + C1, vx + vy + C2
    S = A1 * A2 / (B1 * B2)
    beta = -2.0 * S / (48.0 * B2)
    gamma = 2.0 * A1 / (48.0 * B1 * B2)
    if fault == "drop_gamma":
        gamma = np.zeros_like(gamma)
    alpha = (2.0 * uy * A2 / (B1 * B2) - 2.0 * ux * S / B1) / 49.0 - beta * (ux - m_x) - gamma * (uy - m_y)
    if fault == "seam_row":      # the row of origins past the first tile of pixels (the last one where the image has no second tile)
        r = min(TILE, H - 7)
        alpha, beta, gamma = (np.where(np.arange(H - 6)[:, None] == r, 0.0, c) for c in (alpha, beta, gamma))
    windows = H * W if fault == "norm_hw" else (H - 6) * (W - 6)
    grad = (_box(alpha) + (x - m_x) * _box(beta) + (y - m_y) * _box(gamma)) / windows
    return S.sum() / windows, grad


def closed_terms(pred, target, clamp=True, data_range=1.0, fault=None):
    """-> terms (3,) = [MSE, L1, 1 - SSIM] and grads (3, H, W, C) = their gradients with respect to pred, float64."""
    assert fault is None or fault in FAULTS
    p, t = np.asarray(pred, np.float64), np.asarray(target, np.float64)
    x = np.clip(p, 0.0, 1.0) if clamp else p
    if not clamp:
        mask = np.ones_like(p)
    elif fault == "exclusive_clamp":
        mask = ((p > 0.0) & (p < 1.0)).astype(np.float64)
    else:
        mask = ((p >= 0.0) & (p <= 1.0)).astype(np.float64)      # torch's rule; -0.0 >= 0.0
    d = x - t
    sign = np.sign(d) if fault != "sign0_is_1" else np.where(d >= 0.0, 1.0, -1.0)
    C = p.shape[2]
    per = [_ssim_closed(x[:, :, c], t[:, :, c], data_range, fault) for c in range(C)]
    ssim = np.mean([s for s, _ in per])
    g_ssim = np.stack([g for _, g in per], axis=-1) / C
    terms = np.array([(d * d).mean(), np.abs(d).mean(), 1.0 - ssim])
    grads = np.stack([2.0 * d / d.size, sign / d.size, -g_ssim]) * mask
    return terms, grads


# ---- (a) autograd ----
def _ssim_unfold(x, y, data_range):
    """x, y: (C, H, W) float64 tensors -> mean SSIM (a 0-d tensor), every window centred in two passes."""
    import torch.nn.functional as F
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    wx, wy = F.unfold(x[:, None], WIN), F.unfold(y[:, None], WIN)      # (C, 49, windows)
    ux, uy = wx.mean(1, keepdim=True), wy.mean(1, keepdim=True)
    dx, dy = wx - ux, wy - uy
    vx, vy, vxy = (dx * dx).sum(1) / 48.0, (dy * dy).sum(1) / 48.0, (dx * dy).sum(1) / 48.0
    ux, uy = ux[:, 0], uy[:, 0]
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return S.mean(1).mean()


def autograd_terms(pred, target, clamp=True, data_range=1.0):
    """The same as closed_terms, by torch float64 autograd."""
    import torch
    t = torch.from_numpy(np.asarray(target, np.float64)).permute(2, 0, 1)
    terms, grads = [], []
    for k in range(3):
        p = torch.from_numpy(np.asarray(pred, np.float64)).requires_grad_(True)
        x = p.permute(2, 0, 1)
        x = x.clamp(0, 1) if clamp else x
        term = ((x - t) ** 2).mean() if k == 0 else (x - t).abs().mean() if k == 1 else 1.0 - _ssim_unfold(x, t, data_range)
        term.backward()
        terms.append(float(term.detach()))
        grads.append(p.grad.numpy())
    return np.array(terms), np.stack(grads)


# ---- the error measure, and torch's own formulation ----
def combine(terms, grads, weights):
    w = np.asarray(weights, np.float64)
    return float(w @ terms), np.tensordot(w, grads, 1)


def grad_error(g, g64, weights, batch=1):
    """E = max |g - g64| / max(max |g64|, (|w_l2| + |w_l1| + |w_ssim|) / N), N the elements of the batch (the floor gives an all-zero
    gradient, the identical pair's, a scale: that of one element's share of the weights)."""
    g, g64 = np.asarray(g, np.float64), np.asarray(g64, np.float64)
    return float(np.abs(g - g64).max()) / max(float(np.abs(g64).max()), float(np.abs(np.asarray(weights)).sum()) / (g64.size * batch))


def torch_composition(pred, target, weights, clamp=True, data_range=1.0):
    """The objective the way torch offers it, in the tensors' own precision and on their device: metrics_reference.torch_formulation's
    SSIM (five avg_pool2d planes, raw-moment variances) and MSE / L1 on the clamped prediction.  pred, target: (B, C, H, W) tensors
    -> the loss, a 0-d tensor with autograd.  The GPU tests measure its fp32 error (E_torch), tools/time_image_loss.py its time."""
    import torch.nn.functional as F
    x, y = (pred.clamp(0, 1) if clamp else pred), target
    C1, C2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    ux, uy = F.avg_pool2d(x, WIN, 1), F.avg_pool2d(y, WIN, 1)
    uxx, uyy, uxy = F.avg_pool2d(x * x, WIN, 1), F.avg_pool2d(y * y, WIN, 1), F.avg_pool2d(x * y, WIN, 1)
    n = 49.0 / 48.0
    vx, vy, vxy = n * (uxx - ux * ux), n * (uyy - uy * uy), n * (uxy - ux * uy)
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    ssim = S.mean(dim=(2, 3)).mean(1).mean()      # windows, then channels, then the batch: metrics_reference.torch_formulation's order
    return weights[0] * F.mse_loss(x, y) + weights[1] * F.l1_loss(x, y) + weights[2] * (1.0 - ssim)
