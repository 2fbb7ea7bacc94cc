"""float64 references for the image metrics (ops.image_metrics, metrics.py) and the inputs their tests share.

No fixture can come from the reference program (nerf/metrics.py imports scikit-image, which is not a dependency here), so the yardstick
is a float64 restatement of what it computes, written twice and independently:
  (a) ``ssim_direct``: every 7x7 window taken with sliding_window_view and its statistics formed CENTRED, in two passes (mean, then
      deviations) -- nothing cancels;
  (b) ``ssim_filtered``: the algorithm skimage.metrics.structural_similarity publishes -- five scipy.ndimage.uniform_filter planes,
      vx = 49/48 (E[x^2] - E[x]^2), S cropped by 3 and averaged.
tests/test_metrics_host.py holds them to 1e-12 of each other.  Images are (H, W, C) arrays; uint8 images are scored as x / 255.
"""
import numpy as np

TILE = 32      # include/sahs_nerf.h: SAHS_IMAGE_METRICS_TILE (tests/test_metrics_host.py checks the two agree)
WIN = 7

# (H, W) of the GPU tests: (H - 6, W - 6) = (1,1), (1,2), (2,1), (T,T), (T+1,T), (T,T+1), (T-1,2T+1), and one odd shape
SHAPES = [(7, 7), (7, 8), (8, 7), (TILE + 6, TILE + 6), (TILE + 7, TILE + 6), (TILE + 6, TILE + 7), (TILE + 5, 2 * TILE + 7), (45, 71)]


def as_float64(img):
    img = np.asarray(img)
    return img.astype(np.float64) / 255.0 if img.dtype == np.uint8 else img.astype(np.float64)


def _constants(data_range):
    return (0.01 * data_range) ** 2, (0.03 * data_range) ** 2


def ssim_direct(a, b, data_range=1.0):
    """-> per-channel mean SSIM, (C,) float64."""
    a, b = as_float64(a), as_float64(b)
    C1, C2 = _constants(data_range)
    out = []
    for c in range(a.shape[2]):
        wa = np.lib.stride_tricks.sliding_window_view(a[:, :, c], (WIN, WIN)).reshape(a.shape[0] - 6, a.shape[1] - 6, 49)
        wb = np.lib.stride_tricks.sliding_window_view(b[:, :, c], (WIN, WIN)).reshape(wa.shape)
        ua, ub = wa.mean(-1), wb.mean(-1)
        da, db = wa - ua[..., None], wb - ub[..., None]
        va, vb, vab = (da * da).sum(-1) / 48.0, (db * db).sum(-1) / 48.0, (da * db).sum(-1) / 48.0
        S = ((2 * ua * ub + C1) * (2 * vab + C2)) / ((ua * ua + ub * ub + C1) * (va + vb + C2))
        out.append(S.mean())
    return np.array(out)


def ssim_filtered(a, b, data_range=1.0):
    """skimage's published algorithm (win_size 7, sample covariance, crop 3) -> per-channel mean SSIM, (C,) float64."""
    from scipy.ndimage import uniform_filter
    a, b = as_float64(a), as_float64(b)
    C1, C2 = _constants(data_range)
    cov_norm = 49.0 / 48.0
    out = []
    for c in range(a.shape[2]):
        x, y = a[:, :, c], b[:, :, c]
        ux, uy = uniform_filter(x, size=WIN), uniform_filter(y, size=WIN)
        uxx, uyy, uxy = uniform_filter(x * x, size=WIN), uniform_filter(y * y, size=WIN), uniform_filter(x * y, size=WIN)
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
        out.append(S[3:-3, 3:-3].mean())
    return np.array(out)


def reference_row(a, b, ssim_data_range=1.0, ssim=ssim_direct):
    """The row ops.image_metrics returns for one pair: [mean SSIM, MSE, L1, SSIM per channel], float64."""
    per = ssim(a, b, ssim_data_range)
    d = as_float64(a) - as_float64(b)
    return np.concatenate([[per.mean(), (d * d).mean(), np.abs(d).mean()], per])


def psnr(mse, data_range=1.0):
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(data_range ** 2 / np.asarray(mse, np.float64))


# ---- inputs ----
def _finish(img, dtype):
    img = np.clip(img, 0.0, 1.0)
    return np.round(img * 255.0).astype(np.uint8) if dtype == np.uint8 else img.astype(np.float32)


def ramp(H, W, C):
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([(0.15 + 0.7 * ((x + 3 * c) / (W + 8) * 0.6 + y / max(H - 1, 1) * 0.4)) * (1.0 - 0.1 * c) for c in range(C)], axis=-1)


def ramp_noise_pair(H, W, C, noise, seed, dtype):
    """A smooth ramp and the same ramp plus noise (the SSIM of the pair falls from about 0.99 to about 0.3 as noise goes 0.005 -> 0.07)."""
    rng = np.random.default_rng(seed)
    a = ramp(H, W, C) + rng.normal(0.0, 0.01, (H, W, C))
    return _finish(a, dtype), _finish(a + rng.normal(0.0, noise, (H, W, C)), dtype)


def flat_bright_pair(H, W, C, dtype, seed=5):
    """0.97 +- 0.002: where E[x^2] - E[x]^2 in fp32 cancels."""
    rng = np.random.default_rng(seed)
    return _finish(0.97 + rng.uniform(-0.002, 0.002, (H, W, C)), dtype), _finish(0.97 + rng.uniform(-0.002, 0.002, (H, W, C)), dtype)


def constant_pair(H, W, C, p, q, dtype):
    return _finish(np.full((H, W, C), p), dtype), _finish(np.full((H, W, C), q), dtype)


def seam(n):
    """The first row / column past a tile of window origins (the last one where the image has no second tile)."""
    return min(TILE, n - 1)


def single_pixel_positions(H, W):
    return [(0, 0), (H - 1, W - 1), (seam(H), seam(W))]


def single_pixel_pair(H, W, C, pos, dtype, seed=11):
    """An identical pair but for one pixel, which differs by the whole range in every channel."""
    a, _ = ramp_noise_pair(H, W, C, 0.0, seed, dtype)
    b = a.copy()
    full = 255 if dtype == np.uint8 else 1.0
    a[pos[0], pos[1], :] = 0
    b[pos[0], pos[1], :] = full
    return a, b


NOISE = (0.005, 0.03, 0.07)
GENERIC = tuple("noise%g" % n for n in NOISE)


def content(H, W, C, dtype):
    """The pairs of one shape, [(name, a, b)]: generic content at three noise levels, and the special cases."""
    out = [("noise%g" % n, *ramp_noise_pair(H, W, C, n, 100 + i, dtype)) for i, n in enumerate(NOISE)]
    _, a = ramp_noise_pair(H, W, C, 0.1, 7, dtype)      # (textured: its negative has a negative covariance well above C2)
    out.append(("identical", a, a.copy()))
    out.append(("constants", *constant_pair(H, W, C, 0.25, 0.75, dtype)))
    out.append(("inverted", a, (255 - a) if dtype == np.uint8 else (np.float32(1.0) - a)))
    out.append(("flat_bright", *flat_bright_pair(H, W, C, dtype)))
    out += [("pixel%d_%d" % pos, *single_pixel_pair(H, W, C, pos, dtype)) for pos in single_pixel_positions(H, W)]
    return out


def torch_formulation(a, b, ssim_data_range=1.0):
    """The same metrics the way torch offers them, in the tensors' own precision: five avg_pool2d moment planes and the raw-moment
    variances.  a, b: (B, C, H, W) float tensors -> (B, 3 + C) rows like ops.image_metrics'.  The GPU tests measure its fp32 error
    (E_torch) and tools/time_metrics.py its time."""
    import torch
    import torch.nn.functional as F
    C1, C2 = _constants(ssim_data_range)
    ux, uy = F.avg_pool2d(a, WIN, 1), F.avg_pool2d(b, WIN, 1)
    uxx, uyy, uxy = F.avg_pool2d(a * a, WIN, 1), F.avg_pool2d(b * b, WIN, 1), F.avg_pool2d(a * b, WIN, 1)
    n = 49.0 / 48.0
    vx, vy, vxy = n * (uxx - ux * ux), n * (uyy - uy * uy), n * (uxy - ux * uy)
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    per = S.mean(dim=(2, 3))
    d = a - b
    return torch.cat([per.mean(1, keepdim=True), (d * d).mean(dim=(1, 2, 3))[:, None], d.abs().mean(dim=(1, 2, 3))[:, None], per], dim=1)
