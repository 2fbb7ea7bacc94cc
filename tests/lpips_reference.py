"""float64 reference for LPIPS (net = alex, v0.1; metrics.LPIPS, ops.lpips_prepare, ops.lpips_distance) and the inputs its tests share.

No fixture can come from the lpips package or from the reference program (neither the package nor its weights are available to this
project), so the yardstick is the published definition written directly in float64 on the CPU:
  1. scaling layer  x' = (x - shift) / scale per channel (uint8 images are x / 255; normalize maps x -> 2x - 1 first);
  2. the five ReLU outputs of torchvision's AlexNet ``features`` (convolutions 11/4/2, 5/1/2, 3/1/1 x 3, a 3/2 max-pool ahead of the
     second and third);
  3. per layer  a^ = a / (sqrt(sum_c a_c^2) + 1e-10),  d_l = mean over pixels of sum_c w_lc (a^_c - b^_c)^2;  LPIPS = sum_l d_l.
The head is written three times: ``head_two_pass`` (normalise, subtract, square, weight, mean: THE reference), ``head_pixel_loop`` (an
independent loop over pixels) and ``head_one_pass`` (the expansion the kernel evaluates, in float64); tests/test_lpips_reference_host.py
holds them to each other.  Images are (H, W, 3) arrays, features (C, h, w) arrays.
"""
import numpy as np
import torch
import torch.nn.functional as F

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
EPS = 1e-10
TILE = 256      # include/sahs_nerf.h: SAHS_LPIPS_TILE (tests/test_lpips_host.py checks the two agree)
MIN_SIDE = 31
# (out channels, in channels, kernel, stride, padding, max-pool 3/2 first) of the five convolutions
CONVS = ((64, 3, 11, 4, 2, False), (192, 64, 5, 1, 2, True), (384, 192, 3, 1, 1, True), (256, 384, 3, 1, 1, False), (256, 256, 3, 1, 1, False))
SHAPES = [(31, 31), (45, 71), (127, 130)]      # of the whole-metric GPU tests
MAP_SIZES = {(31, 31): [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)], (45, 71): [(10, 17), (4, 8), (1, 3), (1, 3), (1, 3)]}


def as_float64(img):
    img = np.asarray(img)
    return img.astype(np.float64) / 255.0 if img.dtype == np.uint8 else img.astype(np.float64)


def scaling(images, normalize):
    """(N, H, W, 3) uint8 / float -> (N, 3, H, W) float64 after the scaling layer."""
    x = as_float64(images)
    if normalize:
        x = 2.0 * x - 1.0
    return np.ascontiguousarray(((x - np.array(SHIFT)) / np.array(SCALE)).transpose(0, 3, 1, 2))


def feature_maps(x, conv_weights):
    """x: (N, 3, H, W) tensor; conv_weights: [(weight, bias)] * 5 in x's dtype -> the five ReLU outputs, a list of (N, C, h, w) tensors."""
    if x.shape[-1] < MIN_SIDE or x.shape[-2] < MIN_SIDE:
        raise ValueError("a %d x %d image leaves AlexNet's second max-pool nothing: needs %d <= H, W" % (x.shape[-2], x.shape[-1], MIN_SIDE))
    out = []
    for (_, _, _, stride, pad, pool), (w, b) in zip(CONVS, conv_weights):
        if pool:
            x = F.max_pool2d(x, 3, 2)
        x = F.relu(F.conv2d(x, w, b, stride=stride, padding=pad))
        out.append(x)
    return out


def head_two_pass(fa, fb, w):
    """fa, fb: (C, h, w) float64 arrays, w: (C,) -> d_l."""
    fa, fb, w = np.asarray(fa, np.float64), np.asarray(fb, np.float64), np.asarray(w, np.float64).reshape(-1)
    na = fa / (np.sqrt((fa * fa).sum(0, keepdims=True)) + EPS)
    nb = fb / (np.sqrt((fb * fb).sum(0, keepdims=True)) + EPS)
    diff = (na - nb) ** 2
    return float((diff * w[:, None, None]).sum(0).mean())


def head_pixel_loop(fa, fb, w):
    fa, fb, w = np.asarray(fa, np.float64), np.asarray(fb, np.float64), np.asarray(w, np.float64).reshape(-1)
    C, h, wd = fa.shape
    total = 0.0
    for y in range(h):
        for x in range(wd):
            a, b = fa[:, y, x], fb[:, y, x]
            la, lb = np.sqrt(np.dot(a, a)) + EPS, np.sqrt(np.dot(b, b)) + EPS
            total += sum(w[c] * (a[c] / la - b[c] / lb) ** 2 for c in range(C))
    return total / (h * wd)


def head_one_pass(fa, fb, w):
    """The expansion the kernel evaluates: five channel sums per pixel, then sum w a^2 / na^2 + sum w b^2 / nb^2 - 2 sum w a b / (na nb)."""
    fa, fb, w = np.asarray(fa, np.float64), np.asarray(fb, np.float64), np.asarray(w, np.float64).reshape(-1)[:, None, None]
    sa, sb = (fa * fa).sum(0), (fb * fb).sum(0)
    swa, swb, swab = (w * fa * fa).sum(0), (w * fb * fb).sum(0), (w * fa * fb).sum(0)
    na, nb = np.sqrt(sa) + EPS, np.sqrt(sb) + EPS
    return float((swa / (na * na) + swb / (nb * nb) - 2.0 * (swab / (na * nb))).mean())


def head_rows(features, lin_weights, head=head_two_pass):
    """features: list of (2B, C, h, w) arrays, rows [0, B) one batch and [B, 2B) the other -> (B, 6) float64 [LPIPS, d_0 .. d_4]."""
    B = features[0].shape[0] // 2
    rows = np.zeros((B, 6))
    for l, (f, w) in enumerate(zip(features, lin_weights)):
        f = np.asarray(f, np.float64)
        for i in range(B):
            rows[i, 1 + l] = head(f[i], f[B + i], w)
    rows[:, 0] = rows[:, 1:].sum(1)
    return rows


def float64_weights(model):
    """metrics.LPIPS object -> ([(weight, bias)] * 5, [w_l] * 5) as float64 CPU tensors / arrays."""
    return [(w.double(), b.double()) for w, b in model.conv_weights()], [w.double().numpy().reshape(-1) for w in model.lin_weights()]


def reference_rows(a, b, model, normalize):
    """a, b: (B, H, W, 3) arrays -> (B, 6) float64 rows of the whole metric, every step in float64 on the CPU."""
    convs, lins = float64_weights(model)
    x = torch.from_numpy(np.concatenate([scaling(a, normalize), scaling(b, normalize)]))
    with torch.no_grad():
        maps = [m.numpy() for m in feature_maps(x, convs)]
    return head_rows(maps, lins)


# ---- the same metric the way torch offers it, in the tensors' own precision (E_torch of the GPU tests; tools/time_lpips.py times it) ----
def torch_scaling(a, b, normalize):
    """a, b: (B, H, W, 3) uint8 or float32 tensors -> (2B, 3, H, W) float32, each step one torch operation (true divisions: the
    divisors are tensors)."""
    x = torch.cat([a, b])
    if x.dtype == torch.uint8:
        x = x.float() / torch.tensor(255.0, device=x.device)
    if normalize:
        x = 2.0 * x - 1.0
    shift, scale = torch.tensor(SHIFT, device=x.device), torch.tensor(SCALE, device=x.device)
    return ((x - shift) / scale).permute(0, 3, 1, 2).contiguous()


def torch_head(features, lin_weights):
    """The lpips package's head as torch writes it (normalize_tensor, squared difference, 1x1 convolution as a weighted channel sum,
    spatial mean) in the features' precision -> (B, 6)."""
    B = features[0].shape[0] // 2
    cols = []
    for f, w in zip(features, lin_weights):
        n = f / (torch.sqrt(torch.sum(f * f, dim=1, keepdim=True)) + EPS)
        d = (n[:B] - n[B:]) ** 2
        cols.append((d * w.reshape(1, -1, 1, 1)).sum(1).mean(dim=(1, 2)))
    cols = torch.stack(cols, 1)
    return torch.cat([cols.sum(1, keepdim=True), cols], 1)


# ---- inputs ----
def _finish(img, dtype):
    img = np.clip(img, 0.0, 1.0)
    return np.round(img * 255.0).astype(np.uint8) if dtype == np.uint8 else img.astype(np.float32)


def textured(H, W, seed):
    """Stripes, a ramp and noise in [0, 1], (H, W, 3) float64."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([0.5 + 0.3 * np.sin(0.9 * x + 0.4 * c + 0.1 * seed) * np.cos(0.5 * y - 0.3 * c) + 0.15 * (x / W - y / H) for c in range(3)], -1)
    return base + rng.normal(0.0, 0.05, (H, W, 3))


def textured_pair(H, W, dtype, seed=1):
    return _finish(textured(H, W, seed), dtype), _finish(textured(H, W, seed + 50), dtype)


def noisy_pair(H, W, dtype, seed=2):
    """An image and a copy with every value moved by up to +-20/255."""
    rng = np.random.default_rng(seed)
    a = textured(H, W, seed)
    return _finish(a, dtype), _finish(np.clip(a, 0, 1) + rng.integers(-20, 21, (H, W, 3)) / 255.0, dtype)


def pixel_pair(H, W, dtype, seed=3):
    """An image and a copy with ONE value, in the middle, changed by 1/255."""
    a = _finish(0.1 + 0.8 * np.clip(textured(H, W, seed), 0, 1), np.uint8)      # (inside [25, 230]: the change never saturates)
    b = a.copy()
    b[H // 2, W // 2, 1] += 1
    return (a, b) if dtype == np.uint8 else ((a / 255.0).astype(np.float32), (b / 255.0).astype(np.float32))


def identical_pair(H, W, dtype, seed=4):
    a = _finish(textured(H, W, seed), dtype)
    return a, a.copy()


def constant_region_pair(H, W, dtype, seed=5):
    """A textured pair whose left two thirds are black in both images (a constant region: with bias-free or negative-bias channels
    ReLU leaves whole pixels zero there)."""
    a, b = textured(H, W, seed), textured(H, W, seed + 50)
    a[:, :2 * W // 3], b[:, :2 * W // 3] = 0.0, 0.0
    return _finish(a, dtype), _finish(b, dtype)


def content(H, W, dtype):
    """The pairs of one shape, [(name, a, b)]."""
    return [("textured", *textured_pair(H, W, dtype)), ("noisy", *noisy_pair(H, W, dtype)), ("pixel", *pixel_pair(H, W, dtype)),
            ("identical", *identical_pair(H, W, dtype)), ("constant", *constant_region_pair(H, W, dtype))]


def synthetic_features(B, C, h, w, seed, zero_fraction=0.1):
    """A (2B, C, h, w) float32 feature tensor like a ReLU output (half its values zero) with different content per image; a fraction
    of the pixels is zero in every channel, in one operand or both.  And its (C,) non-negative channel weights, float32."""
    rng = np.random.default_rng(seed)
    f = np.maximum(rng.normal(0.0, 1.0, (2 * B, C, h, w)), 0.0) * rng.uniform(0.5, 4.0, (2 * B, 1, 1, 1))
    f[B:] = np.where(rng.random((B, C, h, w)) < 0.5, f[:B] * 1.01, f[B:])      # correlated operands, as an image and its copy give
    dead = rng.random((2 * B, 1, h, w)) < zero_fraction
    dead[0, 0, 0, 0] = True      # at least one all-zero pixel, and one that is zero in both operands
    dead[B, 0, 0, 0] = True
    f = np.where(dead, 0.0, f).astype(np.float32)
    return f, (rng.uniform(0.0, 2.0 / C, C)).astype(np.float32)
