"""Scoring produced frames against ground truth on the GPU (the reference's nerf/metrics.py: L1, PSNR and SSIM of scikit-image per
frame pair, their means, and a ``metrics.txt``).  The arithmetic is one fused HIP op (ops.image_metrics: two launches per batch, each
image read once); this module shapes its inputs and outputs.  LPIPS (net = alex, v0.1) is computed by an ``LPIPS`` object built from
the user's own two weight files -- torchvision's AlexNet state_dict and the lpips package's weights/v0.1/alex.pth, neither of which
ships here -- and handed to ``score_frames`` / ``two_folders`` as ``lpips=``; without one those two return and write what they always did.

Data ranges.  ``data_range`` (default 1.0, uint8 images being scored as x / 255) is the R of PSNR = 10 log10(R^2 / MSE), which is
``inf`` at MSE == 0 as scikit-image gives.  ``ssim_data_range`` is the R of SSIM's constants C1 = (0.01 R)^2, C2 = (0.03 R)^2 and
defaults to ``data_range``.  They are separate arguments because of a quirk of the reference: it calls scikit-image's SSIM on float
images divided by 255 WITHOUT a data range, and in the scikit-image versions that accept that call the range is then taken from the
dtype -- 2.0 for floats -- while its PSNR takes 1.0 for non-negative floats.  (From the published scikit-image source; the library is
not a dependency here, so this is not checked by a test.)  The default here is the standard 1.0 for both; pass ssim_data_range=2.0 to
reproduce figures that the reference's script printed.
"""
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib, ops, weights


class ScalarMetric(object):
    """The reference's running mean (nerf/metrics.py:22-44): update(x) adds an observation, peek() is the mean so far (0 before any)."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.value = []
        self.num_observations = 0.0
        self.aggregated_value = 0.0

    def __repr__(self):
        return str(self.peek())

    def update(self, x):
        self.aggregated_value += x
        self.num_observations += 1

    def peek(self):
        return self.aggregated_value / (self.num_observations if self.num_observations > 0 else 1)


def image_metrics(a, b, data_range=1.0, ssim_data_range=None, channels_last=True):
    """-> dict of float64 device tensors, scalars for one pair and (B,) for a batch: ssim, psnr, mse, l1, and ssim_channels (..., C).
    Arguments as ops.image_metrics."""
    row = ops.image_metrics(a, b, data_range, ssim_data_range, channels_last)
    mse = row[..., 1]
    return dict(ssim=row[..., 0], psnr=10.0 * torch.log10(float(data_range) ** 2 / mse), mse=mse, l1=row[..., 2], ssim_channels=row[..., 3:])


def ssim(a, b, data_range=1.0, channels_last=True):
    """Mean structural similarity (scikit-image's defaults, multichannel=True) at the SSIM data range ``data_range``."""
    return ops.image_metrics(a, b, data_range, None, channels_last)[..., 0]


def psnr(a, b, data_range=1.0, channels_last=True):
    return image_metrics(a, b, data_range, None, channels_last)["psnr"]


def l1(a, b, channels_last=True):
    """mean |a - b| (uint8: of x / 255)."""
    return ops.image_metrics(a, b, 1.0, None, channels_last)[..., 2]


def quantise(rgb):
    """evaluation.cast_to_image on the device: (..., 3) float -> uint8 (clamp, x255, truncate), what render_frames writes to the PNG."""
    return (rgb.detach().clamp(0.0, 1.0) * 255).to(torch.uint8)


def _frame(x, device):
    """One frame as a (H, W, C) tensor on the device: a render_frames result (its rgb[..., :3], quantised as its PNG is), or an image
    given as an array or tensor (uint8 or float32)."""
    if isinstance(x, dict):
        return quantise(x["rgb"][..., :3]).to(device)
    t = torch.as_tensor(x)
    if t.dtype not in (torch.uint8, torch.float32):
        raise _lib.SahsError("score_frames: frames must be torch.uint8 or torch.float32, got %s" % t.dtype)
    return t.to(device)


# torchvision's AlexNet ``features``: (index in the Sequential, out channels, in channels, kernel, stride, padding, max-pool 3/2 first)
ALEXNET_CONVS = ((0, 64, 3, 11, 4, 2, False), (3, 192, 64, 5, 1, 2, True), (6, 384, 192, 3, 1, 1, True), (8, 256, 384, 3, 1, 1, False),
                 (10, 256, 256, 3, 1, 1, False))
LPIPS_MIN_SIDE = ops.LPIPS_MIN_SIDE


def alexnet_features(x, conv_weights):
    """The five feature maps LPIPS reads: each convolution of torchvision's AlexNet ``features`` followed by its ReLU, a 3/2 max-pool
    ahead of the second and third.  x: (N, 3, H, W), already through the scaling layer; conv_weights: [(weight, bias)] * 5 in x's
    dtype and device -> list of five (N, C_l, h_l, w_l) tensors.  torch.nn.functional only (convolutions run on the vendor library:
    DESIGN section 9); also what the tests' float64 reference runs on the CPU."""
    if x.shape[-1] < LPIPS_MIN_SIDE or x.shape[-2] < LPIPS_MIN_SIDE:
        raise _lib.SahsError("LPIPS: images of %d x %d pixels, AlexNet's second max-pool needs %d <= H, W" % (x.shape[-2], x.shape[-1], LPIPS_MIN_SIDE))
    maps = []
    for (_, _, _, _, stride, pad, pool), (w, b) in zip(ALEXNET_CONVS, conv_weights):
        if pool:
            x = F.max_pool2d(x, 3, 2)
        x = F.relu(F.conv2d(x, w, b, stride=stride, padding=pad))
        maps.append(x)
    return maps


class LPIPS(object):
    """LPIPS, net = alex, version 0.1 (Zhang et al. 2018), restated from its published definition:
      1. scaling layer  x' = (x - shift) / scale per channel, shift = (-0.030, -0.088, -0.188), scale = (0.458, 0.448, 0.450);
      2. the five ReLU outputs of torchvision's AlexNet ``features`` (alexnet_features);
      3. per layer l, with channel weights w_l >= 0:  a^ = a / (sqrt(sum_c a_c^2) + 1e-10),
         d_l = mean over pixels of sum_c w_lc (a^_c - b^_c)^2;   LPIPS = sum_l d_l.
    Steps 1 and 3 are fused HIP ops (ops.lpips_prepare: one launch; ops.lpips_distance: two launches, float64 sums); step 2 is ten
    convolution / pool calls on 2B images at once, in fp32.

    ``normalize``.  The metric's authors feed images in [-1, 1]; their ``normalize=True`` maps [0, 1] images there (x -> 2x - 1) first.
    The reference calls ``lpips_fn(im / 255, im / 255)`` WITHOUT it (nerf/metrics.py:95-100), i.e. it scores [0, 1] images as if they
    were [-1, 1] ones.  The default here, False, is the reference's call and reproduces the figures its script printed; True is the
    metric as its authors define it.  (ssim_data_range above documents the reference's other quirk in the same way.)

    alexnet: a mapping with the keys ``features.{0,3,6,8,10}.{weight,bias}`` (torchvision's AlexNet state_dict; other keys, such as
    ``classifier.*``, are ignored); linear: a mapping with ``lin{0..4}.model.1.weight`` of shape (1, C_l, 1, 1) (the lpips package's
    weights/v0.1/alex.pth).  Either may be a path, read with torch.load(..., weights_only=True).  A missing key or a wrong shape is an
    error that names the key.  device: None, or the GPU the images will live on (others are then refused); the weights go there at the
    first call.  Building the object needs no GPU; scoring does (there is no CPU path).  Parity with the lpips package
    itself is the user's first check -- one image pair against their own install: neither the package nor its weights are available
    to this project's tests, which hold the arithmetic to a float64 restatement on synthetic weights (LPIPS.from_seed)."""

    def __init__(self, alexnet, linear, normalize=False, device=None):
        alexnet, linear = (torch.load(m, map_location="cpu", weights_only=True) if isinstance(m, (str, os.PathLike)) else m for m in (alexnet, linear))
        self.normalize, self.device, self._on_device = bool(normalize), device, None
        self.state = OrderedDict()
        for l, (idx, cout, cin, k, _, _, _) in enumerate(ALEXNET_CONVS):
            self._take(alexnet, "alexnet", "features.%d.weight" % idx, (cout, cin, k, k))
            self._take(alexnet, "alexnet", "features.%d.bias" % idx, (cout,))
            self._take(linear, "linear", "lin%d.model.1.weight" % l, (1, cout, 1, 1))

    def _take(self, mapping, which, key, shape):
        if key not in mapping:
            raise _lib.SahsError("LPIPS: %s has no key %r" % (which, key))
        t = torch.as_tensor(mapping[key]).detach().to("cpu", torch.float32).contiguous()
        if tuple(t.shape) != shape:
            raise _lib.SahsError("LPIPS: %s[%r] has shape %s, expected %s" % (which, key, tuple(t.shape), shape))
        self.state[key] = t
        return t

    @classmethod
    def from_seed(cls, seed=0, normalize=False, device=None):
        """Deterministic synthetic weights, for tests and timing (no real weights ship here): convolutions weights.hash_normal with He
        scaling sqrt(2 / fan_in), biases hashed uniform in +-1 / sqrt(fan_in), channel weights hashed uniform in [0, 2 / C_l)."""
        alexnet, linear = OrderedDict(), OrderedDict()
        for l, (idx, cout, cin, k, _, _, _) in enumerate(ALEXNET_CONVS):
            fan_in = cin * k * k
            alexnet["features.%d.weight" % idx] = torch.from_numpy(
                (weights.hash_normal(cout * fan_in, 3 * l, seed) * np.float32(np.sqrt(2.0 / fan_in))).reshape(cout, cin, k, k))
            alexnet["features.%d.bias" % idx] = torch.from_numpy(
                (weights.hash_uniform(cout, 3 * l + 1, seed) * np.float32(2.0) - np.float32(1.0)) * np.float32(1.0 / np.sqrt(fan_in)))
            linear["lin%d.model.1.weight" % l] = torch.from_numpy((weights.hash_uniform(cout, 3 * l + 2, seed) * np.float32(2.0 / cout)).reshape(1, cout, 1, 1))
        return cls(alexnet, linear, normalize, device)

    def conv_weights(self):
        """[(weight, bias)] * 5 as CPU float32 tensors."""
        return [(self.state["features.%d.weight" % idx], self.state["features.%d.bias" % idx]) for idx, *_ in ALEXNET_CONVS]

    def lin_weights(self):
        return [self.state["lin%d.model.1.weight" % l] for l in range(len(ALEXNET_CONVS))]

    def device_weights(self, device):
        if self._on_device is None or self._on_device[0] != device:
            self._on_device = (device, [(w.to(device), b.to(device)) for w, b in self.conv_weights()], [w.to(device) for w in self.lin_weights()])
        return self._on_device[1], self._on_device[2]

    def features(self, x):
        """x: (N, 3, H, W) float32 on the GPU, through the scaling layer (ops.lpips_prepare) -> the five feature tensors.  The
        convolutions run with torch.backends.cudnn.deterministic set for their duration: left to itself the vendor library picks, for
        the 1 x 1 .. 1 x 3 maps that small images leave the last two layers, kernels whose sums change from call to call (measured:
        DESIGN section 12), and then neither are two calls the same bits nor is the distance of an image to itself exactly 0."""
        want = None if self.device is None else torch.device(self.device)
        if want is not None and (want.type != x.device.type or want.index not in (None, x.device.index)):
            raise _lib.SahsError("LPIPS: built for %s, the images live on %s" % (torch.device(self.device), x.device))
        convs, _ = self.device_weights(x.device)
        before = torch.backends.cudnn.deterministic
        torch.backends.cudnn.deterministic = True
        try:
            with torch.no_grad(), torch.autocast("cuda", enabled=False):
                return alexnet_features(x, convs)
        finally:
            torch.backends.cudnn.deterministic = before

    def loss(self, pred, target, clamp=True, channels_last=False, return_rows=False):
        """LPIPS as a training term -> a 0-d float32 tensor, the mean over the batch, differentiable with respect to ``pred`` only.
        pred: float32 GPU tensor (3, H, W) or (B, 3, H, W) (channels_last=True: (H, W, 3) or (B, H, W, 3)), a generator's output;
        target: the same shape, uint8 or float32, and no gradient.  clamp=True scores pred.clamp(0, 1), as the metric scores the frame.
        The steps: ops.lpips_prepare_loss (one launch, the clamp inside); alexnet_features of pred's B images with autograd on and of
        target's B images under no_grad -- two calls, so that the convolution backward runs over B images and not 2B; the convolution
        weights are plain tensors, so no weight gradients are formed --; ops.lpips_head (two launches, and one launch backward).
        Both feature calls run in the vendor library's deterministic mode and outside autocast, as ``features`` does.  The convolution
        BACKWARD runs later, inside the caller's backward(), under whatever mode the caller has set then: bit-reproducibility is
        promised for the two fused ends, and for the whole gradient only if the caller sets the deterministic mode around backward().
        A feature pixel that ReLU left all zero has a finite gradient here (autograd of the published formula gives NaN there).
        return_rows=True: (loss, rows), rows the detached float64 (B, 6) [LPIPS, d_0 .. d_4] of ``layers``."""
        if not torch.cuda.is_available():
            raise _lib.SahsError("LPIPS: the loss needs a GPU (the HIP path has no CPU fallback)")
        x_pred, x_target = ops.lpips_prepare_loss(pred, target, clamp, self.normalize, channels_last)
        want = None if self.device is None else torch.device(self.device)
        if want is not None and (want.type != x_pred.device.type or want.index not in (None, x_pred.device.index)):
            raise _lib.SahsError("LPIPS: built for %s, the images live on %s" % (torch.device(self.device), x_pred.device))
        convs, lins = self.device_weights(x_pred.device)
        before = torch.backends.cudnn.deterministic
        torch.backends.cudnn.deterministic = True
        try:
            with torch.autocast("cuda", enabled=False):
                fa = alexnet_features(x_pred, convs)
                with torch.no_grad():
                    fb = alexnet_features(x_target, convs)
        finally:
            torch.backends.cudnn.deterministic = before
        per_image, rows = ops.lpips_head(fa, fb, lins)
        loss = per_image.mean()
        return (loss, rows) if return_rows else loss

    def layers(self, a, b, channels_last=True):
        """-> float64 device tensor (6,) for one pair, (B, 6) for a batch: [LPIPS, d_0 .. d_4].  a, b as ops.lpips_prepare takes them."""
        if not torch.cuda.is_available():
            raise _lib.SahsError("LPIPS: scoring needs a GPU (the HIP path has no CPU fallback)")
        batched = isinstance(a, torch.Tensor) and a.dim() == 4
        x = ops.lpips_prepare(a, b, self.normalize, channels_last)
        rows = ops.lpips_distance(self.features(x), self.device_weights(x.device)[1])
        return rows if batched else rows[0]

    def __call__(self, a, b, channels_last=True):
        """-> LPIPS as a float64 device tensor: a scalar for one pair, (B,) for a batch."""
        return self.layers(a, b, channels_last)[..., 0]


def score_frames(predicted, targets, data_range=1.0, ssim_data_range=None, channels_last=True, batch=8, device=None, lpips=None):
    """Per-frame and mean scores of ``predicted`` against ``targets``, two sequences (or batched tensors) of frames of one size.
    predicted: what evaluation.render_frames returned (dicts: rgb[..., :3] is clamped and quantised as cast_to_image does, so the
    score is that of the PNG it wrote) or generator outputs / images (tensors or arrays; channels_last=False for (C, H, W)); targets:
    images of the same layout.  A pair of one uint8 and one float32 frame is scored as float32 in [0, 1] (the uint8 side x / 255).
    -> dict: per-frame float64 device tensors ssim, psnr, mse, l1 of length N, and their means mean_ssim, mean_psnr, mean_l1 (floats;
    the mean PSNR is that of the per-frame PSNRs, as the reference averages).  Frames are scored ``batch`` at a time.
    lpips: an ``LPIPS`` object, or None; with one the result gains ``lpips`` (per frame) and ``mean_lpips``, of the same frames (the
    quantised uint8 of a render_frames dict) in the same batches."""
    if len(predicted) != len(targets):
        raise _lib.SahsError("score_frames: %d predicted frames, %d targets" % (len(predicted), len(targets)))
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    rows, lp = [], []
    for i in range(0, len(predicted), max(int(batch), 1)):
        p = [_frame(x, device) for x in predicted[i:i + batch]]
        t = [_frame(x, device) for x in targets[i:i + batch]]
        pa, ta = torch.stack(p), torch.stack(t)
        if pa.dtype != ta.dtype:
            pa, ta = (x.float() / 255 if x.dtype == torch.uint8 else x for x in (pa, ta))
        rows.append(ops.image_metrics(pa, ta, data_range, ssim_data_range, channels_last))
        if lpips is not None:
            lp.append(lpips(pa, ta, channels_last))
    rows = torch.cat(rows) if rows else torch.zeros(0, 4, dtype=torch.float64, device=device)
    out = dict(ssim=rows[:, 0], mse=rows[:, 1], l1=rows[:, 2], psnr=10.0 * torch.log10(float(data_range) ** 2 / rows[:, 1]))
    for k in ("ssim", "psnr", "l1"):
        out["mean_" + k] = float(out[k].mean()) if len(rows) else 0.0
    if lpips is not None:
        out["lpips"] = torch.cat(lp) if lp else torch.zeros(0, dtype=torch.float64, device=device)
        out["mean_lpips"] = float(out["lpips"].mean()) if len(rows) else 0.0
    return out


def _frame_number(name):
    digits = "".join(filter(str.isdigit, name))
    if not digits:
        raise _lib.SahsError("two_folders: %r has no digits to sort by" % name)
    return int(digits)


def pair_png_names(names_gt, names_generated):
    """The reference's pairing (nerf/metrics.py:120-134) on file names alone: keep the names whose first extension is png, sort both
    lists by the number their digits spell, require generated <= ground truth, and pair them in order -> [(gt, generated)]."""
    def pngs(names):
        return sorted((n for n in names if len(n.split(".")) > 1 and n.split(".")[1] == "png"), key=_frame_number)
    gt, gen = pngs(names_gt), pngs(names_generated)
    if len(gen) > len(gt):
        raise _lib.SahsError("two_folders: %d generated images but only %d ground-truth images" % (len(gen), len(gt)))
    return list(zip(gt, gen))


def frame_lines(name, l1, psnr, ssim, lpips=None):
    """The lines metrics.txt holds for one generated frame (nerf/metrics.py:164-167); without ``lpips`` the layout without its line."""
    text = name + "   L1:  \t%5f \n" % l1 + name + "   PSNR:\t%5f \n" % psnr
    if lpips is None:
        return text + name + "   SSIM:\t%5f \n\n" % ssim
    return text + name + "   SSIM:\t%5f \n" % ssim + name + "   LPIPS:\t%5f\n\n" % lpips


def summary_lines(path_gt, path_generated, l1, psnr, ssim, lpips=None):
    """The summary that ends metrics.txt (nerf/metrics.py:169-175; "mean LPIPS" has no colon there)."""
    text = "=" * 80 + "\n Summary \n folder 1: %s \n folder 2: %s \n" % (path_gt, path_generated) + "-" * 80
    text += "\n mean L1:\t%5f" % l1 + "\n mean PSNR:\t%5f" % psnr
    if lpips is None:
        return text + "\n mean SSIM:\t%5f\n" % ssim
    return text + "\n mean SSIM:\t%5f" % ssim + "\n mean LPIPS\t%5f\n" % lpips


def two_folders(path_gt, path_generated, data_range=1.0, ssim_data_range=None, batch=8, log=print, lpips=None):
    """Score the PNGs of ``path_generated`` against those of ``path_gt`` (paired as pair_png_names does) in batches on the GPU and write
    ``path_generated/metrics.txt`` in the reference's line layout: with ``lpips`` (an ``LPIPS`` object) its complete layout, without
    one the layout minus its LPIPS lines.  Images are read with PIL and scored as uint8 (x / 255).
    -> dict(names, l1, psnr, ssim: per-pair lists; mean_l1, mean_psnr, mean_ssim; with ``lpips`` also lpips and mean_lpips)."""
    from PIL import Image
    listing = {p: [f for f in os.listdir(p) if os.path.isfile(os.path.join(p, f))] for p in (path_gt, path_generated)}
    pairs = pair_png_names(listing[path_gt], listing[path_generated])
    log("Detected %d images in GT folder          %s" % (sum(1 for n in listing[path_gt] if n.split(".")[1:2] == ["png"]), path_gt))
    log("Detected %d images in Generated folder   %s" % (len(pairs), path_generated))
    keys = ("l1", "psnr", "ssim") + (("lpips",) if lpips is not None else ())
    means = {key: ScalarMetric() for key in keys}
    res = dict(names=[g for _, g in pairs], **{key: [] for key in keys})
    with open(os.path.join(path_generated, "metrics.txt"), "w") as fo:
        for i in range(0, len(pairs), max(int(batch), 1)):
            chunk = pairs[i:i + batch]
            real = [np.atleast_3d(np.array(Image.open(os.path.join(path_gt, g)))) for g, _ in chunk]
            fake = [np.atleast_3d(np.array(Image.open(os.path.join(path_generated, f)))) for _, f in chunk]
            for (g, f), r, k in zip(chunk, real, fake):
                if r.shape != k.shape or r.dtype != np.uint8 or k.dtype != np.uint8:
                    raise _lib.SahsError("two_folders: %s is %s %s, %s is %s %s: pairs must be 8-bit images of one size"
                                         % (g, r.shape, r.dtype, f, k.shape, k.dtype))
            # one call for the chunk; where the sizes differ between its pairs, one call each
            scores = score_frames(fake, real, data_range, ssim_data_range, batch=len(chunk) if len(set(r.shape for r in real)) == 1 else 1,
                                  lpips=lpips)
            for j, (_, f) in enumerate(chunk):
                cur = {key: float(scores[key][j]) for key in keys}
                for key in keys:
                    means[key].update(cur[key])
                    res[key].append(cur[key])
                fo.write(frame_lines(f, **cur))
        fo.write(summary_lines(path_gt, path_generated, **{key: means[key].peek() for key in keys}))
    res.update({"mean_" + key: means[key].peek() for key in keys})
    log("mean L1:\t%5f\nmean PSNR:\t%5f\nmean SSIM:\t%5f" % (res["mean_l1"], res["mean_psnr"], res["mean_ssim"]))
    if lpips is not None:
        log("mean LPIPS\t%5f" % res["mean_lpips"])
    return res
