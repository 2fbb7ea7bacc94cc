"""Scoring produced frames against ground truth on the GPU (the reference's nerf/metrics.py: L1, PSNR and SSIM of scikit-image per
frame pair, their means, and a ``metrics.txt``).  The arithmetic is one fused HIP op (ops.image_metrics: two launches per batch, each
image read once); this module shapes its inputs and outputs.  LPIPS is not computed: it needs AlexNet weights.

Data ranges.  ``data_range`` (default 1.0, uint8 images being scored as x / 255) is the R of PSNR = 10 log10(R^2 / MSE), which is
``inf`` at MSE == 0 as scikit-image gives.  ``ssim_data_range`` is the R of SSIM's constants C1 = (0.01 R)^2, C2 = (0.03 R)^2 and
defaults to ``data_range``.  They are separate arguments because of a quirk of the reference: it calls scikit-image's SSIM on float
images divided by 255 WITHOUT a data range, and in the scikit-image versions that accept that call the range is then taken from the
dtype -- 2.0 for floats -- while its PSNR takes 1.0 for non-negative floats.  (From the published scikit-image source; the library is
not a dependency here, so this is not checked by a test.)  The default here is the standard 1.0 for both; pass ssim_data_range=2.0 to
reproduce figures that the reference's script printed.
"""
import os

import torch

from . import _lib, ops


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


def score_frames(predicted, targets, data_range=1.0, ssim_data_range=None, channels_last=True, batch=8, device=None):
    """Per-frame and mean scores of ``predicted`` against ``targets``, two sequences (or batched tensors) of frames of one size.
    predicted: what evaluation.render_frames returned (dicts: rgb[..., :3] is clamped and quantised as cast_to_image does, so the
    score is that of the PNG it wrote) or generator outputs / images (tensors or arrays; channels_last=False for (C, H, W)); targets:
    images of the same layout.  A pair of one uint8 and one float32 frame is scored as float32 in [0, 1] (the uint8 side x / 255).
    -> dict: per-frame float64 device tensors ssim, psnr, mse, l1 of length N, and their means mean_ssim, mean_psnr, mean_l1 (floats;
    the mean PSNR is that of the per-frame PSNRs, as the reference averages).  Frames are scored ``batch`` at a time."""
    if len(predicted) != len(targets):
        raise _lib.SahsError("score_frames: %d predicted frames, %d targets" % (len(predicted), len(targets)))
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    rows = []
    for i in range(0, len(predicted), max(int(batch), 1)):
        p = [_frame(x, device) for x in predicted[i:i + batch]]
        t = [_frame(x, device) for x in targets[i:i + batch]]
        pa, ta = torch.stack(p), torch.stack(t)
        if pa.dtype != ta.dtype:
            pa, ta = (x.float() / 255 if x.dtype == torch.uint8 else x for x in (pa, ta))
        rows.append(ops.image_metrics(pa, ta, data_range, ssim_data_range, channels_last))
    rows = torch.cat(rows) if rows else torch.zeros(0, 4, dtype=torch.float64, device=device)
    out = dict(ssim=rows[:, 0], mse=rows[:, 1], l1=rows[:, 2], psnr=10.0 * torch.log10(float(data_range) ** 2 / rows[:, 1]))
    for k in ("ssim", "psnr", "l1"):
        out["mean_" + k] = float(out[k].mean()) if len(rows) else 0.0
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


def two_folders(path_gt, path_generated, data_range=1.0, ssim_data_range=None, batch=8, log=print):
    """Score the PNGs of ``path_generated`` against those of ``path_gt`` (paired as pair_png_names does) in batches on the GPU and write
    ``path_generated/metrics.txt`` in the reference's line layout, without its LPIPS lines.  Images are read with PIL and scored as
    uint8 (x / 255).  -> dict(names, l1, psnr, ssim: per-pair lists; mean_l1, mean_psnr, mean_ssim)."""
    import numpy as np
    from PIL import Image
    listing = {p: [f for f in os.listdir(p) if os.path.isfile(os.path.join(p, f))] for p in (path_gt, path_generated)}
    pairs = pair_png_names(listing[path_gt], listing[path_generated])
    log("Detected %d images in GT folder          %s" % (sum(1 for n in listing[path_gt] if n.split(".")[1:2] == ["png"]), path_gt))
    log("Detected %d images in Generated folder   %s" % (len(pairs), path_generated))
    L1, PSNR, SSIM = ScalarMetric(), ScalarMetric(), ScalarMetric()
    res = dict(names=[g for _, g in pairs], l1=[], psnr=[], ssim=[])
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
            scores = score_frames(fake, real, data_range, ssim_data_range, batch=len(chunk) if len(set(r.shape for r in real)) == 1 else 1)
            for j, (_, f) in enumerate(chunk):
                cur = {key: float(scores[key][j]) for key in ("l1", "psnr", "ssim")}
                L1.update(cur["l1"])
                PSNR.update(cur["psnr"])
                SSIM.update(cur["ssim"])
                for key in cur:
                    res[key].append(cur[key])
                fo.write(f + "   L1:  \t%5f \n" % cur["l1"])
                fo.write(f + "   PSNR:\t%5f \n" % cur["psnr"])
                fo.write(f + "   SSIM:\t%5f \n\n" % cur["ssim"])
        fo.write("=" * 80)
        fo.write("\n Summary \n folder 1: %s \n folder 2: %s \n" % (path_gt, path_generated))
        fo.write("-" * 80)
        fo.write("\n mean L1:\t%5f" % L1.peek())
        fo.write("\n mean PSNR:\t%5f" % PSNR.peek())
        fo.write("\n mean SSIM:\t%5f\n" % SSIM.peek())
    res.update(mean_l1=L1.peek(), mean_psnr=PSNR.peek(), mean_ssim=SSIM.peek())
    log("mean L1:\t%5f\nmean PSNR:\t%5f\nmean SSIM:\t%5f" % (res["mean_l1"], res["mean_psnr"], res["mean_ssim"]))
    return res
