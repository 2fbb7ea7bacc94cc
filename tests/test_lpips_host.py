"""CPU-side checks of LPIPS in the product: metrics.LPIPS takes the two public weight files' layouts and names what is wrong with a
bad one, LPIPS.from_seed is deterministic, the C entries refuse bad arguments before any HIP call, scoring has no CPU path, and the
lines of metrics.txt with LPIPS are the reference's (nerf/metrics.py:164-175), character for character."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import lpips_reference as R
from conftest import REPO, pkg

FAKE = 0x10000      # a non-null, 8-byte-aligned address that is never dereferenced: every call below is refused before any HIP call


def torchvision_style(seed=0):
    """State dicts laid out like torchvision's AlexNet (with its classifier) and the lpips package's alex.pth."""
    M = pkg("metrics")
    model = M.LPIPS.from_seed(seed)
    alexnet = {k: v.clone() for k, v in model.state.items() if k.startswith("features.")}
    alexnet.update({"classifier.1.weight": torch.zeros(8, 8), "classifier.1.bias": torch.zeros(8)})
    linear = {k: v.clone() for k, v in model.state.items() if k.startswith("lin")}
    return model, alexnet, linear


def test_constants_are_the_headers():
    text = open(os.path.join(REPO, "include", "sahs_nerf.h")).read()
    ops = pkg("ops")
    for name, value in (("TILE", ops.LPIPS_TILE), ("MAX_JOBS", ops.LPIPS_MAX_JOBS), ("MAX_CHANNELS", ops.LPIPS_MAX_CHANNELS), ("MIN_SIDE", ops.LPIPS_MIN_SIDE)):
        assert int(re.search(r"#define SAHS_LPIPS_%s (\d+)" % name, text).group(1)) == value, name
    assert R.TILE == ops.LPIPS_TILE and R.MIN_SIDE == ops.LPIPS_MIN_SIDE == pkg("metrics").LPIPS_MIN_SIDE
    assert [c[1:] for c in pkg("metrics").ALEXNET_CONVS] == list(R.CONVS)


def test_accepts_the_public_layouts(tmp_path):
    M = pkg("metrics")
    model, alexnet, linear = torchvision_style()
    built = M.LPIPS(alexnet, linear, normalize=True)
    assert built.normalize and list(built.state) == list(model.state) and not any(k.startswith("classifier") for k in built.state)
    assert all(torch.equal(built.state[k], model.state[k]) and built.state[k].dtype == torch.float32 for k in model.state)
    # numpy arrays and float64 values are taken too, as float32; paths are read with torch.load(weights_only=True)
    as_np = M.LPIPS({k: v.double().numpy() for k, v in alexnet.items()}, linear)
    assert all(torch.equal(as_np.state[k], model.state[k]) for k in model.state)
    torch.save(alexnet, tmp_path / "alexnet.pth")
    torch.save(linear, tmp_path / "alex.pth")
    loaded = M.LPIPS(str(tmp_path / "alexnet.pth"), tmp_path / "alex.pth")
    assert all(torch.equal(loaded.state[k], model.state[k]) for k in model.state) and not loaded.normalize
    assert [tuple(w.shape) for w, _ in loaded.conv_weights()] == [(co, ci, k, k) for co, ci, k, _, _, _ in R.CONVS]
    assert [tuple(w.shape) for w in loaded.lin_weights()] == [(1, c[0], 1, 1) for c in R.CONVS]


def test_names_the_missing_or_misshaped_key():
    M, lib = pkg("metrics"), pkg("_lib")
    _, alexnet, linear = torchvision_style()
    for key in ("features.0.weight", "features.6.bias", "features.10.weight"):
        with pytest.raises(lib.SahsError, match="alexnet has no key %r" % key):
            M.LPIPS({k: v for k, v in alexnet.items() if k != key}, linear)
    with pytest.raises(lib.SahsError, match="linear has no key 'lin3.model.1.weight'"):
        M.LPIPS(alexnet, {k: v for k, v in linear.items() if k != "lin3.model.1.weight"})
    bad = dict(alexnet, **{"features.3.weight": torch.zeros(192, 64, 3, 3)})
    with pytest.raises(lib.SahsError, match=r"alexnet\['features.3.weight'\] has shape \(192, 64, 3, 3\), expected \(192, 64, 5, 5\)"):
        M.LPIPS(bad, linear)
    bad = dict(linear, **{"lin2.model.1.weight": torch.zeros(384)})
    with pytest.raises(lib.SahsError, match=r"linear\['lin2.model.1.weight'\] has shape \(384,\), expected \(1, 384, 1, 1\)"):
        M.LPIPS(alexnet, bad)
    with pytest.raises(lib.SahsError, match=r"alexnet\['features.8.bias'\] has shape \(384,\), expected \(256,\)"):
        M.LPIPS(dict(alexnet, **{"features.8.bias": torch.zeros(384)}), linear)


def test_from_seed_is_deterministic_and_non_negative():
    M = pkg("metrics")
    a, b, c = M.LPIPS.from_seed(3), M.LPIPS.from_seed(3), M.LPIPS.from_seed(4)
    assert all(torch.equal(a.state[k], b.state[k]) for k in a.state) and any(not torch.equal(a.state[k], c.state[k]) for k in a.state)
    for l, w in enumerate(a.lin_weights()):
        C = R.CONVS[l][0]
        assert bool((w >= 0).all()) and float(w.max()) <= 2.0 / C and float(w.max()) > 1.0 / C
    for (w, bias), (_, cin, k, _, _, _) in zip(a.conv_weights(), R.CONVS):      # He scaling: variance 2 / fan_in
        assert abs(float(w.double().var()) * cin * k * k / 2.0 - 1.0) < 0.1 and float(bias.abs().max()) <= (cin * k * k) ** -0.5
    # the float64 reference on these weights: a sensible metric (the GPU tests' yardstick is not degenerate)
    rows = np.concatenate([R.reference_rows(x[None], y[None], a, False) for _, x, y in R.content(31, 31, np.uint8)])
    names = [n for n, _, _ in R.content(31, 31, np.uint8)]
    assert rows[names.index("identical"), 0] == 0.0 and 0.0 < rows[names.index("pixel"), 0] < rows[names.index("noisy"), 0] < rows[names.index("textured"), 0]
    assert np.all(rows[names.index("textured"), 1:] > 0.0)


def test_scoring_has_no_cpu_path():
    M, ops, lib = pkg("metrics"), pkg("ops"), pkg("_lib")
    a = torch.zeros(31, 31, 3)
    with pytest.raises(lib.SahsError, match="GPU"):
        M.LPIPS.from_seed(0)(a, a)
    with pytest.raises(lib.SahsError, match="a must be a GPU tensor"):
        ops.lpips_prepare(a, a)
    with pytest.raises(lib.SahsError, match=r"features\[0\] must be a GPU tensor"):
        ops.lpips_distance([torch.zeros(2, 4, 3, 3)], [torch.zeros(4)])
    with pytest.raises(lib.SahsError, match="1 .. 5 layers"):
        ops.lpips_distance([torch.zeros(2, 4, 3, 3)] * 6, [torch.zeros(4)] * 6)


def _prepare(L, a=FAKE, b=FAKE, dtype=0, B=1, H=31, W=31, C=3, sa=True, sb=True, out=FAKE):
    strides = (ctypes.c_long * 4)(H * W * C, W * C, C, 1)
    return L.sahs_lpips_prepare(a, b, dtype, B, H, W, C, strides if sa else None, strides if sb else None, 0, out, None)


def _distance(L, jobs=2, f=(FAKE, FAKE), w=(FAKE, FAKE), C=(64, 192), hw=(49, 9), B=1, out=FAKE, work=FAKE, work_bytes=None, tables=True):
    n = len(C)
    fp, wp = (ctypes.c_void_p * n)(*f), (ctypes.c_void_p * n)(*w)
    Cs, hws = (ctypes.c_int * n)(*C), (ctypes.c_long * n)(*hw)
    if work_bytes is None:
        work_bytes = L.sahs_lpips_distance_workspace_bytes(jobs, B, hws)
    return L.sahs_lpips_distance(jobs, fp if tables else None, wp, Cs, hws, B, out, work, work_bytes, None)


def test_c_abi_refuses_before_any_hip_call():
    L = pkg("_lib").lib()
    T = R.TILE
    hw = (ctypes.c_long * 5)(1, T - 16, T, T + 16, 961)
    assert L.sahs_lpips_distance_workspace_bytes(5, 1, hw) == (1 + 1 + 1 + 2 + 4) * 8
    assert L.sahs_lpips_distance_workspace_bytes(5, 3, hw) == 3 * 9 * 8 and L.sahs_lpips_distance_workspace_bytes(2, 3, hw) == 3 * 2 * 8
    for bad in ((0, 1, hw), (6, 1, hw), (5, -1, hw), (5, 1, None), (1, 1, (ctypes.c_long * 1)(0))):
        assert L.sahs_lpips_distance_workspace_bytes(*bad) == 0, bad
    cases = {"C = 4": dict(C=4), "C = 1": dict(C=1), "dtype = 2": dict(dtype=2), "30 x 64": dict(H=30, W=64), "64 x 30": dict(H=64, W=30),
             "for a ": dict(a=None), "for b ": dict(b=None), "for stride_a": dict(sa=False), "for stride_b": dict(sb=False), "for out": dict(out=None),
             "B = -1": dict(B=-1), "4-byte": dict(dtype=1, a=FAKE + 2)}
    for text, kw in cases.items():
        code = _prepare(L, **kw)
        msg = L.sahs_last_error().decode()
        assert code == 1 and msg.startswith("sahs_lpips_prepare:") and text in msg, (kw, code, msg)
    assert _prepare(L, B=0, a=None, b=None, out=None) == 0      # nothing to prepare: success without a launch
    cases = {"jobs = 6": dict(jobs=6, f=(FAKE,) * 6, w=(FAKE,) * 6, C=(4,) * 6, hw=(4,) * 6), "jobs = 0": dict(jobs=0),
             "job 1 has C = 0": dict(C=(64, 0)), "job 0 has C = 1025": dict(C=(1025, 4)), "job 1 has hw = 0": dict(hw=(49, 0)),
             "B = -1": dict(B=-1), "for features": dict(tables=False), "features[1]": dict(f=(FAKE, None)), "weights[0]": dict(w=(None, FAKE)),
             "for out": dict(out=None), "for workspace": dict(work=None), "needs 16": dict(work_bytes=15), "8-byte aligned": dict(out=FAKE + 4),
             "4-byte elements": dict(f=(FAKE + 2, FAKE))}
    for text, kw in cases.items():
        code = _distance(L, **kw)
        msg = L.sahs_last_error().decode()
        assert code == 1 and msg.startswith("sahs_lpips_distance:") and text in msg, (kw, code, msg)
    assert _distance(L, B=0, out=None, work=None) == 0


def test_metrics_txt_lines_are_the_references():
    """nerf/metrics.py:164-175, its format strings restated literally."""
    M = pkg("metrics")
    name, l1, psnr, ssim, lp = "12_fake.png", 0.0123456789, 31.4159265, 0.98765432, 0.0456789
    want = (name + '   L1:  \t%5f \n' % l1 + name + '   PSNR:\t%5f \n' % psnr + name + '   SSIM:\t%5f \n' % ssim
            + name + '   LPIPS:\t%5f\n\n' % lp)
    assert M.frame_lines(name, l1, psnr, ssim, lp) == want
    assert want == "12_fake.png   L1:  \t0.012346 \n12_fake.png   PSNR:\t31.415927 \n12_fake.png   SSIM:\t0.987654 \n12_fake.png   LPIPS:\t0.045679\n\n"
    want = ('=' * 80 + '\n Summary \n folder 1: %s \n folder 2: %s \n' % ("gt", "gen") + '-' * 80 + "\n mean L1:\t%5f" % l1
            + "\n mean PSNR:\t%5f" % psnr + "\n mean SSIM:\t%5f" % ssim + "\n mean LPIPS\t%5f\n" % lp)
    assert M.summary_lines("gt", "gen", l1, psnr, ssim, lp) == want and want.endswith("\n mean SSIM:\t0.987654\n mean LPIPS\t0.045679\n")
    # without LPIPS: the layout the function has always written (SSIM closes the frame's block; the summary ends after SSIM)
    assert M.frame_lines(name, l1, psnr, ssim) == (name + "   L1:  \t%5f \n" % l1 + name + "   PSNR:\t%5f \n" % psnr + name + "   SSIM:\t%5f \n\n" % ssim)
    assert M.summary_lines("gt", "gen", l1, psnr, ssim) == ("=" * 80 + "\n Summary \n folder 1: gt \n folder 2: gen \n" + "-" * 80
                                                          + "\n mean L1:\t%5f" % l1 + "\n mean PSNR:\t%5f" % psnr + "\n mean SSIM:\t%5f\n" % ssim)
