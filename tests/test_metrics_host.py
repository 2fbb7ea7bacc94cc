"""CPU-side checks of the image metrics: the two float64 references agree, closed forms hold, a single wrong pixel anywhere moves the
references by far more than the GPU tests' tolerances (so those cannot pass with a dropped halo or an unowned pixel), the C entry
refuses bad arguments before any HIP call, and the host-side pieces of metrics.py (ScalarMetric, the pairing of file names)."""
import ctypes
import os
import re

import numpy as np
import pytest

import metrics_reference as R
from conftest import REPO, pkg

FAKE = 0x10000      # a non-null, 8-byte-aligned address that is never dereferenced: every call below is refused before any HIP call


def test_tile_edge_is_the_headers():
    text = open(os.path.join(REPO, "include", "sahs_nerf.h")).read()
    assert int(re.search(r"#define SAHS_IMAGE_METRICS_TILE (\d+)", text).group(1)) == R.TILE == pkg("ops").IMAGE_METRICS_TILE


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_the_two_references_agree(dtype):
    worst = 0.0
    for H, W in R.SHAPES:
        for C in (1, 3):
            for name, a, b in R.content(H, W, C, dtype):
                for rng in (1.0, 2.0):
                    d = np.abs(R.ssim_direct(a, b, rng) - R.ssim_filtered(a, b, rng)).max()
                    worst = max(worst, d)
                    assert d <= 1e-12, (H, W, C, name, rng, d)
    print("direct vs filtered float64 SSIM: worst difference %.2e" % worst)


def test_content_spans_the_ssim_range():
    s = {name: R.ssim_direct(a, b).mean() for name, a, b in R.content(45, 71, 3, np.float32)}
    assert s["noise0.005"] > 0.97 and 0.2 < s["noise0.07"] < 0.4 and s["inverted"] < 0.0 and s["identical"] == 1.0, s


def test_closed_forms():
    a, _ = R.ramp_noise_pair(20, 23, 3, 0.1, 1, np.uint8)
    row = R.reference_row(a, a)
    assert row[0] == 1.0 and row[1] == 0.0 and row[2] == 0.0 and np.isinf(R.psnr(row[1]))
    for rng in (1.0, 2.0):
        p, q = 64 / 255, 191 / 255
        a, b = R.constant_pair(9, 12, 2, p, q, np.uint8)
        C1 = (0.01 * rng) ** 2
        want = (2 * p * q + C1) / (p * p + q * q + C1)
        for f in (R.ssim_direct, R.ssim_filtered):
            assert np.abs(f(a, b, rng) - want).max() < 1e-13
        row = R.reference_row(a, b, rng)
        assert abs(row[1] - (p - q) ** 2) < 1e-15 and abs(row[2] - (q - p)) < 1e-15
    # a 7x7 image is one window
    a, b = R.ramp_noise_pair(7, 7, 1, 0.1, 3, np.float32)
    x, y = a[:, :, 0].astype(np.float64).ravel(), b[:, :, 0].astype(np.float64).ravel()
    cov = np.cov(x, y, ddof=1)
    want = ((2 * x.mean() * y.mean() + 1e-4) * (2 * cov[0, 1] + 9e-4)) / ((x.mean() ** 2 + y.mean() ** 2 + 1e-4) * (cov[0, 0] + cov[1, 1] + 9e-4))
    assert abs(R.ssim_direct(a, b)[0] - want) < 1e-13
    assert abs(R.psnr(0.01) - 20.0) < 1e-12 and abs(R.psnr(0.01, 2.0) - (20.0 + 20 * np.log10(2.0))) < 1e-12


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_one_wrong_pixel_moves_the_references(dtype):
    """The GPU tolerances are 2^-19 absolute for SSIM (uint8; the fp32 floor is 2^-20) and 1e-12 / 2^-20 relative for MSE and L1: a
    pixel that is off by the whole range -- in the first corner, the last corner or on a tile seam -- moves each figure by more than
    100 times that, at every shape of the GPU list."""
    for H, W in R.SHAPES:
        for C in (1, 3):
            for pos in R.single_pixel_positions(H, W):
                a, b = R.single_pixel_pair(H, W, C, pos, dtype)
                good, bad = R.reference_row(a, a), R.reference_row(a, b)
                assert np.all(np.abs(good[[0] + list(range(3, 3 + C))] - bad[[0] + list(range(3, 3 + C))]) > 100 * 2.0 ** -19), (H, W, C, pos, bad)
                # against a pair that already differs (MSE, L1 > 0) the one pixel is a relative change far above 100 * 2^-20
                a2, b2 = R.ramp_noise_pair(H, W, C, 0.05, 9, dtype)
                base = R.reference_row(a2, b2)
                b3 = b2.copy()
                b3[pos[0], pos[1], :] = np.where(a2[pos[0], pos[1], :] > (127 if dtype == np.uint8 else 0.5), 0, 255 if dtype == np.uint8 else 1.0)
                moved = R.reference_row(a2, b3)
                assert abs(moved[1] - base[1]) / base[1] > 100 * 2.0 ** -20 and abs(moved[2] - base[2]) / base[2] > 100 * 2.0 ** -20, (H, W, C, pos)


def _call(L, a=FAKE, b=FAKE, dtype=0, B=1, H=16, W=16, C=3, sa=True, sb=True, rng=1.0, out=FAKE, work=FAKE, work_bytes=None):
    strides = (ctypes.c_long * 4)(H * W * C, W * C, C, 1)
    if work_bytes is None:
        work_bytes = L.sahs_image_metrics_workspace_bytes(B, H, W, C)
    return L.sahs_image_metrics(a, b, dtype, B, H, W, C, strides if sa else None, strides if sb else None, rng, out, work, work_bytes, None)


def test_c_abi_refuses_before_any_hip_call():
    lib = pkg("_lib")
    L = lib.lib()
    T = R.TILE
    assert L.sahs_image_metrics_workspace_bytes(1, 7, 7, 1) == 3 * 8
    assert L.sahs_image_metrics_workspace_bytes(3, T + 7, 2 * T + 7, 3) == 3 * 2 * 3 * 5 * 8
    for bad in ((1, 6, 16, 3), (1, 16, 6, 3), (1, 16, 16, 0), (1, 16, 16, 5), (-1, 16, 16, 3)):
        assert L.sahs_image_metrics_workspace_bytes(*bad) == 0, bad
    cases = {"for a ": dict(a=None), "for b ": dict(b=None), "for stride_a": dict(sa=False), "for stride_b": dict(sb=False),
             "for out": dict(out=None), "for workspace": dict(work=None), "7 <= H": dict(H=6), "7 <= H, W": dict(W=6), "C = 5": dict(C=5), "C = 0": dict(C=0),
             "dtype = 2": dict(dtype=2), "ssim_data_range = 0": dict(rng=0.0), "ssim_data_range = -1": dict(rng=-1.0),
             "ssim_data_range = nan": dict(rng=float("nan")), "needs 40": dict(work_bytes=39), "B = -1": dict(B=-1),
             "4-byte": dict(dtype=1, a=FAKE + 2), "8-byte aligned": dict(out=FAKE + 4)}
    for text, kw in cases.items():
        code = _call(L, **kw)
        msg = L.sahs_last_error().decode()
        assert code == 1 and msg.startswith("sahs_image_metrics:") and text in msg, (kw, code, msg)
    assert _call(L, B=0, a=None, b=None, out=None, work=None) == 0      # nothing to score: success without a launch


def test_scalar_metric_is_the_references():
    m = pkg("metrics").ScalarMetric()
    assert m.peek() == 0.0 and repr(m) == "0.0"
    for x in (1.0, 2.0, 6.0):
        m.update(x)
    assert m.peek() == 3.0 and m.num_observations == 3 and m.aggregated_value == 9.0 and repr(m) == "3.0"
    m.reset()
    assert m.peek() == 0.0 and m.num_observations == 0.0 and m.value == []


def test_two_folders_pairs_by_number():
    M, lib = pkg("metrics"), pkg("_lib")
    gt = ["f_0010.png", "f_0002.png", "f_0001.png", "notes.txt", "f_0003.jpg", "f_0100.png"]
    gen = ["2_fake.png", "10_fake.png", "1_fake.png", "metrics.txt"]
    assert M.pair_png_names(gt, gen) == [("f_0001.png", "1_fake.png"), ("f_0002.png", "2_fake.png"), ("f_0010.png", "10_fake.png")]
    assert M.pair_png_names(gt, []) == []
    with pytest.raises(lib.SahsError, match="5 generated images but only 4"):
        M.pair_png_names(gt, gen + ["11.png", "12.png"])
    with pytest.raises(lib.SahsError, match="no digits"):
        M.pair_png_names(gt, ["fake.png"])
