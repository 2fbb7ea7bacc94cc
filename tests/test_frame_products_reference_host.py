"""The numpy statement of the frame products (tests/frame_products_reference.py) on the CPU: it reproduces the reference's own vectors
(tests/golden/post.npz), agrees with evaluation.py's torch functions on square maps, and three single faults planted in it each
break the bound tests/test_gpu_frame_products.py holds the kernel to -- so that bound has teeth."""
import numpy as np
import pytest
import torch

import frame_products_reference as R
from conftest import load_golden, pkg

SQUARE = [(3, 3), (24, 24), (32, 32), (65, 65)]


def torch_normals(E, disp, focal, w_bg, clean, central):
    return E.normal_map(torch.from_numpy(disp), focal, torch.from_numpy(w_bg) if w_bg is not None else None, clean=clean,
                        central_difference=central).numpy()


def test_statement_reproduces_the_reference_vectors():
    g = load_golden("post")
    for key, kw in (("normals_clean", dict(w_bg=g["w_bg"], clean=True)), ("normals_raw", dict(w_bg=None, clean=False)),
                    ("normals_central", dict(w_bg=g["w_bg"], clean=True, central_difference=True))):
        n = R.normals(g["disp"], g["focal"], **kw)
        assert n.shape == g[key].shape
        assert np.abs(n - g[key]).max() <= 2e-3, (key, np.abs(n - g[key]).max())
    assert np.array_equal(R.seg(g["seg"]), R.image(g["seg_color"]))      # the colours as bytes ...
    assert np.array_equal(R.seg(g["seg"]).astype(np.float32) / np.float32(255), g["seg_color"])      # ... and as the reference's floats
    assert np.array_equal(R.disparity(g["disp"]), g["disp_img"])


@pytest.mark.parametrize("H,W", SQUARE)
def test_statement_agrees_with_the_torch_functions(H, W):
    E = pkg("evaluation")
    rgb, disp, w_bg, focal = R.make_rgb(H, W, 3), R.make_disp(H, W, 3), R.make_w_bg(H, W, 3), R.focal_for(H, W)
    t = torch.from_numpy(rgb)
    assert np.array_equal(R.image(rgb), E.cast_to_image(t[..., :3]))
    assert np.array_equal(R.seg(rgb[..., 3:]), E.cast_to_image(E.label2color(t[..., 3:])))
    assert np.array_equal(R.disparity(disp), E.cast_to_disparity_image(torch.from_numpy(disp)))
    for clean in (True, False):
        for central in (False, True):
            want = R.normals(disp, focal, w_bg, clean, central)
            got = torch_normals(E, disp, focal, w_bg, clean, central)
            assert got.shape == want.shape
            e = np.abs(got - want).max()
            assert e <= 2e-3, (clean, central, e)      # the bound the reference's vectors are held to
            if clean:
                white = R.white_mask(w_bg, central)
                assert (white.any() or H < 24) and np.all(want[white] == 255.0) and np.all(got[white] == 255.0)


def test_statement_nan_rule():
    rgb = R.make_rgb(5, 4, 1, nan=True)
    assert np.array_equal(R.seg(rgb[..., 3:])[0, 2], R.SEG_COLOURS[2])      # the FIRST NaN wins, not the 9.0 behind it
    assert R.image(rgb)[2, 2, 1] == 0
    d = R.make_disp(5, 4, 1)
    assert R.disparity(np.full((5, 4), 0.7, np.float32)).max() == 0      # 0 / 0
    d[3, 1] = np.nan
    assert R.disparity(d).max() == 0
    n = R.normals(d, R.focal_for(5, 4))
    lo, hi = R.byte_bounds(n, 1e-3)
    assert np.isnan(n).any() and np.all(lo[np.isnan(n)] == 0) and np.all(hi[np.isnan(n)] == 0)


@pytest.mark.parametrize("H,W", [(24, 24), (33, 31)])
def test_single_faults_exceed_the_gpu_bound(H, W):
    """The GPU test allows the normals 4 e, e = the torch functions' own fp32 error against the statement, and the bytes the
    truncations of that interval; image, seg and disparity no byte at all."""
    E = pkg("evaluation")
    disp, w_bg, focal = R.make_disp(H, W, 3), R.make_w_bg(H, W, 3), R.focal_for(H, W)
    want = R.normals(disp, focal, w_bg, True, False)
    white = R.white_mask(w_bg)
    e = 2e-3      # no smaller than any e measured on these shapes (the square ones: test_statement_agrees_with_the_torch_functions)
    if H == W:
        e = np.abs(torch_normals(E, disp, focal, w_bg, True, False) - want)[~white].max()
    lo, hi = R.byte_bounds(want, 4 * e)
    swapped = R.normals(disp, focal, w_bg, True, False, fault="swap")
    assert np.abs(swapped - want)[~white].max() > 4 * e
    b = R.to_u8(np.clip(swapped, 0, 255))
    assert np.any((b < lo) | (b > hi))
    unwhitened = R.normals(disp, focal, w_bg, True, False, fault="no_white")
    assert np.any(R.to_u8(np.clip(unwhitened, 0, 255))[white] != 255)
    edges = R.make_disp_on_byte_edges(H, W, 3)
    assert np.any(R.disparity(edges, fault="reciprocal") != R.disparity(edges))
    assert np.array_equal(R.disparity(edges), E.cast_to_disparity_image(torch.from_numpy(edges)))
