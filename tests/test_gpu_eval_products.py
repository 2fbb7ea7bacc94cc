"""evaluation.render_frames(fused_products=True) on the MI355X: the same frames as the default path -- bit-identical renders, identical
RGB, mask and disparity PNGs -- with the normal PNG held to the float64 statement by the byte rule of tests/test_gpu_frame_products.py."""
import numpy as np
import pytest
import torch

import frame_products_reference as R
from conftest import pkg

pytestmark = pytest.mark.gpu


def test_render_frames_fused_products(tmp_path):
    from PIL import Image
    sahs, E, Wt = pkg(), pkg("evaluation"), pkg("weights")
    dev = torch.device("cuda:0")
    cfg = sahs.default_config("expression")      # the smallest model and frame size of tests/test_gpu_eval.py
    cfg.nerf.validation.perturb = False
    fw = Wt.flatten_state_dict(Wt.hash_state_dict(0, 8.0, 30.0, model="nerface"), model="nerface")
    model = sahs.NeRFaceModel(cfg).to(dev).load_flat(fw).eval()
    H = Wd = 16
    focal = np.array([1100.0 * Wd / 512, 1100.0 * Wd / 512, 0.5, 0.5], np.float32)
    rng = np.random.default_rng(4)
    frames = [dict(pose=np.concatenate([np.eye(3), [[0.0], [0.0], [0.5]]], 1).astype(np.float32),
                   expression=(rng.standard_normal(76) * 0.5).astype(np.float32), name="f_%04d.png" % i) for i in range(2)]
    bg = torch.rand(H, Wd, 15, generator=torch.Generator().manual_seed(2))
    outs = {}
    for fused in (False, True):
        torch.manual_seed(0)
        outs[fused] = E.render_frames(model, cfg, frames, (H, Wd, focal), background=bg, savedir=str(tmp_path / str(fused)),
                                      save_disparity=True, log=lambda s: None, fused_products=fused)
    for i, (a, b) in enumerate(zip(outs[False], outs[True])):
        name = "f_%04d.png" % i
        assert set(b) == set(a) | {"bytes"} and set(b["bytes"]) == {"image", "seg", "normals", "disparity"}
        assert all(v.dtype == torch.uint8 and v.is_cuda for v in b["bytes"].values())
        assert torch.equal(a["rgb"], b["rgb"]) and torch.equal(a["disp"], b["disp"])      # the keyword touches nothing before the tail
        assert b["normals"].shape == a["normals"].shape and b["normals"].dtype == torch.float32
        for sub in ("", "masks", "disparity"):
            pa, pb = (np.asarray(Image.open(tmp_path / str(f) / sub / name)) for f in (False, True))
            assert pa.shape[:2] == (H, Wd) and np.array_equal(pa, pb), (i, sub)
        png = np.asarray(Image.open(tmp_path / "True" / "normals" / name))
        assert np.array_equal(png, b["bytes"]["normals"].cpu().numpy())
        disp, w_bg = a["disp"].cpu(), a["w_bg"].cpu()
        r64, white = R.normals(disp.numpy(), focal, w_bg.numpy()), R.white_mask(w_bg.numpy())
        t32 = E.normal_map(disp, focal, w_bg, clean=True).numpy()      # the existing function's own fp32 rounding, on the CPU
        rest = np.broadcast_to(~white[..., None], r64.shape) & ~np.isnan(r64)
        e = float(np.abs(t32 - r64)[rest].max())
        f32 = b["normals"].cpu().numpy()
        dev_op = float(np.abs(f32 - r64)[rest].max())
        lo, hi = R.byte_bounds(r64, 4 * e)
        share = float((hi > lo)[rest].mean())
        print("frame %d: e = %.3e, op deviation = %.3e, two-byte share = %.4f, white = %.2f" % (i, e, dev_op, share, white.mean()))
        assert np.all(png[white] == 255) and np.all(png[np.isnan(r64)] == 0)
        assert dev_op <= 4 * e
        assert np.all((png >= lo) & (png <= hi)) and share <= 0.02
