"""The fused image metrics on the GPU (include/sahs_nerf.h: sahs_image_metrics; ops.image_metrics; metrics.py) against the float64
references of tests/metrics_reference.py, at the smallest shapes that can break the kernel: with T the tile edge, (H - 6, W - 6) =
(1,1), (1,2), (2,1), (T,T), (T+1,T), (T,T+1), (T-1,2T+1) and 45 x 71; C = 1 and 3; batches of 3 and 1 with different content per image;
channels-last, channels-first and a cropped view.  tests/test_metrics_host.py shows on the CPU that one wrong pixel -- first corner, last
corner, tile seam -- moves every figure by more than 100 times the tolerances used here.

Tolerances.  uint8: the integer sums are exact and the finalize kernel is float64, so MSE and L1 are within 1e-12 relative; SSIM (mean
and per channel) within 2^-19 absolute (moments exact, |S| <= 1, at most ~16 roundings of 2^-24 per window, doubled).  fp32, against
float64 on the same fp32 values, with E_torch the error of torch's fp32 formulation (five avg_pool2d planes, raw-moment variances) on
the same GPU: E_fused <= max(4 E_torch, 2^-20), absolute for SSIM and relative for MSE and L1 -- and on the flat bright pair
E_fused < E_torch, because the centred moments must beat the raw ones where they cancel.  Every E is printed (pytest -s).
"""
import functools

import numpy as np
import pytest
import torch

import metrics_reference as R
from conftest import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SSIM_TOL_U8, REL_TOL_U8, FLOOR_F32 = 2.0 ** -19, 1e-12, 2.0 ** -20


@functools.lru_cache(maxsize=None)
def cases(H, W, C, dtype):
    """-> (names, a (N, H, W, C), b, {ssim_data_range: reference rows (N, 3 + C)}), computed once per shape."""
    items = R.content(H, W, C, dtype)
    refs = {rng: np.stack([R.reference_row(a, b, rng) for _, a, b in items]) for rng in (1.0, 2.0)}
    return [n for n, _, _ in items], np.stack([a for _, a, _ in items]), np.stack([b for _, _, b in items]), refs


def rel(got, ref):
    """|got - ref| / ref, and where ref == 0: 0 if got == 0 else inf."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ref == 0, np.where(got == 0, 0.0, np.inf), np.abs(got - ref) / np.abs(ref))


def errors(rows, ref):
    """-> (SSIM error: the worst of the mean and the channels, absolute), relative MSE error, relative L1 error; each (N,)."""
    return np.abs(rows[:, [0] + list(range(3, rows.shape[1]))] - ref[:, [0] + list(range(3, rows.shape[1]))]).max(1), rel(rows[:, 1], ref[:, 1]), rel(rows[:, 2], ref[:, 2])


def run(a, b, rng, channels_last=True, batch=3):
    """ops.image_metrics over the N pairs in batches of ``batch`` (the last one smaller: N = 10 gives 3, 3, 3, 1) -> (N, 3 + C) numpy."""
    ops = pkg("ops")
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    if not channels_last:
        ta, tb = ta.permute(0, 3, 1, 2).contiguous(), tb.permute(0, 3, 1, 2).contiguous()
    out = [ops.image_metrics(ta[i:i + batch], tb[i:i + batch], ssim_data_range=rng, channels_last=channels_last) for i in range(0, len(a), batch)]
    out = torch.cat(out)
    assert out.dtype == torch.float64 and out.is_cuda and out.shape == (len(a), 3 + a.shape[3])
    return out.cpu().numpy()


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d" % s)
def test_uint8_against_float64(shape):
    worst = np.zeros(3)
    for C in (1, 3):
        names, a, b, refs = cases(*shape, C, np.uint8)
        for rng in (1.0, 2.0):
            for channels_last in (True, False):
                rows = run(a, b, rng, channels_last)
                e = np.stack(errors(rows, refs[rng]))
                print("uint8 %s C=%d R=%g %s: SSIM %.2e  MSE rel %.2e  L1 rel %.2e" % (shape, C, rng, "HWC" if channels_last else "CHW", *e.max(1)))
                worst = np.maximum(worst, e.max(1))
                for k, name in enumerate(names):
                    assert e[0, k] <= SSIM_TOL_U8 and e[1, k] <= REL_TOL_U8 and e[2, k] <= REL_TOL_U8, (shape, C, rng, channels_last, name, e[:, k])
                k = names.index("identical")
                assert rows[k, 0] == 1.0 and rows[k, 1] == 0.0 and rows[k, 2] == 0.0
    print("uint8 %s worst: SSIM %.2e  MSE rel %.2e  L1 rel %.2e" % (shape, *worst))


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d" % s)
def test_fp32_error_rule(shape):
    for C in (1, 3):
        names, a, b, refs = cases(*shape, C, np.float32)
        ta, tb = (torch.from_numpy(x).to(DEV).permute(0, 3, 1, 2).contiguous() for x in (a, b))
        for rng in (1.0, 2.0):
            e_torch = np.stack(errors(R.torch_formulation(ta, tb, rng).double().cpu().numpy(), refs[rng]))
            for channels_last in (True, False):
                e = np.stack(errors(run(a, b, rng, channels_last), refs[rng]))
                for k, name in enumerate(names):
                    print("fp32 %s C=%d R=%g %s %-12s E_fused SSIM %.2e MSE %.2e L1 %.2e | E_torch SSIM %.2e MSE %.2e L1 %.2e"
                          % (shape, C, rng, "HWC" if channels_last else "CHW", name, *e[:, k], *e_torch[:, k]))
                for k, name in enumerate(names):
                    assert np.all(e[:, k] <= np.maximum(4.0 * e_torch[:, k], FLOOR_F32)), (shape, C, rng, channels_last, name, e[:, k], e_torch[:, k])
                    if name == "flat_bright":
                        assert e[0, k] < e_torch[0, k], (shape, C, rng, "centred moments no better than raw ones", e[0, k], e_torch[0, k])


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["uint8", "fp32"])
def test_same_bits_every_call_and_batch_equals_singles(dtype):
    ops = pkg("ops")
    _, a, b, _ = cases(R.TILE + 5, 2 * R.TILE + 7, 3, dtype)
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    first, again = ops.image_metrics(ta, tb), ops.image_metrics(ta, tb)
    assert torch.equal(first.view(torch.int64), again.view(torch.int64))
    for batch in (1, 3):
        parts = torch.cat([ops.image_metrics(ta[i:i + batch], tb[i:i + batch]) for i in range(0, len(a), batch)])
        assert torch.equal(first.view(torch.int64), parts.view(torch.int64)), batch
    single = ops.image_metrics(ta[2], tb[2])      # no batch dimension: one row
    assert single.shape == (6,) and torch.equal(single.view(torch.int64), first[2].view(torch.int64))


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["uint8", "fp32"])
def test_cropped_view_is_read_through_its_strides(dtype):
    """A crop of a larger batch: row stride > W * C, batch stride > H * W * C, and the two operands with different strides."""
    ops = pkg("ops")
    H, W = 45, 71
    _, a, b, _ = cases(H, W, 3, dtype)
    big = torch.full((len(a), H + 5, W + 9, 3), 77, dtype=torch.from_numpy(a).dtype, device=DEV)      # (anything read outside the crop shows in every figure)
    big[:, 2:2 + H, 3:3 + W] = torch.from_numpy(a).to(DEV)
    va, tb = big[:, 2:2 + H, 3:3 + W], torch.from_numpy(b).to(DEV)
    assert not va.is_contiguous() and va.stride(1) > W * 3
    rows, plain = ops.image_metrics(va, tb), ops.image_metrics(torch.from_numpy(a).to(DEV), tb)      # (the latter is held to float64 above)
    assert torch.equal(rows.view(torch.int64), plain.view(torch.int64))
    swapped = ops.image_metrics(tb, va)      # SSIM, MSE and L1 are symmetric, and so is every sum the kernel forms
    assert torch.equal(rows.view(torch.int64), swapped.view(torch.int64))


def test_refusals_by_name():
    ops, lib = pkg("ops"), pkg("_lib")
    u = torch.zeros(9, 9, 3, dtype=torch.uint8, device=DEV)
    f = torch.zeros(9, 9, 3, dtype=torch.float32, device=DEV)
    with pytest.raises(lib.SahsError, match="both be torch.uint8 or both torch.float32, got torch.uint8 and torch.float32"):
        ops.image_metrics(u, f)
    with pytest.raises(lib.SahsError, match="got torch.float64 and torch.float64"):
        ops.image_metrics(f.double(), f.double())
    with pytest.raises(lib.SahsError, match="got torch.bfloat16"):
        ops.image_metrics(f.bfloat16(), f.bfloat16())
    with pytest.raises(lib.SahsError, match=r"one shape.*got \(9, 9, 3\) and \(9, 8, 3\)"):
        ops.image_metrics(f, f[:, :8])
    with pytest.raises(lib.SahsError, match="b must be a GPU tensor"):
        ops.image_metrics(f, f.cpu())
    with pytest.raises(lib.SahsError, match="a must be a GPU tensor"):
        ops.image_metrics(np.zeros((9, 9, 3), np.float32), f)
    with pytest.raises(lib.SahsError, match="7 <= H, W"):
        ops.image_metrics(f[:6], f[:6])
    with pytest.raises(lib.SahsError, match="C = 5 channels"):
        ops.image_metrics(torch.zeros(9, 9, 5, device=DEV), torch.zeros(9, 9, 5, device=DEV))
    with pytest.raises(lib.SahsError, match="must be > 0"):
        ops.image_metrics(f, f, data_range=0.0)
    with pytest.raises(lib.SahsError, match="must be > 0"):
        ops.image_metrics(f, f, ssim_data_range=-2.0)
    torch.cuda.synchronize()


def test_metrics_module():
    M = pkg("metrics")
    names, a, b, refs = cases(45, 71, 3, np.uint8)
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    m = M.image_metrics(ta, tb, data_range=1.0, ssim_data_range=2.0)
    k = names.index("identical")
    assert m["mse"][k] == 0.0 and torch.isinf(m["psnr"][k]) and m["psnr"][k] > 0 and m["ssim"][k] == 1.0
    fin = [i for i in range(len(names)) if i != k]
    want = R.psnr(refs[2.0][fin, 1])
    assert np.abs(m["psnr"].cpu().numpy()[fin] - want).max() <= 10.0 / np.log(10.0) * 2 * REL_TOL_U8      # d psnr = 10 / ln 10 * d mse / mse
    assert np.abs(m["ssim"].cpu().numpy() - refs[2.0][:, 0]).max() <= SSIM_TOL_U8 and m["ssim_channels"].shape == (len(a), 3)
    assert torch.equal(M.ssim(ta, tb, 2.0), m["ssim"]) and torch.equal(M.l1(ta, tb), m["l1"])
    assert np.abs(M.ssim(ta, tb).cpu().numpy() - refs[1.0][:, 0]).max() <= SSIM_TOL_U8      # ssim_data_range defaults to data_range
    p2 = M.psnr(ta, tb, data_range=2.0).cpu().numpy()[fin]
    assert np.abs(p2 - R.psnr(refs[1.0][fin, 1], 2.0)).max() <= 10.0 / np.log(10.0) * 2 * REL_TOL_U8
    assert M.psnr(ta[0], tb[0]).shape == ()


def test_score_frames_scores_what_the_png_holds():
    """A render_frames-shaped result (rgb with 15 columns, values outside [0, 1]) is scored as evaluation.cast_to_image quantises it."""
    M, ops, ev = pkg("metrics"), pkg("ops"), pkg("evaluation")
    rng = np.random.default_rng(3)
    H, W = 40, 45
    results = [dict(rgb=torch.from_numpy(rng.uniform(-0.2, 1.2, (H, W, 15)).astype(np.float32)).to(DEV), disp=None) for _ in range(5)]
    targets = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(5)]
    s = M.score_frames(results, targets, batch=2)
    pngs = np.stack([ev.cast_to_image(r["rgb"][..., :3]) for r in results])
    want = ops.image_metrics(torch.from_numpy(pngs).to(DEV), torch.from_numpy(np.stack(targets)).to(DEV))
    for key, col in (("ssim", 0), ("mse", 1), ("l1", 2)):
        assert torch.equal(s[key].view(torch.int64), want[:, col].contiguous().view(torch.int64)), key
    ref = np.stack([R.reference_row(p, t) for p, t in zip(pngs, targets)])
    assert np.abs(s["ssim"].cpu().numpy() - ref[:, 0]).max() <= SSIM_TOL_U8 and rel(s["l1"].cpu().numpy(), ref[:, 2]).max() <= REL_TOL_U8
    assert abs(s["mean_ssim"] - ref[:, 0].mean()) <= SSIM_TOL_U8 and abs(s["mean_psnr"] - R.psnr(ref[:, 1]).mean()) <= 1e-11
    # generator outputs: float (B, 3, H, W) against float targets
    g = torch.from_numpy(rng.uniform(0, 1, (2, 3, H, W)).astype(np.float32)).to(DEV)
    t = torch.from_numpy(rng.uniform(0, 1, (2, 3, H, W)).astype(np.float32)).to(DEV)
    s = M.score_frames(g, t, channels_last=False)
    assert torch.equal(s["ssim"], ops.image_metrics(g, t, channels_last=False)[:, 0])


def test_two_folders_writes_the_references_layout(tmp_path):
    from PIL import Image
    M = pkg("metrics")
    gt, gen = tmp_path / "gt", tmp_path / "gen"
    gt.mkdir()
    gen.mkdir()
    H, W, pairs = 20, 24, {}
    for i, n in enumerate((3, 1, 10, 2, 7, 5)):      # written out of order: the pairing sorts by number
        a, b = R.ramp_noise_pair(H, W, 3, 0.01 * (i + 1), 40 + i, np.uint8)
        Image.fromarray(a).save(gt / ("f_%04d.png" % n))
        Image.fromarray(b).save(gen / ("%d_fake.png" % n))
        pairs[n] = R.reference_row(a, b)
    Image.fromarray(a).save(gt / "f_0099.png")      # ground truth may have more frames than were generated
    res = M.two_folders(str(gt), str(gen), batch=4, log=lambda *_: None)
    order = sorted(pairs)
    ref = np.stack([pairs[n] for n in order])
    assert res["names"] == ["%d_fake.png" % n for n in order]
    assert np.abs(np.array(res["ssim"]) - ref[:, 0]).max() <= SSIM_TOL_U8 and rel(np.array(res["l1"]), ref[:, 2]).max() <= REL_TOL_U8
    want = dict(L1=ref[:, 2].mean(), PSNR=R.psnr(ref[:, 1]).mean(), SSIM=ref[:, 0].mean())
    assert abs(res["mean_ssim"] - want["SSIM"]) <= SSIM_TOL_U8 and abs(res["mean_l1"] - want["L1"]) <= REL_TOL_U8 and abs(res["mean_psnr"] - want["PSNR"]) <= 1e-11
    lines = (gen / "metrics.txt").read_text().splitlines()
    per_frame = [l for l in lines if "_fake.png" in l]
    assert [l.split()[0] for l in per_frame] == [n for n in res["names"] for _ in range(3)] and not any("LPIPS" in l for l in lines)
    assert [l.split()[1] for l in per_frame[:3]] == ["L1:", "PSNR:", "SSIM:"] and "=" * 80 in lines and " Summary " in lines
    # the file prints six decimals (%5f, the reference's format): its means are the references' to half a unit of the last one printed
    for key, value in want.items():
        line = [l for l in lines if l.startswith(" mean %s:" % key)]
        assert len(line) == 1 and abs(float(line[0].split()[-1]) - value) <= 0.5e-6 + SSIM_TOL_U8, (key, line, value)
