"""LPIPS on the GPU (include/sahs_nerf.h: sahs_lpips_prepare, sahs_lpips_distance; ops.lpips_prepare, ops.lpips_distance; metrics.LPIPS)
against the float64 reference of tests/lpips_reference.py, which tests/test_lpips_reference_host.py holds to the definition.

Head, on synthetic fp32 feature tensors against float64 on the same values, at layer pixel counts 1, 3, 49, T - 16, T, T + 16 (T = 256:
15x16, 16x16, 16x17) and 961 (four tiles, the last partial), C = 64 and 384, B = 1 and 3, and a job list of all five layers with mixed
sizes.  Rule: |fused - ref| <= 1e-12 * sum_l max_c w_lc, per image and per layer -- every per-pixel term is at most max_c w_lc because
sum_c a^_c^2 <= 1, a float64 chain over at most 384 + 5 terms carries about 4e-14 of that, and the rule is that figure times ten and more.
Identical features give exactly 0.0, all-zero pixels finite results, a batch the bits of its single calls, two calls the same bits.

Prepare: the formula in fp32 evaluated by torch on the same GPU, one torch operation per step (tests/lpips_reference.py:
torch_scaling), within 2 fp32 ulps of each value.  (Each step of the kernel is the same correctly rounded fp32 operation in the same
order -- a true division by 255, 2x - 1 with 2x exact, a subtraction, a true division -- so equal bits are expected; the count of
unequal values is printed.)

Whole metric, LPIPS.from_seed weights, shapes 31x31, 45x71 and 127x130, uint8 and fp32, both ``normalize`` values, the five pairs of
lpips_reference.content as one batch.  With E_torch the error of the same convolutions -- the same feature tensors, from scaled inputs
that are equal bits either way -- under a torch-written head in fp32 on the same GPU: E_fused <= max(4 E_torch, 2^-20), relative to the
float64 value (absolute where that is 0).  Every E is printed (pytest -s).  (For the pair that differs in one value by 1/255 the
float64 LPIPS is ~1e-10, a difference of features that agree to 1e-3 and less, which fp32 convolutions resolve to 1e-5 .. 1e-3 only:
both E are then the convolutions' error.  So that the rule says something about the head there too, the fused head is also held, on
the GPU's own fp32 feature tensors, to float64 on the same values by the head's rule above.)  The public call gives the bits of its
steps every time, and exactly 0 for an identical pair: metrics.LPIPS runs the convolutions in the vendor library's deterministic mode.
"""
import functools

import numpy as np
import pytest
import torch

import lpips_reference as R
from conftest import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HEAD_TOL, FLOOR = 1e-12, 2.0 ** -20
# What two fp32 evaluations of the same convolutions may differ by, relative to an LPIPS value in which nothing cancels (unrelated or
# visibly different images): a feature value is an fp32 chain of up to 3 * 3 * 384 = 3456 products, whose worst-case relative error is
# 3456 * 2^-24 = 2.1e-4; half of that.  The vendor library may pick another kernel for another batch size, so a batch and its single
# pairs are compared through this, each against float64; the same call twice gives the same bits (metrics.LPIPS.features).
CONV_TOL = 1e-4
T = R.TILE
PIXELS = [(1, 1), (1, 3), (7, 7), (15, 16), (16, 16), (16, 17), (31, 31)]      # 1, 3, 49, T - 16, T, T + 16, 961
assert [h * w for h, w in PIXELS] == [1, 3, 49, T - 16, T, T + 16, 961]


@functools.lru_cache(maxsize=None)
def head_case(B, C, h, w, seed):
    """-> (features (2B, C, h, w) float32, weights (C,) float32, float64 d per image (B,)), computed once."""
    f, lw = R.synthetic_features(B, C, h, w, seed)
    return f, lw, R.head_rows([f], [lw])[:, 1]


def fused_head(features, lin_weights):
    ops = pkg("ops")
    out = ops.lpips_distance([torch.from_numpy(f).to(DEV) for f in features], [torch.from_numpy(w).to(DEV) for w in lin_weights])
    assert out.dtype == torch.float64 and out.is_cuda and out.shape == (features[0].shape[0] // 2, 6)
    return out


def bits(t):
    return t.contiguous().view(torch.int64)


@pytest.mark.parametrize("C", [64, 384])
@pytest.mark.parametrize("hw", PIXELS, ids=lambda s: "%dx%d" % s)
def test_head_against_float64(hw, C):
    for B in (1, 3):
        f, lw, ref = head_case(B, C, *hw, 10 + B)
        got = fused_head([f], [lw]).cpu().numpy()
        tol = HEAD_TOL * float(lw.max())
        err = np.abs(got[:, 1] - ref).max()
        print("head %s C=%d B=%d: worst |fused - float64| %.2e (tolerance %.2e, d ~ %.3f)" % (hw, C, B, err, tol, ref.mean()))
        assert np.all(np.isfinite(got)) and err <= tol, (hw, C, B, got[:, 1], ref)
        assert np.array_equal(got[:, 0], got[:, 1]) and not got[:, 2:].any()      # one layer: LPIPS = d_0, the others 0


def test_head_all_five_layers_mixed_sizes():
    shapes = [(64, 7, 9), (192, 16, 17), (384, 1, 1), (256, 31, 31), (256, 1, 3)]
    for B in (1, 3):
        cases = [head_case(B, C, h, w, 20 + l) for l, (C, h, w) in enumerate(shapes)]
        feats, lws = [c[0] for c in cases], [c[1] for c in cases]
        ref = R.head_rows(feats, lws)
        got = fused_head(feats, lws).cpu().numpy()
        tol = HEAD_TOL * sum(float(w.max()) for w in lws)
        print("head, five layers, B=%d: worst |fused - float64| %.2e (tolerance %.2e)" % (B, np.abs(got - ref).max(), tol))
        assert np.abs(got - ref).max() <= tol, (B, got, ref)
        assert np.array_equal(got[:, 0], ((((got[:, 1] + got[:, 2]) + got[:, 3]) + got[:, 4]) + got[:, 5]))
        # fewer layers: the rest of the row is 0, the layers given keep their bits
        part = fused_head(feats[1:4], lws[1:4]).cpu().numpy()
        assert np.array_equal(part[:, 1:4], got[:, 2:5]) and not part[:, 4:].any()


def test_head_identical_features_and_zero_pixels():
    f, lw, _ = head_case(3, 384, 16, 17, 13)
    same = np.concatenate([f[:3], f[:3]])
    assert not fused_head([same], [lw]).cpu().numpy().any()      # exactly 0.0, every image
    dead = f.copy()
    dead[:, :, :8] = 0.0      # half the pixels zero in every channel, in both operands
    dead[0] = 0.0      # and one image all zero against one that is not
    got = fused_head([dead], [lw]).cpu().numpy()
    ref = R.head_rows([dead], [lw])
    assert np.all(np.isfinite(got)) and np.abs(got - ref).max() <= HEAD_TOL * float(lw.max()) and got[0, 0] > 0.0
    zeros = np.zeros_like(f)
    assert not fused_head([zeros], [lw]).cpu().numpy().any()


def test_head_same_bits_every_call_and_batch_equals_singles():
    shapes = [(64, 16, 17), (384, 31, 31), (256, 1, 1)]
    cases = [head_case(3, C, h, w, 30 + l) for l, (C, h, w) in enumerate(shapes)]
    feats, lws = [torch.from_numpy(c[0]).to(DEV) for c in cases], [torch.from_numpy(c[1]).to(DEV) for c in cases]
    ops = pkg("ops")
    first, again = ops.lpips_distance(feats, lws), ops.lpips_distance(feats, lws)
    assert torch.equal(bits(first), bits(again))
    singles = torch.cat([ops.lpips_distance([torch.cat([f[i:i + 1], f[3 + i:4 + i]]) for f in feats], lws) for i in range(3)])
    assert torch.equal(bits(first), bits(singles))


def ulps(got, want):
    """|got - want| in units of the fp32 spacing at want."""
    spacing = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / spacing


@pytest.mark.parametrize("dtype", [np.uint8, np.float32], ids=["uint8", "fp32"])
@pytest.mark.parametrize("shape", [(31, 31), (45, 71)], ids=lambda s: "%dx%d" % s)
def test_prepare_is_the_formula(shape, dtype):
    ops = pkg("ops")
    H, W = shape
    items = R.content(H, W, dtype)
    a, b = (torch.from_numpy(np.stack(x)).to(DEV) for x in zip(*[(p, q) for _, p, q in items]))
    B = len(items)
    big = torch.full((B, H + 5, W + 9, 3), 77, dtype=a.dtype, device=DEV)      # (anything read outside the crop shows in the output)
    big[:, 2:2 + H, 3:3 + W] = a
    crop = big[:, 2:2 + H, 3:3 + W]
    assert not crop.is_contiguous()
    for normalize in (False, True):
        want = R.torch_scaling(a, b, normalize)
        assert want.shape == (2 * B, 3, H, W) and want.dtype == torch.float32
        layouts = {"HWC": ops.lpips_prepare(a, b, normalize), "crop": ops.lpips_prepare(crop, b, normalize),
                   "CHW": ops.lpips_prepare(a.permute(0, 3, 1, 2).contiguous(), b.permute(0, 3, 1, 2).contiguous(), normalize, channels_last=False)}
        for name, got in layouts.items():
            assert got.shape == want.shape and got.dtype == torch.float32 and got.is_contiguous()
            u = ulps(got.cpu().numpy(), want.cpu().numpy())
            print("prepare %s %s normalize=%s %s: worst %.2f ulps, %d of %d values not bit-equal"
                  % (shape, np.dtype(dtype).name, normalize, name, u.max(), int((u > 0).sum()), u.size))
            assert u.max() <= 2.0, (shape, dtype, normalize, name, u.max())
        # rows [B, 2B) come from b: swapping the operands swaps the halves, and a single pair is its rows of the batch
        swapped = ops.lpips_prepare(b, a, normalize)
        assert torch.equal(swapped[:B], layouts["HWC"][B:]) and torch.equal(swapped[B:], layouts["HWC"][:B])
        assert not torch.equal(layouts["HWC"][:B], layouts["HWC"][B:])
        one = ops.lpips_prepare(a[1], b[1], normalize)
        assert one.shape == (2, 3, H, W) and torch.equal(one[0], layouts["HWC"][1]) and torch.equal(one[1], layouts["HWC"][B + 1])


@functools.lru_cache(maxsize=None)
def whole_case(H, W, dtype, normalize):
    """-> (names, a (N, H, W, 3), b, float64 rows (N, 6)) of the five pairs, the reference computed once."""
    model = pkg("metrics").LPIPS.from_seed(0)
    items = R.content(H, W, dtype)
    a, b = np.stack([x for _, x, _ in items]), np.stack([y for _, _, y in items])
    return [n for n, _, _ in items], a, b, R.reference_rows(a, b, model, normalize)


def rel(got, ref):
    """|got - ref| / |ref|, absolute where ref == 0."""
    return np.where(ref == 0, np.abs(got - ref), np.abs(got - ref) / np.where(ref == 0, 1.0, np.abs(ref)))


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d" % s)
def test_whole_metric_error_rule(shape):
    M, ops = pkg("metrics"), pkg("ops")
    worst = 0.0
    for dtype in (np.uint8, np.float32):
        for normalize in (False, True):
            names, a, b, ref = whole_case(*shape, dtype, normalize)
            model = M.LPIPS.from_seed(0, normalize=normalize)
            ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
            lins = model.device_weights(torch.device(DEV))[1]
            # the same convolutions for both: one set of feature tensors, from scaled inputs that are the same bits either way
            x = ops.lpips_prepare(ta, tb, normalize)
            assert torch.equal(x, R.torch_scaling(ta, tb, normalize))
            feats = model.features(x)
            rows, rows_torch = ops.lpips_distance(feats, lins).cpu().numpy(), R.torch_head(feats, lins).double().cpu().numpy()
            e, e_torch = rel(rows[:, 0], ref[:, 0]), rel(rows_torch[:, 0], ref[:, 0])
            for k, name in enumerate(names):
                print("whole %s %s normalize=%s %-9s LPIPS %.6e  E_fused %.2e  E_torch %.2e" % (shape, np.dtype(dtype).name, normalize, name, ref[k, 0], e[k], e_torch[k]))
                worst = max(worst, e[k])
                assert e[k] <= max(4.0 * e_torch[k], FLOOR), (shape, dtype, normalize, name, e[k], e_torch[k])
            # the head on these very features against float64 on the same fp32 values: the head's own rule, on real feature maps
            exact = R.head_rows([f.cpu().numpy() for f in feats], [w.cpu().numpy().reshape(-1) for w in lins])
            tol = HEAD_TOL * sum(float(w.max()) for w in lins)
            print("whole %s %s normalize=%s: head on the GPU's own features, worst |fused - float64| %.2e (tolerance %.2e)"
                  % (shape, np.dtype(dtype).name, normalize, np.abs(rows - exact).max(), tol))
            assert np.abs(rows - exact).max() <= tol and rows[names.index("pixel"), 0] > 0.0
            # the public call is these steps: the same bits (the convolutions run in deterministic mode), every time; an image is at
            # distance exactly 0 from itself
            public = model.layers(ta, tb)
            assert public.shape == (len(a), 6) and public.dtype == torch.float64 and public.is_cuda
            assert np.array_equal(public.cpu().numpy(), rows) and torch.equal(bits(model(ta, tb)), bits(public[:, 0]))
            assert not public[names.index("identical")].any()
            if dtype == np.uint8 and not normalize:      # one pair, no batch dimension: a scalar, and a (6,) row
                one = model(ta[0], tb[0])
                assert one.shape == () and model.layers(ta[0], tb[0]).shape == (6,) and abs(float(one) - ref[0, 0]) <= CONV_TOL * ref[0, 0]
    print("whole %s: worst E_fused %.2e" % (shape, worst))


def score_frames_inputs(H, W, seed=3):
    """Four render_frames-shaped results (rgb with 15 columns, values outside [0, 1]) that stray further and further from their uint8
    targets, so that every frame has a score of its own."""
    rng = np.random.default_rng(seed)
    targets = [rng.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(4)]
    results = []
    for t, mix in zip(targets, (0.2, 0.4, 0.7, 1.0)):
        rgb = rng.uniform(-0.2, 1.2, (H, W, 15))
        rgb[..., :3] = (1.0 - mix) * t / 255.0 + mix * rgb[..., :3]
        results.append(rgb.astype(np.float32))
    return results, targets


def test_score_frames_with_lpips_equals_per_pair_calls():
    M = pkg("metrics")
    model = M.LPIPS.from_seed(1)
    H, W = 40, 36
    results, targets = score_frames_inputs(H, W)
    results = [dict(rgb=torch.from_numpy(r).to(DEV), disp=None) for r in results]
    plain = M.score_frames(results, targets, batch=2)
    s = M.score_frames(results, targets, batch=2, lpips=model)
    assert "lpips" not in plain and "mean_lpips" not in plain
    for key in plain:      # the other figures are untouched
        assert torch.equal(s[key], plain[key]) if isinstance(plain[key], torch.Tensor) else s[key] == plain[key], key
    assert s["lpips"].shape == (4,) and s["lpips"].dtype == torch.float64 and s["lpips"].is_cuda
    singles = M.score_frames(results, targets, batch=1, lpips=model)
    ref = []
    for k, (r, t) in enumerate(zip(results, targets)):
        q, tt = M.quantise(r["rgb"][..., :3]), torch.from_numpy(t).to(DEV)
        pair = float(model(q, tt))      # the call a user makes pair by pair, on the quantised frame
        ref.append(R.reference_rows(q.cpu().numpy()[None], t[None], model, False)[0, 0])
        assert float(singles["lpips"][k]) == pair, k      # batch=1 makes that very call
        for got in (pair, float(s["lpips"][k])):
            assert abs(got - ref[-1]) <= CONV_TOL * ref[-1], (k, got, ref[-1])
        assert abs(float(s["lpips"][k]) - pair) <= 2 * CONV_TOL * ref[-1]
    assert abs(s["mean_lpips"] - np.mean(ref)) <= CONV_TOL * np.max(ref) and s["mean_lpips"] == float(s["lpips"].mean())
    # a wrong pairing would show: the frames' scores differ from each other by far more than the tolerance
    assert np.abs(np.diff(np.sort(ref))).min() > 10 * CONV_TOL * np.max(ref)


def test_two_folders_writes_the_complete_layout(tmp_path):
    from PIL import Image
    M = pkg("metrics")
    model = M.LPIPS.from_seed(2)
    gt, gen = tmp_path / "gt", tmp_path / "gen"
    gt.mkdir()
    gen.mkdir()
    H, W, pairs = 40, 36, []
    for n, (a, b) in ((2, R.noisy_pair(H, W, np.uint8, 8)), (1, R.textured_pair(H, W, np.uint8, 9))):      # written out of order
        Image.fromarray(a).save(gt / ("f_%04d.png" % n))
        Image.fromarray(b).save(gen / ("%d_fake.png" % n))
        pairs.append((n, a, b))
    pairs.sort(key=lambda p: p[0])
    plain = M.two_folders(str(gt), str(gen), log=lambda *_: None)
    text_plain = (gen / "metrics.txt").read_bytes()
    res = M.two_folders(str(gt), str(gen), log=lambda *_: None, lpips=model)
    text = (gen / "metrics.txt").read_text()
    # the values are those of the direct call on the batch two_folders forms (generated first, as score_frames is called)
    fake, real = (torch.from_numpy(np.stack(x)).to(DEV) for x in ([p[2] for p in pairs], [p[1] for p in pairs]))
    direct = model(fake, real).cpu().numpy()
    assert res["names"] == ["1_fake.png", "2_fake.png"] and res["lpips"] == [float(direct[0]), float(direct[1])]
    assert res["mean_lpips"] == (res["lpips"][0] + res["lpips"][1]) / 2 and 0.0 < direct[1] < (1 - 10 * CONV_TOL) * direct[0]
    for key in ("l1", "psnr", "ssim", "mean_l1", "mean_psnr", "mean_ssim"):
        assert res[key] == plain[key], key
    # the complete layout, character for character from the values returned
    want = "".join(name + "   L1:  \t%5f \n" % l1 + name + "   PSNR:\t%5f \n" % p + name + "   SSIM:\t%5f \n" % s + name + "   LPIPS:\t%5f\n\n" % lp
                   for name, l1, p, s, lp in zip(res["names"], res["l1"], res["psnr"], res["ssim"], res["lpips"]))
    want += "=" * 80 + "\n Summary \n folder 1: %s \n folder 2: %s \n" % (gt, gen) + "-" * 80
    want += "\n mean L1:\t%5f" % res["mean_l1"] + "\n mean PSNR:\t%5f" % res["mean_psnr"] + "\n mean SSIM:\t%5f" % res["mean_ssim"]
    want += "\n mean LPIPS\t%5f\n" % res["mean_lpips"]
    assert text == want
    # without lpips: byte for byte what the function wrote before it knew of LPIPS
    old = "".join(name + "   L1:  \t%5f \n" % l1 + name + "   PSNR:\t%5f \n" % p + name + "   SSIM:\t%5f \n\n" % s
                  for name, l1, p, s in zip(plain["names"], plain["l1"], plain["psnr"], plain["ssim"]))
    old += "=" * 80 + "\n Summary \n folder 1: %s \n folder 2: %s \n" % (gt, gen) + "-" * 80
    old += "\n mean L1:\t%5f" % plain["mean_l1"] + "\n mean PSNR:\t%5f" % plain["mean_psnr"] + "\n mean SSIM:\t%5f\n" % plain["mean_ssim"]
    assert text_plain == old.encode() and sorted(plain) == ["l1", "mean_l1", "mean_psnr", "mean_ssim", "names", "psnr", "ssim"]


def test_refusals_by_name():
    M, ops, lib = pkg("metrics"), pkg("ops"), pkg("_lib")
    f = torch.zeros(64, 64, 3, device=DEV)
    with pytest.raises(lib.SahsError, match="C = 4 channels"):
        ops.lpips_prepare(torch.zeros(64, 64, 4, device=DEV), torch.zeros(64, 64, 4, device=DEV))
    with pytest.raises(lib.SahsError, match="30 x 64 pixels"):
        ops.lpips_prepare(f[:30], f[:30])
    with pytest.raises(lib.SahsError, match="64 x 30 pixels"):
        M.LPIPS.from_seed(0)(f[:, :30], f[:, :30])
    with pytest.raises(lib.SahsError, match="got torch.float64 and torch.float64"):
        ops.lpips_prepare(f.double(), f.double())
    with pytest.raises(lib.SahsError, match="got torch.uint8 and torch.float32"):
        ops.lpips_prepare(f.to(torch.uint8), f)
    with pytest.raises(lib.SahsError, match=r"one shape.*got \(64, 64, 3\) and \(64, 63, 3\)"):
        ops.lpips_prepare(f, f[:, :63])
    feat, w = torch.zeros(2, 64, 7, 7, device=DEV), torch.zeros(64, device=DEV)
    with pytest.raises(lib.SahsError, match="1 .. 5 layers"):
        ops.lpips_distance([feat] * 6, [w] * 6)
    with pytest.raises(lib.SahsError, match=r"features\[0\] must be contiguous float32"):
        ops.lpips_distance([feat.permute(0, 1, 3, 2)[:, :, :, :5]], [w])
    with pytest.raises(lib.SahsError, match=r"features\[0\] must be contiguous float32 .* got torch.float64"):
        ops.lpips_distance([feat.double()], [w])
    with pytest.raises(lib.SahsError, match=r"features\[0\] is \(2, 64, 7, 7\) with 63 weights"):
        ops.lpips_distance([feat], [w[:63]])
    with pytest.raises(lib.SahsError, match=r"features\[0\] is \(3, 64, 7, 7\)"):
        ops.lpips_distance([torch.zeros(3, 64, 7, 7, device=DEV)], [w])
    with pytest.raises(lib.SahsError, match="job 0 has C = 1025"):
        ops.lpips_distance([torch.zeros(2, 1025, 1, 1, device=DEV)], [torch.zeros(1025, device=DEV)])
    torch.cuda.synchronize()
