"""CPU-side checks of the fused image objective: its two float64 references agree on every test input, the inputs exercise what they are
meant to, each fault a kernel could have -- a dropped gamma term, a dropped row of window origins at a tile seam, an exclusive clamp mask,
sign(0) = 1, the wrong normalisation -- moves the error measure by more than 100 times the GPU tests' tolerance, and the C entry refuses
bad arguments before any HIP call."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import image_loss_reference as R
import metrics_reference as M
from conftest import REPO, pkg

FAKE = 0x10000      # a non-null, 8-byte-aligned address that is never dereferenced: every call below is refused before any HIP call
SHAPES = M.SHAPES + [(44, 44), (70, 39)]


def test_tile_edge_is_the_headers():
    text = open(os.path.join(REPO, "include", "sahs_nerf.h")).read()
    assert int(re.search(r"#define SAHS_IMAGE_LOSS_TILE (\d+)", text).group(1)) == R.TILE == pkg("ops").IMAGE_LOSS_TILE


def test_gpu_shapes_are_the_issues():
    T = R.TILE
    assert R.gpu_shapes() == [(7, 7), (7, 8), (8, 7), (13, 13), (T, T), (T + 1, T), (T, T + 1), (T - 1, 2 * T + 1), (2 * T + 7, T + 6), (45, 71)]
    assert R.WEIGHTS == [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0.5, 0.25)]


def test_inputs_exercise_the_clamp_and_the_planted_elements():
    for C in (1, 3, 4):
        items = R.inputs(45, 71, C)
        assert [n for n, _, _ in items] == [n for n, _, _ in M.content(45, 71, C, np.float32)] + ["identical_exact", "planted_edges", "planted_equal"]
        for name, pred, target in items:
            assert pred.dtype == target.dtype == np.float32 and pred.shape == target.shape == (45, 71, C)
            outside = float(((pred < 0) | (pred > 1)).mean())
            if name == "identical_exact":
                assert outside == 0.0 and np.array_equal(pred, target)
            else:
                assert 0.01 <= outside <= 0.45, (C, name, outside)
    for H, W in R.gpu_shapes():
        by_name = {n: (p, t) for n, p, t in R.inputs(H, W, 1)}
        pred, target = by_name["planted_edges"]
        assert [float(pred.flat[k]) for k, _ in R.PLANTED_EDGES] == [0.0, 1.0, 0.0] and np.signbit(pred.flat[R.PLANTED_EDGES[2][0]])
        pred, target = by_name["planted_equal"]
        assert all(pred.flat[k] == target.flat[k] and 0.0 < target.flat[k] < 1.0 for k in R.PLANTED_EQUAL)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_two_references_agree(shape):
    worst = 0.0
    for C in (1, 3):
        for name, pred, target in R.inputs(*shape, C):
            for clamp in (True, False):
                ta, ga = R.autograd_terms(pred, target, clamp)
                tb, gb = R.closed_terms(pred, target, clamp)
                assert np.abs(ta - tb).max() <= 1e-12, (shape, C, name, clamp, ta, tb)
                for w in R.WEIGHTS:
                    (_, a), (_, b) = R.combine(ta, ga, w), R.combine(tb, gb, w)
                    e = R.grad_error(a, b, w)
                    worst = max(worst, e)
                    assert e <= 1e-11, (shape, C, name, clamp, w, e)
    print("%dx%d: autograd vs closed form, worst E %.2e" % (*shape, worst))


def test_closed_forms():
    """What needs no reference: the identical pair has loss 0 and gradient 0 under MSE; the terms are image_metrics' reference's; the
    planted elements pass the gradient, elements outside [0, 1] do not, and L1 contributes 0 where pred == target."""
    by_name = {n: (p, t) for n, p, t in R.inputs(45, 71, 3)}
    terms, grads = R.closed_terms(*by_name["identical_exact"])
    assert terms[0] == 0.0 and terms[1] == 0.0 and abs(terms[2]) < 1e-15 and not grads[0].any() and not grads[1].any()
    pred, target = by_name["noise0.03"]
    terms, grads = R.closed_terms(pred, target)
    row = M.reference_row(np.clip(pred, 0, 1), target)
    assert abs(terms[0] - row[1]) < 1e-15 and abs(terms[1] - row[2]) < 1e-15 and abs(1.0 - terms[2] - row[0]) < 1e-13
    outside = (pred < 0) | (pred > 1)
    assert outside.any() and not grads[:, outside].any() and np.all(grads[0][~outside] != 0)
    pred, target = by_name["planted_edges"]
    _, grads = R.closed_terms(pred, target)
    for k, _ in R.PLANTED_EDGES:
        assert all(g.reshape(-1)[k] != 0.0 for g in grads)
    pred, target = by_name["planted_equal"]
    _, grads = R.closed_terms(pred, target)
    for k in R.PLANTED_EQUAL:
        assert grads[0].reshape(-1)[k] == 0.0 and grads[1].reshape(-1)[k] == 0.0 and grads[2].reshape(-1)[k] != 0.0


def _e_torch_fp32(pred, target, weights, g64):
    """E of torch's fp32 formulation on the CPU: what the GPU tests' tolerance max(4 E_torch, 2^-20) is made of."""
    p = torch.from_numpy(pred).permute(2, 0, 1)[None].contiguous().requires_grad_(True)
    R.torch_composition(p, torch.from_numpy(target).permute(2, 0, 1)[None].contiguous(), weights).backward()
    return R.grad_error(p.grad[0].permute(1, 2, 0).numpy(), g64, weights)


# fault -> the input that exercises it, and the weightings under which it must show (the SSIM faults wherever w_ssim != 0, the clamp's
# wherever any weight is, sign(0) wherever w_l1 is)
FAULT_CASES = {"drop_gamma": ("noise0.03", [R.WEIGHTS[2], R.WEIGHTS[3]]), "seam_row": ("noise0.03", [R.WEIGHTS[2], R.WEIGHTS[3]]),
               "norm_hw": ("noise0.03", [R.WEIGHTS[2], R.WEIGHTS[3]]), "exclusive_clamp": ("planted_edges", R.WEIGHTS),
               "sign0_is_1": ("planted_equal", [R.WEIGHTS[1], R.WEIGHTS[3]])}


@pytest.mark.parametrize("fault", R.FAULTS)
def test_each_fault_moves_the_error_measure(fault):
    """The GPU tests require E_fused <= max(4 E_torch, 2^-20).  Every fault gives an E above 100 times that, at every shape and channel
    count of the GPU list, with E_torch measured here from torch's fp32 formulation on the CPU."""
    name, weightings = FAULT_CASES[fault]
    least = np.inf
    for H, W in R.gpu_shapes():
        for C in (1, 3, 4):
            pred, target = {n: (p, t) for n, p, t in R.inputs(H, W, C)}[name]
            good, bad = R.closed_terms(pred, target), R.closed_terms(pred, target, fault=fault)
            for w in weightings:
                g64, g_bad = R.combine(*good, w)[1], R.combine(*bad, w)[1]
                tolerance = max(4.0 * _e_torch_fp32(pred, target, w, g64), R.FLOOR)
                e = R.grad_error(g_bad, g64, w)
                least = min(least, e / tolerance)
                assert e > 100.0 * tolerance, (fault, H, W, C, w, e, tolerance)
    print("%s: E is at least %.0f times the GPU tolerance" % (fault, least))


def _call(L, pred=FAKE, target=FAKE, B=1, H=16, W=16, C=3, sp=True, st=True, w=(1.0, 0.5, 0.25), clamp=1, rng=1.0, grad=FAKE, sg=True,
          out=FAKE, work=FAKE, work_bytes=None, neg=None):
    strides = [(ctypes.c_long * 4)(H * W * C, W * C, C, 1) for _ in range(3)]
    if neg is not None:
        strides[neg][1] = -1
    if work_bytes is None:
        work_bytes = L.sahs_image_loss_workspace_bytes(B, H, W, C)
    return L.sahs_image_loss(pred, target, B, H, W, C, strides[0] if sp else None, strides[1] if st else None, w[0], w[1], w[2], clamp, rng,
                             grad, strides[2] if sg else None, out, work, work_bytes, None)


def test_c_abi_refuses_before_any_hip_call():
    lib = pkg("_lib")
    L = lib.lib()
    T = R.TILE
    assert L.sahs_image_loss_workspace_bytes(1, 7, 7, 1) == 3 * 8
    assert L.sahs_image_loss_workspace_bytes(1, T, T, 4) == 6 * 8 and L.sahs_image_loss_workspace_bytes(1, T + 1, T, 4) == 2 * 6 * 8
    assert L.sahs_image_loss_workspace_bytes(3, T + 7, 2 * T + 7, 3) == 3 * 2 * 3 * 5 * 8
    for bad in ((1, 6, 16, 3), (1, 16, 6, 3), (1, 16, 16, 0), (1, 16, 16, 5), (-1, 16, 16, 3), (1, 40000, 16, 3)):
        assert L.sahs_image_loss_workspace_bytes(*bad) == 0, bad
    inf, nan = float("inf"), float("nan")
    cases = {"for pred": dict(pred=None), "for target": dict(target=None), "for stride_pred": dict(sp=False), "for stride_target": dict(st=False),
             "for out": dict(out=None), "for workspace": dict(work=None), "for stride_grad": dict(sg=False), "7 <= H": dict(H=6), "7 <= H, W": dict(W=6),
             "C = 5": dict(C=5), "C = 0": dict(C=0), "ssim_data_range = 0": dict(rng=0.0), "ssim_data_range = -1": dict(rng=-1.0),
             "ssim_data_range = nan": dict(rng=nan), "w_l2 = inf": dict(w=(inf, 0.0, 0.0)), "w_l1 = nan": dict(w=(1.0, nan, 0.0)),
             "w_ssim = -inf": dict(w=(1.0, 0.0, -inf)), "needs 40": dict(work_bytes=39), "B = -1": dict(B=-1),
             "pred and target must be aligned": dict(pred=FAKE + 2), "target must be aligned": dict(target=FAKE + 1),
             "grad must be aligned": dict(grad=FAKE + 2), "8-byte aligned": dict(out=FAKE + 4), "workspace must be 8-byte": dict(work=FAKE + 4),
             "stride 1 is negative (-1, 48, grad 48)": dict(neg=0), "stride 1 is negative (48, -1, grad 48)": dict(neg=1),
             "stride 1 is negative (48, 48, grad -1)": dict(neg=2)}
    for text, kw in cases.items():
        code = _call(L, **kw)
        msg = L.sahs_last_error().decode()
        assert code == 1 and msg.startswith("sahs_image_loss:") and text in msg, (kw, code, msg)
    assert _call(L, B=0, pred=None, target=None, grad=None, out=None, work=None) == 0      # nothing to score: success without a launch


def test_python_refusals_that_need_no_gpu():
    ops, lib = pkg("ops"), pkg("_lib")
    f = torch.zeros(1, 3, 9, 9)
    with pytest.raises(lib.SahsError, match="pred must be a GPU tensor"):
        ops.image_loss(f, f)
    with pytest.raises(lib.SahsError, match="pred must be a GPU tensor"):
        ops.image_loss(np.zeros((3, 9, 9), np.float32), f)
    with pytest.raises(ValueError, match="loss must be None or a callable"):      # (a dtype in the place autocast_dtype once had)
        pkg("spade").refine_step(None, None, None, None, None, None, torch.bfloat16)
    loss = pkg("spade").RefineLoss(1, 0.5, 0.25, ssim_data_range=2.0)
    assert (loss.l2, loss.l1, loss.ssim, loss.ssim_data_range) == (1.0, 0.5, 0.25, 2.0) and repr(loss) == "RefineLoss(l2=1, l1=0.5, ssim=0.25, ssim_data_range=2)"
