"""CPU-side checks of LPIPS as a training term: the closed-form head gradient of tests/lpips_grad_reference.py against float64 autograd of
the safe-sqrt statement and against a central difference at an all-zero pixel, the NaN of the published formula's autograd there, the
exact zero for equal operands, the new C entries' refusals (before any HIP call) and the header's new declarations against _lib.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import lpips_grad_reference as G
import lpips_reference as R
from conftest import REPO, pkg

FAKE = 0x10000      # a non-null, 8-byte-aligned address that is never dereferenced: every call below is refused before any HIP call
NEW_ENTRIES = ["sahs_lpips_prepare_loss", "sahs_lpips_prepare_grad", "sahs_lpips_head_stats_bytes", "sahs_lpips_head_forward",
               "sahs_lpips_head_backward"]
UPSTREAM = np.array([0.7, -1.3])


@pytest.mark.parametrize("shape", [(37, 5, 7), (5, 3, 3), (64, 1, 1), (384, 1, 3)], ids=lambda s: "%dx%dx%d" % s)
def test_closed_form_is_autograd_of_the_safe_head(shape):
    C, h, w = shape
    fa, fb, lw = G.head_case(2, C, h, w, 11)
    assert G.dead_pixels(fa).any()
    closed, auto = G.closed_head_grad(fa, fb, lw, UPSTREAM), G.autograd_head_grad(fa, fb, lw, UPSTREAM)
    assert np.all(np.isfinite(closed)) and np.all(np.isfinite(auto))
    err = np.abs(closed - auto).max() / np.abs(auto).max()
    print("closed form against float64 autograd of the safe head, C=%d %dx%d: %.2e of the largest element" % (C, h, w, err))
    assert err <= 1e-13


def test_closed_form_is_a_central_difference_at_a_dead_pixel():
    """At a pixel whose a is all zero, a -> a / (|a| + eps) is a / eps - a |a| / eps^2 + ...: a central difference of step h along
    one channel is the derivative times (1 - h / eps + ...), and its rounding error is that of two values of size d divided by 2h.
    h = 1e-15 is small against eps = 1e-10; tolerance 4 (h / eps) m + 2^-50 d / h, m the pixel's largest derivative."""
    fa, fb, lw = G.head_case(1, 37, 5, 7, 11)
    assert not fa[0, :, -1, -1].any() and fb[0, :, -1, -1].any()
    a, b, w = np.zeros(37), fb[0, :, -1, -1].astype(np.float64), lw.astype(np.float64)
    closed = G.closed_head_grad(fa, fb, lw, [1.0])[0, :, -1, -1] * 35      # (the pixel's own d: undo the mean over 5 x 7 pixels)

    def d(a):
        return float((w * (a / (np.sqrt((a * a).sum()) + G.EPS) - b / (np.sqrt((b * b).sum()) + G.EPS)) ** 2).sum())

    h, m = 1e-15, np.abs(closed).max()
    assert m > 1e6      # (2 w b^ / 1e-10: large, and finite)
    for k in range(37):
        step = np.zeros(37)
        step[k] = h
        numeric = (d(a + step) - d(a - step)) / (2 * h)
        assert abs(numeric - closed[k]) <= 4 * (h / G.EPS) * m + 2.0 ** -50 * d(a) / h, (k, numeric, closed[k])


def test_naive_autograd_is_nan_exactly_at_the_dead_pixels():
    """Why the yardstick is the safe statement: the published formula's own autograd gives NaN in every channel of a pixel that is all
    zero in the first operand (sqrt's derivative at 0 is inf, behind it 0 * inf), and agrees with the closed form everywhere else."""
    f, lw = R.synthetic_features(2, 37, 5, 7, 11)
    fa, fb = f[:2], f[2:]
    dead = G.dead_pixels(fa)
    naive = G.autograd_head_grad(fa, fb, lw, UPSTREAM, head=G.naive_head)
    closed = G.closed_head_grad(fa, fb, lw, UPSTREAM)
    per_image = [int(np.isnan(naive[i]).sum()) for i in range(2)]
    print("naive float64 autograd: %s NaN elements for %s dead pixels" % (per_image, [int(dead[i].sum()) for i in range(2)]))
    assert dead.sum() >= 2 and per_image == [37 * int(dead[i].sum()) for i in range(2)]
    assert np.array_equal(np.isnan(naive), np.broadcast_to(dead[:, None], naive.shape))
    alive = ~np.isnan(naive)
    assert np.abs(naive[alive] - closed[alive]).max() <= 1e-13 * np.abs(closed).max() and np.all(np.isfinite(closed))


GPU_PIXELS = [(1, 1), (1, 3), (7, 7), (15, 16), (16, 16), (16, 17)]      # tests/test_gpu_lpips_loss.py: PIXELS, and its C and seed


@pytest.mark.parametrize("C", [5, 64, 384])
def test_kernel_order_meets_the_gpu_rule_on_the_gpu_cases(C):
    """The GPU test's rule, |got - ref| <= 2^-23 |ref| + 2^-40 m, is met by the kernel's evaluation order written in numpy, on the GPU
    test's own inputs; those inputs have no pixel whose a^ and b^ agree to rounding (lpips_grad_reference.head_case on why)."""
    g = np.array([0.7, -1.3], np.float32).astype(np.float64)
    for hw in GPU_PIXELS:
        fa, fb, lw = G.head_case(2, C, *hw, 40)
        assert G.separation(fa, fb) >= 2.0 ** -10, (hw, C, G.separation(fa, fb))
        worst = G.head_rule(G.kernel_order_head_grad(fa, fb, lw, g), G.closed_head_grad(fa, fb, lw, g))
        print("kernel order in numpy, %s C=%d: worst error %.3f of the rule" % (hw, C, worst))
        assert worst <= 1.0, (hw, C, worst)
    fa, _, lw = G.head_case(2, C, 7, 7, 40)
    assert not G.kernel_order_head_grad(fa, fa.copy(), lw, g).any()      # equal operands: exactly 0 in this order too


def test_equal_operands_give_exactly_zero():
    fa, _, lw = G.head_case(2, 37, 5, 7, 12)
    assert not G.closed_head_grad(fa, fa.copy(), lw, UPSTREAM).any()
    assert not G.autograd_head_grad(fa, fa.copy(), lw, UPSTREAM).any()
    # and the whole chain: an identical pair has loss 0 and no gradient, in float64
    model = pkg("metrics").LPIPS.from_seed(0)
    a, b = R.identical_pair(31, 31, np.float32)
    loss, per_image, grad, _ = G.chain64(a[None], b[None], model, False)
    assert loss == 0.0 and not per_image.any() and not grad.any()


def test_chain64_is_the_forward_reference_and_negative_biases_leave_dead_pixels():
    model = pkg("metrics").LPIPS.from_seed(0)
    items = R.content(45, 71, np.float32)
    a, b = np.stack([x for _, x, _ in items]), np.stack([y for _, _, y in items])
    for normalize in (False, True):
        loss, per_image, grad, _ = G.chain64(a, b, model, normalize)      # (the content lies in [0, 1]: the clamp changes nothing)
        rows = R.reference_rows(a, b, model, normalize)
        assert np.abs(per_image - rows[:, 0]).max() <= 1e-13 * rows[:, 0].max() and abs(loss - rows[:, 0].mean()) <= 1e-13
        assert np.all(np.isfinite(grad)) and grad.shape == a.shape
    name, a, b = items[4]
    assert name == "constant"
    _, _, grad, maps = G.chain64(a[None], b[None], model, False, conv_weights=G.negative_bias_convs(model))
    counts = [(int(G.dead_pixels(m).sum()), m.shape[2] * m.shape[3]) for m in maps]
    print("negative biases, the constant-region pair at 45 x 71: dead pixels per layer %s" % counts)
    assert counts == [(100, 170), (12, 32), (1, 3), (3, 3), (3, 3)] and np.all(np.isfinite(grad))


def _strides(H, W, C=3):
    return (ctypes.c_long * 4)(H * W * C, W * C, C, 1)


def _prepare_loss(L, pred=FAKE, target=FAKE, dtype=1, B=1, H=31, W=31, C=3, sp=True, st=True, out=FAKE, neg=None):
    s = [_strides(H, W, C), _strides(H, W, C)]
    if neg is not None:
        s[neg][1] = -1
    return L.sahs_lpips_prepare_loss(pred, target, dtype, B, H, W, C, s[0] if sp else None, s[1] if st else None, 0, 1, out, None)


def _prepare_grad(L, pred=FAKE, gx=FAKE, B=1, H=31, W=31, C=3, sp=True, grad=FAKE, sg=True, neg=None):
    s = [_strides(H, W, C), _strides(H, W, C)]
    if neg is not None:
        s[neg][1] = -1
    return L.sahs_lpips_prepare_grad(pred, gx, B, H, W, C, s[0] if sp else None, 0, 1, grad, s[1] if sg else None, None)


def _tables(f, w, C, hw):
    n = len(C)
    return (ctypes.c_void_p * n)(*f), (ctypes.c_void_p * n)(*w), (ctypes.c_int * n)(*C), (ctypes.c_long * n)(*hw)


def _forward(L, jobs=2, fa=(FAKE, FAKE), fb=(FAKE, FAKE), w=(FAKE, FAKE), C=(64, 192), hw=(49, 9), B=1, out=FAKE, stats=FAKE, stats_bytes=None,
             work=FAKE, work_bytes=None, tables=(True, True)):
    pa, pw, Cs, hws = _tables(fa, w, C, hw)
    pb = (ctypes.c_void_p * len(C))(*fb)
    if work_bytes is None:
        work_bytes = L.sahs_lpips_distance_workspace_bytes(jobs, B, hws)
    if stats_bytes is None:
        stats_bytes = L.sahs_lpips_head_stats_bytes(jobs, B, hws)
    return L.sahs_lpips_head_forward(jobs, pa if tables[0] else None, pb if tables[1] else None, pw, Cs, hws, B, out, stats, stats_bytes, work,
                                     work_bytes, None)


def _backward(L, jobs=2, fa=(FAKE, FAKE), fb=(FAKE, FAKE), w=(FAKE, FAKE), C=(64, 192), hw=(49, 9), B=1, g=FAKE, g_is_double=0, stats=FAKE,
              stats_bytes=None, grads=(FAKE, FAKE), grad_table=True):
    pa, pw, Cs, hws = _tables(fa, w, C, hw)
    pb, pg = (ctypes.c_void_p * len(C))(*fb), (ctypes.c_void_p * len(C))(*grads)
    if stats_bytes is None:
        stats_bytes = L.sahs_lpips_head_stats_bytes(jobs, B, hws)
    return L.sahs_lpips_head_backward(jobs, pa, pb, pw, Cs, hws, B, g, g_is_double, stats, stats_bytes, pg if grad_table else None, None)


def _refused(L, call, who, cases):
    for text, kw in cases.items():
        code = call(L, **kw)
        msg = L.sahs_last_error().decode()
        assert code == 1 and msg.startswith(who + ":") and text in msg, (kw, code, msg)


def test_c_abi_refuses_before_any_hip_call():
    L = pkg("_lib").lib()
    T = R.TILE
    hw = (ctypes.c_long * 5)(1, T - 16, T, T + 16, 961)
    pixels = 1 + T - 16 + T + T + 16 + 961
    assert L.sahs_lpips_head_stats_bytes(5, 1, hw) == 24 * pixels and L.sahs_lpips_head_stats_bytes(5, 3, hw) == 3 * 24 * pixels
    assert L.sahs_lpips_head_stats_bytes(2, 3, hw) == 3 * 24 * (1 + T - 16)
    for bad in ((0, 1, hw), (6, 1, hw), (5, -1, hw), (5, 1, None), (1, 1, (ctypes.c_long * 1)(0)), (1, 1 << 31, (ctypes.c_long * 1)(1))):
        assert L.sahs_lpips_head_stats_bytes(*bad) == 0, bad
    _refused(L, _prepare_loss, "sahs_lpips_prepare_loss", {
        "C = 4": dict(C=4), "target_dtype = 2": dict(dtype=2), "30 x 64": dict(H=30, W=64), "64 x 30": dict(H=64, W=30), "for pred ": dict(pred=None),
        "for target ": dict(target=None), "for stride_pred": dict(sp=False), "for stride_target": dict(st=False), "for out": dict(out=None),
        "B = -1": dict(B=-1), "4-byte": dict(pred=FAKE + 2), "pred, target and out must be aligned": dict(target=FAKE + 1),
        "stride 1 is negative (-1, 93)": dict(neg=0), "stride 1 is negative (93, -1)": dict(neg=1)})
    assert _prepare_loss(L, dtype=0, target=FAKE + 1, B=0) == 0 and _prepare_loss(L, B=0, pred=None, target=None, out=None) == 0
    _refused(L, _prepare_grad, "sahs_lpips_prepare_grad", {
        "C = 1": dict(C=1), "30 x 64": dict(H=30, W=64), "for pred": dict(pred=None), "for gx": dict(gx=None), "for stride_pred": dict(sp=False),
        "for grad ": dict(grad=None), "for stride_grad": dict(sg=False), "B = -1": dict(B=-1), "4-byte": dict(gx=FAKE + 2),
        "pred, gx and grad must be aligned": dict(grad=FAKE + 1), "stride 1 is negative (-1, grad 93)": dict(neg=0),
        "stride 1 is negative (93, grad -1)": dict(neg=1)})
    assert _prepare_grad(L, B=0, pred=None, gx=None, grad=None) == 0
    shared = {"jobs = 6": dict(jobs=6, fa=(FAKE,) * 6, fb=(FAKE,) * 6, w=(FAKE,) * 6, C=(4,) * 6, hw=(4,) * 6), "jobs = 0": dict(jobs=0),
              "job 1 has C = 0": dict(C=(64, 0)), "job 0 has C = 1025": dict(C=(1025, 4)), "job 1 has hw = 0": dict(hw=(49, 0)),
              "job 0 has hw = 1073741825": dict(hw=((1 << 30) + 1, 9)), "B * tiles < 2^31": dict(B=1 << 31), "B = -1": dict(B=-1),
              "fa[1]": dict(fa=(FAKE, None)), "fb[0]": dict(fb=(None, FAKE)), "weights[0]": dict(w=(None, FAKE)),
              "fa[0], fb[0] and weights[0] must be aligned": dict(fb=(FAKE + 2, FAKE)), "needs 1392": dict(stats_bytes=1391)}
    _refused(L, _forward, "sahs_lpips_head_forward", dict(shared, **{
        "for fa": dict(tables=(False, True)), "for fb": dict(tables=(True, False)), "for out": dict(out=None), "for workspace": dict(work=None),
        "needs 16": dict(work_bytes=15), "8-byte aligned": dict(out=FAKE + 4), "out, stats and workspace": dict(stats=FAKE + 4)}))
    assert _forward(L, B=0, out=None, work=None, stats=None) == 0
    _refused(L, _backward, "sahs_lpips_head_backward", dict(shared, **{
        "for g ": dict(g=None), "for stats": dict(stats=None), "for grad_a": dict(grad_table=False), "grad_a[1]": dict(grads=(FAKE, None)),
        "grad_a[0] must be aligned": dict(grads=(FAKE + 2, FAKE)), "g aligned to its 8-byte": dict(g=FAKE + 4, g_is_double=1),
        "g aligned to its 4-byte": dict(g=FAKE + 2), "stats must be 8-byte aligned": dict(stats=FAKE + 4)}))
    assert _backward(L, B=0, g=None, stats=None) == 0 and L.sahs_lpips_head_stats_bytes(2, 1, (ctypes.c_long * 2)(49, 9)) == 1392


def test_new_declarations_agree_with_the_ctypes_signatures():
    """Each new entry is declared once in the header, and _lib.SIGNATURES gives it the same return type and arguments."""
    lib = pkg("_lib")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sahs_nerf.h")).read(), flags=re.S)

    def ctype(decl):
        decl = decl.strip()
        if "*" in decl:
            return ctypes.c_void_p
        return {"int": ctypes.c_int, "long": ctypes.c_long, "size_t": ctypes.c_size_t, "double": ctypes.c_double}[decl.split()[0]]

    for name in NEW_ENTRIES:
        found = re.findall(r"(\w+)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
        assert len(found) == 1, "%s is declared %d times" % (name, len(found))
        ret, args = found[0]
        restype, argtypes = lib.SIGNATURES[name]
        assert restype is ctype(ret) and list(argtypes) == [ctype(a) for a in args.split(",")], name
    launchers = open(os.path.join(REPO, "sahs-deformable-nerf_amd", "csrc", "sahs_launchers.hpp")).read()
    for name in ("sahs_lpips_prepare_launch", "sahs_lpips_prepare_grad_launch", "sahs_lpips_head_forward_launch", "sahs_lpips_head_backward_launch"):
        assert len(re.findall(r"\b%s\s*\(" % name, launchers)) == 1, name


def test_python_refusals_that_need_no_gpu():
    ops, lib, S, M = pkg("ops"), pkg("_lib"), pkg("spade"), pkg("metrics")
    f = torch.zeros(1, 3, 31, 31)
    with pytest.raises(lib.SahsError, match="lpips_prepare_loss: pred must be a GPU tensor"):
        ops.lpips_prepare_loss(f, f)
    with pytest.raises(lib.SahsError, match=r"lpips_head: fa\[0\] must be a GPU tensor"):
        ops.lpips_head([torch.zeros(1, 4, 3, 3)], [torch.zeros(1, 4, 3, 3)], [torch.zeros(4)])
    with pytest.raises(lib.SahsError, match="1 fa, 2 fb and 1 weight tensors"):
        ops.lpips_head([f], [f, f], [f])
    with pytest.raises(lib.SahsError, match="GPU"):
        M.LPIPS.from_seed(0).loss(f, f)
    with pytest.raises(ValueError, match="lpips = 0.5 needs lpips_model"):
        S.RefineLoss(1, lpips=0.5)
    # lpips == 0: the object is, and prints as, the one without the term
    plain, zero = S.RefineLoss(1, 0.5, 0.25, ssim_data_range=2.0), S.RefineLoss(1, 0.5, 0.25, ssim_data_range=2.0, lpips=0.0)
    assert repr(zero) == repr(plain) == "RefineLoss(l2=1, l1=0.5, ssim=0.25, ssim_data_range=2)"
    with_term = S.RefineLoss(1, lpips=0.5, lpips_model=M.LPIPS.from_seed(0))
    assert with_term.lpips == 0.5 and repr(with_term) == "RefineLoss(l2=1, l1=0, ssim=0, ssim_data_range=1, lpips=0.5)"
