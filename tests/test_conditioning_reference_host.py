"""The yardstick of tests/test_gpu_conditioning.py, checked on the host (tests/conditioning_reference.py): the float64 AudioNet and pose
encoding reproduce the reference's fixture; every case keeps its pre-activations clear of the LeakyReLU kink (or, for the one case built
for it, exactly on it); float32 CPU autograd of the same layers -- the E_f32 of the GPU rule E_hip <= max(4 * E_f32, 2^-21) -- is
printed per case and tensor; and each of three deliberately wrong backwards (slope 0.01, circular padding, the last convolution's
padding tap fed from t = 1) moves every gradient it should by more than twice that bound, at every case.

Measured on the host (float32 CPU autograd against float64, E = max |g32 - g64| / max |g64|, over the 15 cases; the figures depend on the
CPU's ATen kernels in the last digit): convolution weights up to 5.3e-7 (0 for the first one under the all-zero window), convolution
biases 7.7e-8 .. 5.5e-7, encoder_fc1.0 8.4e-8 .. 3.3e-7, encoder_fc1.2.weight 6.5e-8 .. 1.4e-7, encoder_fc1.2.bias 0, the window 1.8e-7 ..
4.2e-7; the driving vector 4.8e-8 .. 9.8e-8.  The mutants: the slope moves its tensors by 7.5e-3 .. 3.5e-2 of scale (0.5 .. 0.97 in the
exact-zero case), the two paddings by 9.0e-2 .. 2.6; the bounds they must clear twice are 4.8e-7 .. 2.2e-6."""
import numpy as np
import pytest
import torch

import conditioning_reference as C
from conftest import load_golden

CASE_IDS = ["%s-%s" % c for c in C.CASES]


def close(a, b, rtol, atol, what):
    """|a - b| <= atol + rtol |b| elementwise, as tests/test_oracle_vs_golden.py holds the C oracle to the same fixture."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err, tol = np.abs(a - b), atol + rtol * np.abs(b)
    assert np.all(err <= tol), "%s: max abs err %.3e" % (what, err.max())


def _e_f32(ref64, ref32):
    return {k: C.rel_max(ref32["grads"][k], ref64["grads"][k]) for k in ref64["grads"]}


def test_float64_reference_reproduces_the_fixture():
    """driving and pose36 of tests/golden/cond.npz (the unmodified reference on the default seed-0 weights), within test_oracle_vs_golden's bounds."""
    g = load_golden("cond")
    ref = C.reference("default", (torch.from_numpy(g["audio"]), torch.zeros(76)))
    close(ref["driving"].numpy(), g["driving"], 1e-5, 1e-6, "driving")
    close(C.pose36(torch.from_numpy(g["pose"])).numpy(), g["pose36"], 1e-6, 1e-6, "pose36")
    ref32 = C.reference("default", (torch.from_numpy(g["audio"]), torch.zeros(76)), dtype=torch.float32)
    close(ref32["driving"].numpy(), g["driving"], 1e-5, 1e-6, "driving, float32")


def test_slots_and_weight_sets():
    """The twelve tensors are the tail of the flat vector, in order; "hdr" and "default" hold one AudioNet, "seed1" another."""
    W = C.pkg("weights")
    slots = C.audio_slots()
    assert len(slots) == 12 and list(slots) == C.audio_keys()
    end = 0
    for k, (o, shp) in slots.items():
        assert end in (0, o), k
        end = o + int(np.prod(shp))
    assert end == W.param_count("audio")
    a, b, c = (C.audio_tensors(n) for n in ("hdr", "default", "seed1"))
    assert all(torch.equal(a[k], b[k]) for k in a) and all(not torch.equal(a[k], c[k]) for k in a)
    assert not np.array_equal(C.flat_weights("hdr"), C.flat_weights("default"))       # (the folded biases' layers differ)
    z = C.audio_tensors("hdr", zero_bias=True)
    assert all(float(z[k].abs().max()) == 0.0 if k.endswith(".bias") else torch.equal(z[k], a[k]) for k in z)


def test_windows():
    for name, (seed, kind) in C.WINDOWS.items():
        a, g = C.window_and_upstream(name)
        assert a.shape == (16, 29) and g.shape == (76,) and a.dtype == g.dtype == torch.float32 and not a.requires_grad
        gen = torch.Generator().manual_seed(seed)
        a0, g0 = torch.randn(16, 29, generator=gen), torch.randn(76, generator=gen)
        assert torch.equal(g, g0)
        if kind == "randn":
            assert torch.equal(a, a0)
        elif kind == "zero":
            assert float(a.abs().max()) == 0.0
        else:
            assert torch.equal(a[[0, 15]], a0[[0, 15]]) and float(a[1:15].abs().max()) == 0.0 and float(a[[0, 15]].abs().min()) > 0.0


@pytest.mark.parametrize("weights,window", C.CASES, ids=CASE_IDS)
def test_kink_condition_and_float32_error(weights, window):
    """No pre-activation within 1e-4 of its layer's scale of the kink; E_f32 per tensor is printed and is float32-sized."""
    ref64, ref32 = C.yardstick(weights, window)
    print("%s / %s: min |pre| / max |pre| %s" % (weights, window, "  ".join("%s %.2e" % (n[8:], v) for n, v in ref64["kink"].items())))
    assert list(ref64["pre"]) == list(C.PRE_NAMES)
    assert [tuple(p.shape) for p in ref64["pre"].values()] == [(32, 8), (32, 4), (64, 2), (64,), (64,)]
    assert all(v >= C.KINK_LINE for v in ref64["kink"].values()), ref64["kink"]
    for n in C.PRE_NAMES:       # and float32 is on the same side of every kink, so its gradient is one of the same function
        assert torch.equal(ref32["pre"][n] > 0, ref64["pre"][n] > 0), n
    E = _e_f32(ref64, ref32)
    print("   E_f32 %s  driving %.2e" % ("  ".join("%s %.2e" % (C.short(k), v) for k, v in E.items()), C.rel_max(ref32["driving"], ref64["driving"])))
    assert max(E.values()) <= 2e-6 and C.rel_max(ref32["driving"], ref64["driving"]) <= 1e-6
    assert E[C.PREFIX + "encoder_fc1.2.bias"] == 0.0 and torch.equal(ref64["grads"][C.PREFIX + "encoder_fc1.2.bias"], C.window_and_upstream(window)[1].double())
    if C.WINDOWS[window][1] == "zero":
        assert float(ref64["grads"][C.PREFIX + "encoder_conv.0.weight"].abs().max()) == 0.0


def test_exact_zero_case_sits_on_the_kink():
    """All-zero window, zeroed biases: every pre-activation is exactly 0 in both precisions, the derivative taken there is the slope
    (each bias gradient is 0.02 x the one of the layer after it, down to 0.02^5 at the first convolution), every weight gradient is 0."""
    ref64, ref32 = C.yardstick(*C.EXACT_ZERO, True)
    for ref in (ref64, ref32):
        assert all(float(p.abs().max()) == 0.0 for p in ref["pre"].values())
        assert float(ref["driving"].abs().max()) == 0.0
        for k, v in ref["grads"].items():
            assert (float(v.abs().max()) == 0.0) == k.endswith(".weight"), k
    g = C.window_and_upstream("zero")[1].double()
    sd = C.audio_tensors("hdr", True)
    want = 0.02 * (sd[C.PREFIX + "encoder_fc1.2.weight"].t() @ g)
    assert C.rel_max(ref64["grads"][C.PREFIX + "encoder_fc1.0.bias"], want) <= 1e-15
    want = 0.02 * (sd[C.PREFIX + "encoder_fc1.0.weight"].t() @ want)
    assert C.rel_max(ref64["grads"][C.PREFIX + "encoder_conv.6.bias"], want) <= 1e-15
    E = _e_f32(ref64, ref32)
    print("exact zero: E_f32 %s" % "  ".join("%s %.2e" % (C.short(k), v) for k, v in E.items()))
    assert max(E.values()) <= 2e-6


@pytest.mark.parametrize("weights,window", C.CASES, ids=CASE_IDS)
def test_last_conv_padding_tap_gets_no_gradient(weights, window):
    """encoder_conv.6 maps length 2 to length 1: its k = 0 tap reads the padding, so that column of its weight gradient is exactly 0."""
    ref64, ref32 = C.yardstick(weights, window)
    for ref in (ref64, ref32):
        gw = ref["grads"][C.PREFIX + "encoder_conv.6.weight"]
        assert gw.shape == (64, 64, 3) and float(gw[:, :, 0].abs().max()) == 0.0 and float(gw[:, :, 1].abs().max()) > 0.0
    assert float(C.reference(weights, window, mutant="last_tap")["grads"][C.PREFIX + "encoder_conv.6.weight"][:, :, 0].abs().max()) > 0.0


@pytest.mark.parametrize("mutant", C.MUTANTS)
@pytest.mark.parametrize("weights,window", C.CASES, ids=CASE_IDS)
def test_mutants_fail_the_rule(weights, window, mutant):
    """Every tensor the mutant should move is off float64 by more than twice the bound the GPU test holds the kernel to."""
    ref64, ref32 = C.yardstick(weights, window)
    E = _e_f32(ref64, ref32)
    bad = C.reference(weights, window, mutant=mutant)["grads"]
    rows = [(k, C.rel_max(bad[k], ref64["grads"][k]), C.bound(E[k])) for k in C.moved_by(mutant, window)]
    print("%s / %s, %s: %s" % (weights, window, mutant, "  ".join("%s %.1e (bound %.1e)" % (C.short(k), e, b) for k, e, b in rows)))
    assert len(rows) >= 10
    for k, e, b in rows:
        assert e > 2.0 * b, (k, e, b)


def test_slope_mutant_fails_at_the_kink():
    ref64, ref32 = C.yardstick(*C.EXACT_ZERO, True)
    E = _e_f32(ref64, ref32)
    bad = C.reference(*C.EXACT_ZERO, True, mutant="slope")["grads"]
    keys = C.moved_by("slope", C.EXACT_ZERO[1], True)
    assert len(keys) == 6       # five biases and the window
    for k in keys:
        assert C.rel_max(bad[k], ref64["grads"][k]) > 2.0 * C.bound(E[k]), k


def test_poses():
    """Shapes, exact entries of the quarter turns, finite encodings in both precisions; float32's own error per pose is printed."""
    P = C.poses()
    assert [tuple(p.shape) for p in P.values()].count((4, 4)) == 1 and torch.equal(P["euler1_4x4"][:3], P["euler1"])
    assert torch.equal(P["identity"], torch.tensor([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0.8]]))
    for n, p in P.items():
        assert p.dtype == torch.float32 and p.shape[1] == 4 and float(p[:3, 3].abs().max()) <= 1.0
        R = p[:3, :3].double()
        assert float((R @ R.t() - torch.eye(3, dtype=torch.float64)).abs().max()) <= 2e-7 and abs(float(torch.linalg.det(R)) - 1.0) <= 3e-7, n
        if n.startswith("quarter"):
            assert sorted(R.abs().flatten().tolist()) == [0.0] * 6 + [1.0] * 3 and not bool(torch.signbit(p).logical_and(p == 0).any()), n
        e64, e32 = C.pose36(p), C.pose36(p, torch.float32)
        assert e64.shape == (36,) and bool(torch.isfinite(e64).all()) and bool(torch.isfinite(e32).all())
        print("%s: float32 |pose36 - float64| %.2e" % (n, float((e32.double() - e64).abs().max())))
    assert float(P["quarter_y"][0, 2]) == 1.0 and float(P["quarter_y_back"][0, 2]) == -1.0      # asin(-+1), the ends of its domain
    assert abs(float(C.pose36(P["quarter_y"])[1]) + 1.0) <= 1e-15                                  # sin(asin(-1)) = -1
    assert float(P["quarter_x"][2, 2]) == 0.0 and float(P["quarter_x"][1, 2]) == -1.0          # atan2(0, -1) = pi
