"""The two conditioning kernels against float64 (yardstick and inputs: tests/conditioning_reference.py, checked on the host by
tests/test_conditioning_reference_host.py): ``conditioning_backward_kernel`` (csrc/train_bwd.hip; grad_cond[0:76] through AudioNet into
twelve parameter tensors and the audio window) through the C ABI itself, and ``fold_conditioning_kernel`` (csrc/pack.hip; AudioNet, the
Euler / translation pose encoding, the folded biases).

The rule for every AudioNet result: with E = max |hip - f64| / max |f64|, E_hip <= max(4 * E_f32, 2^-21), E_f32 being float32 CPU
autograd (or the float32 CPU forward) of the same case.  The kernels are plain fp32 without atomics, so they and ATen differ by the
order of a few sums: the 4 is what this project grants two correct fp32 summation orders (tests/test_gpu_spade_backward.py), 2^-21
covers results with no long sum in them (encoder_fc1.2.bias is a copy of g: E_f32 = 0).  A wrong term -- a padding tap, a parity of
the transposed convolution, a kink read from the wrong buffer, a slope -- moves E by orders of magnitude: the host file shows three
such mutants missing twice this bound at every case.  A gradient float64 says is identically zero must be exactly zero.  The pose
encoding is held to max(4 x the float32 CPU evaluation's own error on that pose, 1e-6) absolute.  The argument contracts of the C ABI
(`+=` into grad_flat and grad_audio, grad_audio == NULL, only grad_cond[0:76] read, pose_ld) are held bit for bit.

Measured on an MI355X (each test prints its figures before it asserts; DESIGN.md section 4 has them too).  Worst E_hip over the 15
cases (three weight sets, two of them with the same AudioNet, x five windows) and the exact-zero case, with E_f32 of that very tensor
and case in brackets; no kernel fault was found:
  backward: convolution weights 7.9e-7 (7.5e-7), convolution biases 6.4e-7 (6.4e-7), encoder_fc1.0.weight 5.9e-7 (3.0e-7),
  encoder_fc1.0.bias 2.2e-7 (2.2e-7), encoder_fc1.2.weight 4.2e-7 (8.5e-8: under the 2^-21 = 4.8e-7 floor, at 0.87 of it),
  encoder_fc1.2.bias 0 (0), the window 5.3e-7 (3.2e-7), its rows 0 and 15 against their own scale 8.9e-7 (8.9e-7) and 9.4e-7 (9.4e-7);
  E_hip = E_f32 to three digits in 127 of the 240 figures, the exact zeros among them (the worst entry is the same fp32 number in
  both).  At the kink: every weight gradient exactly 0, the biases and the window 1.7e-7 .. 6.5e-7 (1.7e-7 .. 6.5e-7).  The k = 0
  column of encoder_conv.6.weight: 0.0 in all 15.
  forward: driving vector 2.6e-7 .. 4.2e-7 (E_f32 6.0e-8 .. 9.1e-8): the kernel adds each output as one k-ordered fmaf chain of up to
  192 terms where ATen adds in blocks, which is 3 .. 7 x float32 CPU's error and passes on the floor, at 0.88 of it at the worst;
  pose36 worst |hip - f64| 4.0e-7 (float32 CPU 3.5e-7 on that pose), on the four quarter turns 1.8e-7 .. 3.5e-7, float32 CPU's own
  to three digits (4 x the rounding of pi), the same for the three architectures; of a frame's 9,184 / 7,136 / 4,768 words all but the
  16 padding words [76:80], [116:128] are written.
  The file: 83 tests, 3.7 s of wall time (the float64 and float32 yardsticks on the CPU included).
"""
import functools

import numpy as np
import pytest
import torch

import conditioning_reference as C
from conftest import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASE_IDS = ["%s-%s" % c for c in C.CASES]
ARCHS = ("audio", "nerface", "nerface_static")
GUARD = 64                  # sentinel words on either side of a buffer a kernel writes
POSE_FLOOR = 1e-6           # what test_gpu_parity.py::test_conditioning holds pose36 to at the golden pose


@functools.lru_cache(maxsize=None)
def _flat(weights, zero_bias=False):
    return torch.from_numpy(C.flat_weights(weights, zero_bias).copy()).to(DEV)


@functools.lru_cache(maxsize=None)
def _flat_of(arch):
    """The weights the forward tests give each architecture."""
    if arch == "audio":
        return _flat("hdr")
    W = pkg("weights")
    return torch.from_numpy(W.flatten_state_dict(W.hash_state_dict(0, 8.0, 30.0, model=arch), model=arch)).to(DEV)


def _guarded(words, fill):
    """-> (whole buffer, the view of ``words`` words in its middle), every word of the buffer = fill(n) first."""
    whole = fill(words + 2 * GUARD)
    return whole, whole[GUARD:GUARD + words]


def _guards_intact(whole, before):
    return torch.equal(whole[:GUARD], before[:GUARD]) and torch.equal(whole[-GUARD:], before[-GUARD:])


def _backward(flat, audio, grad_cond, grad_flat, grad_audio):
    """sahs_conditioning_backward as ops._driving_grad calls it, on the caller's buffers (grad_audio may be None: NULL)."""
    ops, lib = pkg("ops"), pkg("_lib")
    for t in (flat, audio, grad_cond, grad_flat) + (() if grad_audio is None else (grad_audio,)):
        assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
    assert flat.numel() == grad_flat.numel() == ops.param_count("audio") and audio.shape == (16, 29) and grad_cond.numel() >= 76
    assert grad_audio is None or grad_audio.numel() == 16 * 29
    lib.check(lib.lib().sahs_conditioning_backward(ops._p(flat), ops._p(audio), ops._p(grad_cond), ops._p(grad_flat), ops._p(grad_audio),
                                                   ops._stream()), "sahs_conditioning_backward")
    torch.cuda.synchronize()


def _inputs(weights, window, zero_bias=False, tail=0.0):
    a, g = C.window_and_upstream(window)
    grad_cond = torch.full((116,), tail)
    grad_cond[:76] = g
    return _flat(weights, zero_bias), a.to(DEV), grad_cond.to(DEV)


def _split(grad_flat, grad_audio):
    out = {k: grad_flat[o:o + int(np.prod(shp))].reshape(shp).cpu() for k, (o, shp) in C.audio_slots().items()}
    out["audio"] = None if grad_audio is None else grad_audio.reshape(16, 29).cpu()
    return out


@functools.lru_cache(maxsize=None)
def _hip_grads(weights, window, zero_bias=False):
    """One call into zeroed buffers -> {the twelve keys + "audio": CPU tensor}; every word outside the twelve slots must still be 0."""
    flat, audio, grad_cond = _inputs(weights, window, zero_bias)
    grad_flat = torch.zeros_like(flat)
    whole, grad_audio = _guarded(16 * 29, lambda n: torch.zeros(n, device=DEV))
    _backward(flat, audio, grad_cond, grad_flat, grad_audio)
    first = next(iter(C.audio_slots().values()))[0]
    assert float(grad_flat[:first].abs().max()) == 0.0 and float(whole[:GUARD].abs().max()) == 0.0 and float(whole[-GUARD:].abs().max()) == 0.0
    return _split(grad_flat, grad_audio)


def _hold_to_float64(got, ref64, ref32, what):
    rows = [(C.short(k), C.rel_max(got[k], ref64["grads"][k]), C.rel_max(ref32["grads"][k], ref64["grads"][k])) for k in ref64["grads"]]
    for r in (0, 15):       # the window's rows next to the padding, each against its own scale
        rows.append(("audio[%d]" % r, C.rel_max(got["audio"][r], ref64["grads"]["audio"][r]), C.rel_max(ref32["grads"]["audio"][r], ref64["grads"]["audio"][r])))
    print("%s: E_hip (E_f32)  %s" % (what, "  ".join("%s %.2e (%.2e)" % r for r in rows)))
    for k, v in ref64["grads"].items():
        assert bool(torch.isfinite(got[k]).all()), k
        if float(v.abs().max()) == 0.0:
            assert float(got[k].abs().max()) == 0.0, "%s: %s is identically zero in float64" % (what, k)
    bad = ["%s E_hip %.3e > max(4 x %.3e, 2^-21)" % r for r in rows if not r[1] <= C.bound(r[2])]
    assert not bad, "%s: %s" % (what, "; ".join(bad))


# ---------------------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights,window", C.CASES, ids=CASE_IDS)
def test_backward_vs_float64(weights, window):
    """The thirteen gradients of one call into zeroed buffers, each against float64 autograd under the rule."""
    ref64, ref32 = C.yardstick(weights, window)
    assert all(v >= C.KINK_LINE for v in ref64["kink"].values()), ref64["kink"]
    _hold_to_float64(_hip_grads(weights, window), ref64, ref32, "%s / %s" % (weights, window))


def test_backward_at_the_kink():
    """All-zero window, zeroed AudioNet biases: every pre-activation is exactly 0 and the derivative there is the slope 0.02."""
    ref64, ref32 = C.yardstick(*C.EXACT_ZERO, True)
    assert all(float(p.abs().max()) == 0.0 for p in ref64["pre"].values())
    got = _hip_grads(*C.EXACT_ZERO, True)
    _hold_to_float64(got, ref64, ref32, "exact zero")
    assert all(float(got[k].abs().max()) == 0.0 for k in got if k.endswith(".weight"))
    assert all(float(got[k].abs().max()) > 0.0 for k in got if not k.endswith(".weight"))


@pytest.mark.parametrize("weights,window", C.CASES, ids=CASE_IDS)
def test_last_conv_padding_tap_is_exactly_zero(weights, window):
    """encoder_conv.6 maps length 2 to length 1; its k = 0 tap reads the padding and gets no gradient."""
    gw = _hip_grads(weights, window)[C.PREFIX + "encoder_conv.6.weight"]
    assert gw.shape == (64, 64, 3)
    print("%s / %s: max |d conv.6.weight| per tap %s" % (weights, window, ["%.3e" % float(gw[:, :, k].abs().max()) for k in range(3)]))
    assert bool((gw[:, :, 0] == 0.0).all()) and float(gw[:, :, 1].abs().max()) > 0.0 and float(gw[:, :, 2].abs().max()) > 0.0


@pytest.mark.parametrize("weights,window", [("hdr", "seed0"), ("seed1", "ends")], ids=["hdr-seed0", "seed1-ends"])
def test_accumulates_and_touches_nothing_else(weights, window):
    """`+=` into grad_flat and grad_audio, and nothing written anywhere else."""
    flat, audio, grad_cond = _inputs(weights, window)
    one = _hip_grads(weights, window)
    first = next(iter(C.audio_slots().values()))[0]
    gen = torch.Generator(device=DEV).manual_seed(11)
    rnd = lambda n: torch.randn(n, device=DEV, generator=gen)
    # a finite random sentinel everywhere: outside the twelve slots not a bit moves; inside them one IEEE addition per word
    grad_flat = rnd(flat.numel())
    whole, grad_audio = _guarded(16 * 29, rnd)
    before_flat, before_whole = grad_flat.clone(), whole.clone()
    _backward(flat, audio, grad_cond, grad_flat, grad_audio)
    assert bool(torch.isfinite(before_flat).all())
    assert torch.equal(grad_flat[:first], before_flat[:first]) and _guards_intact(whole, before_whole)
    after = _split(grad_flat, grad_audio)
    start = _split(before_flat, before_whole[GUARD:GUARD + 16 * 29])
    for k in one:
        assert torch.equal(after[k], start[k] + one[k]), k
    # two calls into the same zeroed buffers: g + g is exact in fp32 and the kernel has no atomics
    grad_flat = torch.zeros_like(flat)
    whole, grad_audio = _guarded(16 * 29, lambda n: torch.zeros(n, device=DEV))
    _backward(flat, audio, grad_cond, grad_flat, grad_audio)
    again = _split(grad_flat, grad_audio)
    _backward(flat, audio, grad_cond, grad_flat, grad_audio)
    twice = _split(grad_flat, grad_audio)
    assert float(grad_flat[:first].abs().max()) == 0.0 and float(whole[:GUARD].abs().max()) == 0.0 and float(whole[-GUARD:].abs().max()) == 0.0
    for k in one:
        assert torch.equal(again[k], one[k]), k                   # two separate one-call runs: the same bits
        assert torch.equal(twice[k], 2.0 * one[k]), k
    print("%s / %s: %d words outside the slots untouched; one call twice == 2 x one call in all 13 tensors" % (weights, window, first))


@pytest.mark.parametrize("weights,window", [("hdr", "seed2"), ("seed1", "zero")], ids=["hdr-seed2", "seed1-zero"])
def test_null_grad_audio_and_grad_cond_tail(weights, window):
    """grad_audio == NULL changes no parameter gradient; grad_cond[76:116] (the pose encoding's gradient and the padding) is never read."""
    one = _hip_grads(weights, window)
    flat, audio, grad_cond = _inputs(weights, window)
    grad_flat = torch.zeros_like(flat)
    _backward(flat, audio, grad_cond, grad_flat, None)
    got = _split(grad_flat, None)
    for k in C.audio_keys():
        assert torch.equal(got[k], one[k]), k
    flat, audio, poisoned = _inputs(weights, window, tail=float("nan"))
    assert poisoned.numel() == 116 and bool(torch.isnan(poisoned[76:]).all()) and torch.equal(poisoned[:76], grad_cond[:76])
    grad_flat = torch.zeros_like(flat)
    whole, grad_audio = _guarded(16 * 29, lambda n: torch.zeros(n, device=DEV))
    _backward(flat, audio, poisoned, grad_flat, grad_audio)
    assert bool(torch.isfinite(grad_flat).all()) and bool(torch.isfinite(whole).all())
    got = _split(grad_flat, grad_audio)
    for k in one:
        assert torch.equal(got[k], one[k]), k


# ---------------------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------------------
def _identity():
    return C.poses()["identity"].to(DEV)


@pytest.mark.parametrize("weights,window", C.CASES, ids=CASE_IDS)
def test_driving_vs_float64(weights, window):
    """frame[0:76] of the AudioFaceModel against float64 AudioNet, as close as the float32 CPU forward is."""
    ops = pkg("ops")
    ref64, ref32 = C.yardstick(weights, window)
    frame = ops.fold_conditioning(_flat(weights), C.window_and_upstream(window)[0].to(DEV), _identity())
    e_hip, e_f32 = C.rel_max(frame[0:76], ref64["driving"]), C.rel_max(ref32["driving"], ref64["driving"])
    print("%s / %s: driving E_hip %.2e  E_f32 %.2e  scale %.3f" % (weights, window, e_hip, e_f32, float(ref64["driving"].abs().max())))
    assert bool(torch.isfinite(frame[0:76]).all()) and e_hip <= C.bound(e_f32), (e_hip, e_f32)


def test_driving_at_the_kink():
    """The exact-zero case: with no bias anywhere, the driving vector is exactly 0."""
    frame = pkg("ops").fold_conditioning(_flat(C.EXACT_ZERO[0], True), torch.zeros(16, 29, device=DEV), _identity())
    assert float(frame[0:76].abs().max()) == 0.0


@pytest.mark.parametrize("arch", ARCHS[1:])
def test_expression_is_the_driving_vector(arch):
    """NeRFaceModels: frame[0:76] is the expression vector bit for bit."""
    ops = pkg("ops")
    for window in ("seed0", "seed2"):
        expr = C.window_and_upstream(window)[1].to(DEV)
        frame = ops.fold_conditioning(_flat_of(arch), expr, _identity(), arch=arch)
        assert torch.equal(frame[0:76], expr), (arch, window)


@pytest.mark.parametrize("name", list(C.poses()))
@pytest.mark.parametrize("arch", ARCHS)
def test_pose36_vs_float64(arch, name):
    """frame[80:116] against the float64 pose encoding of the same float32 matrix: finite, and within max(4 x the float32 CPU
    evaluation's error on that pose, 1e-6)."""
    ops = pkg("ops")
    pose = C.poses()[name]
    e64, e32 = C.pose36(pose), C.pose36(pose, torch.float32)
    a, g = C.window_and_upstream("seed0")
    frame = ops.fold_conditioning(_flat_of(arch), (a if arch == "audio" else g).to(DEV), pose.to(DEV), arch=arch)
    got = frame[80:116].cpu()
    err, err32 = float((got.double() - e64).abs().max()), float((e32.double() - e64).abs().max())
    print("%s %s: |pose36 - f64| hip %.2e  float32 CPU %.2e  (worst entry %d)" % (arch, name, err, err32, int((got.double() - e64).abs().argmax())))
    assert bool(torch.isfinite(got).all())
    assert err <= max(4.0 * err32, POSE_FLOOR), (err, err32)


def _fold_direct(arch, flat, driving, pose_buf, pose_ld, fill):
    """sahs_model_fold_conditioning on a frame between sentinel guards -> (frame view, guards intact); the frame is prefilled with
    ``fill`` (the kernel leaves the padding words of the layout alone)."""
    ops, lib = pkg("ops"), pkg("_lib")
    words = int(lib.lib().sahs_model_frame_words(ops.ARCHS.index(arch)))
    whole, frame = _guarded(words, lambda n: torch.full((n,), fill, device=DEV))
    before = whole.clone()
    assert frame.data_ptr() % 16 == 0 and pose_buf.is_contiguous() and pose_buf.shape[0] >= 3 and pose_buf.shape[1] == pose_ld
    lib.check(lib.lib().sahs_model_fold_conditioning(ops.ARCHS.index(arch), ops._p(flat), ops._p(driving), ops._p(pose_buf), int(pose_ld),
                                                     ops._p(frame), ops._stream()), "sahs_model_fold_conditioning")
    torch.cuda.synchronize()
    return frame, _guards_intact(whole, before)


@pytest.mark.parametrize("arch", ARCHS)
def test_pose_shape_and_stride(arch):
    """A (4, 4) pose is its top (3, 4); a row stride of 7 with NaN in the other columns gives the whole frame, folded biases included,
    bit for bit; two calls give the same bits; nothing is written outside the frame."""
    ops = pkg("ops")
    flat = _flat_of(arch)
    a, g = C.window_and_upstream("seed3")
    driving = (a if arch == "audio" else g).to(DEV)
    p44 = C.poses()["euler1_4x4"].to(DEV)
    p34 = p44[:3].contiguous()
    fill = 12345.0
    ld4, ok4 = _fold_direct(arch, flat, driving, p34, 4, fill)
    wide = torch.full((3, 7), float("nan"), device=DEV)
    wide[:, :4] = p34
    ld7, ok7 = _fold_direct(arch, flat, driving, wide, 7, fill)
    rep, ok_rep = _fold_direct(arch, flat, driving, p34, 4, fill)
    sq, ok_sq = _fold_direct(arch, flat, driving, p44, 4, fill)
    written = ld4 != fill
    print("%s: frame of %d words, %d written (the rest is the layout's padding)" % (arch, ld4.numel(), int(written.sum())))
    assert ok4 and ok7 and ok_rep and ok_sq
    assert bool(written[0:76].all()) and bool(written[80:116].all()) and not bool(written[76:80].any()) and not bool(written[116:128].any())
    assert bool(written[128:].any())
    assert bool(torch.isfinite(ld4).all()) and bool(torch.isfinite(ld7).all())
    assert torch.equal(ld7, ld4) and torch.equal(rep, ld4) and torch.equal(sq, ld4)
    # and through ops.fold_conditioning, which accepts (3|4, 4): the same bits in every word the kernel writes
    f34, f44 = ops.fold_conditioning(flat, driving, p34, arch=arch), ops.fold_conditioning(flat, driving, p44, arch=arch)
    assert torch.equal(f34[written], ld4[written]) and torch.equal(f44[written], ld4[written])

