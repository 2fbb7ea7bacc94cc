"""The float64 yardstick and the inputs of the conditioning tests (tests/test_conditioning_reference_host.py, tests/test_gpu_conditioning.py).

* ``reference``: AudioNet as oracle/torch_eager.py states it (``EagerField.audionet``) over the ``audNet_head.*`` tensors of a state dict, in
  a chosen dtype -> the driving vector, the five pre-activations (the four convolutions and ``encoder_fc1.0``; from a layer-by-layer
  restatement here whose result must equal ``EagerField``'s bit for bit) and, for an upstream ``g[76]``, the autograd gradients of the
  twelve parameter tensors and of the (16, 29) window.  ``mutant`` gives one of three deliberately wrong gradients instead.
* ``pose36``: ``EagerField.pose_encoding`` of a float32 pose in a chosen dtype.
* the weight sets, windows, upstreams and poses, the same for every caller.

A float64 gradient is a fair yardstick only while the fp32 kernel sits on the same side of every LeakyReLU(0.02) kink, so ``reference``
reports min |pre-activation| / max |pre-activation| per layer and the tests hold every case to ``KINK_LINE``.  The exception is the case
built to sit ON the kink: the all-zero window with the AudioNet biases zeroed, where every pre-activation is exactly 0 and the derivative
is the slope (``F.leaky_relu``'s convention, and ``dl02``'s in csrc/train_bwd.hip).
"""
import functools
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from conftest import pkg
from oracle.torch_eager import EagerField

PREFIX = "audNet_head."
CONVS = (0, 2, 4, 6)
PRE_NAMES = tuple("encoder_conv.%d" % i for i in CONVS) + ("encoder_fc1.0",)
KINK_LINE = 1e-4
FLOOR = 2.0 ** -21
MUTANTS = ("slope", "circular", "last_tap")

# name -> hash_state_dict arguments.  hash_state_dict's hdr scaling leaves audNet_head alone, so "hdr" and "default" hold the SAME AudioNet
# (they differ in the layers the folded biases are made of); "seed1" is there so that more than one AudioNet is exercised.
WEIGHT_SETS = OrderedDict([("hdr", dict(seed=0, density_bias=2.0, density_gain=30.0, hdr=True)), ("default", dict()), ("seed1", dict(seed=1))])
# name -> (seed, kind).  Two seeds are left out because their smallest pre-activation ratio on the seed-0 AudioNet is under the line: seed 1
# as a whole window (8.3e-5) and seed 5 as the "ends" window (6.2e-5); the next seed took their place.
WINDOWS = OrderedDict([("seed0", (0, "randn")), ("seed2", (2, "randn")), ("seed3", (3, "randn")),
                       ("zero", (4, "zero")),          # every tap of the first convolution reads 0: the biases alone drive the net
                       ("ends", (6, "ends"))])         # zero except time steps 0 and 15, the steps next to the padding
CASES = [(w, a) for w in WEIGHT_SETS for a in WINDOWS]
EXACT_ZERO = ("hdr", "zero")     # with zero_bias=True


def audio_keys():
    """The twelve AudioNet parameter tensors, in state_dict order."""
    return [k for k in pkg("weights").canonical_offsets("audio") if k.startswith(PREFIX)]


def audio_slots():
    """key -> (offset, shape) of the twelve tensors in the flat parameter vector."""
    return OrderedDict((k, v) for k, v in pkg("weights").canonical_offsets("audio").items() if k.startswith(PREFIX))


@functools.lru_cache(maxsize=None)
def state_dict(name, model="audio"):
    return pkg("weights").hash_state_dict(model=model, **WEIGHT_SETS[name])


@functools.lru_cache(maxsize=None)
def flat_weights(name, zero_bias=False, model="audio"):
    """The flat float32 parameter vector (numpy); zero_bias: with the six AudioNet biases zeroed."""
    flat = pkg("weights").flatten_state_dict(state_dict(name, model), model=model).copy()
    if zero_bias:
        for k, (o, shp) in audio_slots().items():
            if k.endswith(".bias"):
                flat[o:o + shp[0]] = 0.0
    flat.setflags(write=False)
    return flat


def audio_tensors(name, zero_bias=False, dtype=torch.float64):
    """The audNet_head.* tensors, cut out of the flat vector by canonical_offsets, as fresh torch tensors of ``dtype``."""
    flat = flat_weights(name, zero_bias)
    return OrderedDict((k, torch.from_numpy(flat[o:o + int(np.prod(shp))].reshape(shp).copy()).to(dtype)) for k, (o, shp) in audio_slots().items())


@functools.lru_cache(maxsize=None)
def window_and_upstream(name):
    """-> float32 CPU (16, 29) window and (76,) upstream gradient: randn(16, 29) then randn(76) from one seeded CPU generator."""
    seed, kind = WINDOWS[name]
    gen = torch.Generator().manual_seed(seed)
    a = torch.randn(16, 29, generator=gen)
    g = torch.randn(76, generator=gen)
    if kind == "zero":
        a = torch.zeros(16, 29)
    elif kind == "ends":
        a[1:15] = 0.0
    return a, g


def _leaky(x, slope, back_slope):
    """LeakyReLU(slope) whose derivative is that of LeakyReLU(back_slope): the value of one, the gradient of the other."""
    y = F.leaky_relu(x, slope)
    if back_slope == slope:
        return y
    z = F.leaky_relu(x, back_slope)
    return y.detach() + (z - z.detach())


def _layers(sd, audio, mutant=None):
    """modules.py:68-73 layer by layer -> (driving, [pre-activations]).  mutant: "slope" -- the backward takes slope 0.01 (the forward
    keeps 0.02); "circular" -- every convolution pads with the other end of its input instead of zeros; "last_tap" -- the last
    convolution alone does (its k = 0 tap reads t = 1 where the padding is)."""
    back = 0.01 if mutant == "slope" else 0.02
    pres = []
    x = audio.unsqueeze(0)[:, 0:16, :].permute(0, 2, 1)
    for i in CONVS:
        w, b = sd[PREFIX + "encoder_conv.%d.weight" % i], sd[PREFIX + "encoder_conv.%d.bias" % i]
        if mutant == "circular" or (mutant == "last_tap" and i == 6):
            pre = F.conv1d(F.pad(x, (1, 1), mode="circular"), w, b, stride=2)
        else:
            pre = F.conv1d(x, w, b, stride=2, padding=1)
        pres.append(pre)
        x = _leaky(pre, 0.02, back)
    x = x.squeeze(-1)
    pre = F.linear(x, sd[PREFIX + "encoder_fc1.0.weight"], sd[PREFIX + "encoder_fc1.0.bias"])
    pres.append(pre)
    x = _leaky(pre, 0.02, back)
    return F.linear(x, sd[PREFIX + "encoder_fc1.2.weight"], sd[PREFIX + "encoder_fc1.2.bias"]).squeeze(), pres


def moved_by(mutant, window, zero_bias=False):
    """The gradients a mutant must move.  A wrong backward slope reaches everything upstream of an activation (not encoder_fc1.2); wrong
    padding changes the forward too, so everything but encoder_fc1.2.bias (a copy of g).  Left out: the first convolution's weight under
    the all-zero window (its gradient is a product with the window), and in the exact-zero case every weight (products with activations
    that are all 0)."""
    keys = audio_keys() + ["audio"]
    keys = [k for k in keys if not k.endswith("encoder_fc1.2.bias") and not (mutant == "slope" and k.endswith("encoder_fc1.2.weight"))]
    if WINDOWS[window][1] == "zero":
        keys = [k for k in keys if not k.endswith("encoder_conv.0.weight")]
    if zero_bias:
        keys = [k for k in keys if not k.endswith(".weight")]
    return keys


def reference(weights, window, zero_bias=False, dtype=torch.float64, mutant=None):
    """window: a name of WINDOWS, or a pair of float32 tensors (window (16, 29), upstream (76,)).
    -> dict(driving (76,), pre {layer: tensor}, kink {layer: min |pre| / max |pre|, nan where the layer is all zero},
    grads {the twelve keys + "audio": tensor}) in ``dtype`` on the CPU."""
    a32, g32 = window_and_upstream(window) if isinstance(window, str) else window
    sd = audio_tensors(weights, zero_bias, dtype)
    for v in sd.values():
        v.requires_grad_(True)
    audio = a32.clone().to(dtype).requires_grad_(True)      # (a copy: the cached window itself must never become an autograd leaf)
    driving, pres = _layers(sd, audio, mutant)
    if mutant is None:
        eager = EagerField(sd).audionet(audio)
        assert torch.equal(eager, driving), "the layer-by-layer restatement left EagerField.audionet"
        driving = eager
    driving.backward(g32.to(dtype))
    grads = OrderedDict((k, v.grad.detach()) for k, v in sd.items())
    grads["audio"] = audio.grad.detach()
    pre = OrderedDict((n, p.detach().reshape(p.shape[1:]).squeeze(-1) if p.dim() == 3 else p.detach().reshape(-1)) for n, p in zip(PRE_NAMES, pres))
    kink = OrderedDict((n, float(p.abs().min()) / float(p.abs().max()) if float(p.abs().max()) > 0 else float("nan")) for n, p in pre.items())
    return dict(driving=driving.detach(), pre=pre, kink=kink, grads=grads)


@functools.lru_cache(maxsize=None)
def yardstick(weights, window, zero_bias=False):
    """reference(...) in float64 and in float32, computed once per session: -> (ref64, ref32).  Treat as read-only."""
    return reference(weights, window, zero_bias), reference(weights, window, zero_bias, dtype=torch.float32)


def rel_max(got, ref):
    """E = max |got - ref| / max |ref| (ref in float64), as spade_reference.rel_max; 0 / 0 = 0 and x / 0 = inf, so that a tensor float64 says
    is identically zero passes the rule only when it is exactly zero."""
    ref = ref.detach().double().cpu()
    err, scale = float((got.detach().double().cpu() - ref).abs().max()), float(ref.abs().max())
    if scale == 0.0:
        return 0.0 if err == 0.0 else float("inf")
    return err / scale


def bound(e_f32):
    """The rule: as close to float64 as float32 CPU autograd is, within the factor two correct fp32 summation orders are granted."""
    return max(4.0 * e_f32, FLOOR)


def short(key):
    return key[len(PREFIX):].replace("encoder_", "") if key.startswith(PREFIX) else key


# ---- poses ----
def _rot(axis, c, s):
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def _pose(R, t, rows=3):
    p = np.concatenate([np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3, 1)], 1)
    if rows == 4:
        p = np.concatenate([p, [[0.0, 0.0, 0.0, 1.0]]], 0)
    return torch.from_numpy(np.ascontiguousarray(p.astype(np.float32) + 0.0))      # (+ 0.0: no negative zeros from the products)


@functools.lru_cache(maxsize=None)
def poses():
    """name -> float32 CPU pose, (3, 4) but for the last.  The quarter turns hold exact 0 and +-1: exact zeros in the atan2 arguments, and
    about y R02 = +1 / -1 exactly, the two ends of asin's domain (both atan2 then read (0, 0) and (0, -0))."""
    out = OrderedDict()
    out["identity"] = _pose(np.eye(3), (0.0, 0.0, 0.8))
    rng = np.random.default_rng(7)
    for n in range(3):
        e = rng.uniform(-np.pi, np.pi, 3) * np.array([1.0, 0.49, 1.0])
        R = _rot(2, np.cos(e[2]), np.sin(e[2])) @ _rot(1, np.cos(e[1]), np.sin(e[1])) @ _rot(0, np.cos(e[0]), np.sin(e[0]))
        out["euler%d" % n] = _pose(R, rng.uniform(-1.0, 1.0, 3))
    out["quarter_x"] = _pose(_rot(0, 0.0, 1.0), (0.3, -0.2, 0.8))
    out["quarter_y"] = _pose(_rot(1, 0.0, 1.0), (-1.0, 0.5, 0.25))
    out["quarter_y_back"] = _pose(_rot(1, 0.0, -1.0), (0.0, 1.0, -0.5))
    out["quarter_z"] = _pose(_rot(2, 0.0, 1.0), (0.125, 0.0, 1.0))
    out["euler1_4x4"] = torch.cat([out["euler1"], torch.tensor([[0.0, 0.0, 0.0, 1.0]])], 0)
    return out


def pose36(pose, dtype=torch.float64):
    """EagerField.pose_encoding of the float32 pose, evaluated in ``dtype`` -> (36,)."""
    return EagerField.pose_encoding(pose.to(dtype)).reshape(-1)
