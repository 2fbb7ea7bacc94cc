"""Shared references for the frozen SPADE modulation and the frozen generator (tests/test_spade_frozen_host.py,
tests/test_gpu_spade_frozen.py):

* ``torch_modulate_frozen``: ``spade_reference.torch_modulate`` on the interpolated, broadcast operands -- what
  ``ops.spade_modulate_frozen`` computes, written with torch ops in the operands' own dtype;
* ``torch_spectral_normalize``: eval-mode ``ops.spectral_normalize`` in torch ops (sigma = u . (W v), no power iteration);
* ``swapped``: ``ops.spade_modulate`` and ``ops.spade_modulate_frozen`` (and the fused spectral norm's op) replaced by those, which makes
  the generators and their frozen form run on the CPU and in float64;
* seeded eval-mode generators and inputs, the same for every caller.
"""
import contextlib
import copy
import functools

import torch

import spade_reference as R
from conftest import pkg


def torch_modulate_frozen(x, gamma, beta, eps=R.EPS, slope=1.0, up=False):
    if up:
        x = torch.nn.functional.interpolate(x, scale_factor=2, mode="nearest")
    return R.torch_modulate(x, gamma.expand_as(x), beta.expand_as(x), eps=eps, slope=slope)


def torch_spectral_normalize(weights, us, vs, training, eps=1e-12):
    assert not training, "the frozen generator is built from eval-mode modules"
    return [W / torch.dot(u, torch.mv(W.reshape(W.shape[0], -1), v)) for W, u, v in zip(weights, us, vs)]


@contextlib.contextmanager
def swapped():
    ops = pkg("ops")
    saved = ops.spade_modulate, ops.spade_modulate_frozen, ops.spectral_normalize
    ops.spade_modulate, ops.spade_modulate_frozen, ops.spectral_normalize = R.torch_modulate, torch_modulate_frozen, torch_spectral_normalize
    try:
        yield
    finally:
        ops.spade_modulate, ops.spade_modulate_frozen, ops.spectral_normalize = saved


SIZES = {"generator": (32, 32),            # the smallest at which the deepest planes are still 4 x 4
         "generator_audio": (48, 80)}      # the training fixture's shape: map widths 10 and 20 do not divide 4096


@functools.lru_cache(maxsize=None)
def _seeded_eval(name):
    return R.seeded(name).eval()


IMAGE_SCALE = {"generator": 1.0 / 350, "generator_audio": 1.0 / 80}      # 1 / (4 standard deviations of the seeded generator's output)


def generator(name, image_range=False):
    """A fresh float32 eval-mode copy of the seeded generator (spade_reference.seeded: the fixture's initialisation).  image_range (the
    byte tests): its last convolution rescaled to y * IMAGE_SCALE + 0.5, which puts most of the untrained generator's output inside
    [0, 1] -- as it comes, 99.6 % of it is clipped to 0 or 255 and any two byte images agree."""
    G = copy.deepcopy(_seeded_eval(name))
    if image_range:
        with torch.no_grad():
            G.refine_network.layer8.weight.mul_(IMAGE_SCALE[name])
            G.refine_network.layer8.bias.mul_(IMAGE_SCALE[name]).add_(0.5)
    return G


@functools.lru_cache(maxsize=None)
def inputs(name, batch=3, seed=0):
    """-> float32 CPU tensors I_src (1, 3, H, W), I_raw (batch, 3, H, W) in [0, 1], windows (batch, 16, 29) or None; different frames
    and different audio windows per row."""
    h, w = SIZES[name]
    gen = torch.Generator().manual_seed(7000 + seed + sorted(SIZES).index(name))
    i_src, i_raw = torch.rand(1, 3, h, w, generator=gen), torch.rand(batch, 3, h, w, generator=gen)
    windows = torch.randn(batch, 16, 29, generator=gen) if name == "generator_audio" else None
    return i_src, i_raw, windows


def run(G, i_src, i_raw, windows):
    """G frame by frame (Generator_audio takes one window per call) -> (B, 3, H, W), under no_grad."""
    with torch.no_grad():
        rows = [G(i_src, i_raw[b:b + 1]) if windows is None else G(i_src, i_raw[b:b + 1], windows[b]) for b in range(i_raw.shape[0])]
    return torch.cat(rows)


@functools.lru_cache(maxsize=None)
def reference64(name, batch=3, seed=0):
    """The unfrozen generator in float64 on the CPU (swapped ops), row by row: the yardstick of both test files."""
    i_src, i_raw, windows = (None if t is None else t.double() for t in inputs(name, batch, seed))
    with swapped():
        return run(generator(name).double(), i_src, i_raw, windows)


BYTES_EQUAL_CAP = 0.99      # refine_frames in fp32 against the float64 bytes: at least this fraction of positions equal, none off by more than 1


def frames_u8(name, n=3, seed=99):
    """n (H, W, 3) uint8 CPU frames of the generator's size, the same for every caller."""
    gen = torch.Generator().manual_seed(seed)
    h, w = SIZES[name]
    return [torch.randint(0, 256, (h, w, 3), generator=gen, dtype=torch.uint8) for _ in range(n)]


def frames_input(frames, dtype=torch.float32):
    """The reference's generator input of uint8 frames: / 255 in float32, CHW, then widened to ``dtype``."""
    return torch.stack([f.cpu().to(torch.float32) / 255 for f in frames]).permute(0, 3, 1, 2).contiguous().to(dtype)


@functools.lru_cache(maxsize=None)
def frames_bytes64(name):
    """Bytes of the unfrozen float64 generator on frames_u8(name) -> (uint8 (B, H, W, 3), the float64 values x255 they truncate)."""
    i_src, _, windows = (None if t is None else t.double() for t in inputs(name))
    with swapped():
        y = run(generator(name, image_range=True).double(), i_src, frames_input(frames_u8(name), torch.float64), windows)
    return to_bytes(y), (y.clamp(0.0, 1.0) * 255).permute(0, 2, 3, 1)


def bytes_agreement(got, want):
    """-> (largest difference in levels, fraction of positions equal) of two uint8 byte stacks."""
    got, want = (torch.stack(list(t)).cpu().int() if not isinstance(t, torch.Tensor) else t.cpu().int() for t in (got, want))
    return int((got - want).abs().max()), float((got == want).double().mean())


def to_bytes(y):
    """The reference's output rule: clip, x255, truncate -> (B, H, W, 3) uint8."""
    return (y.clamp(0.0, 1.0) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
