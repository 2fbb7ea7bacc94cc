"""Shared references for the bf16 form of the fused SPADE modulation (tests/test_spade_bf16_host.py, tests/test_gpu_spade_bf16.py).

* ``op_case_bf16``: the op-level inputs, drawn directly in bfloat16 -- the yardstick and the kernels then read the SAME values, and what
  is compared is the kernels' arithmetic and their one rounding, not a rounding of the inputs;
* ``reference``: the forward and ``spade_reference.analytic_backward`` in float64 on those values;
* ``figures`` / ``assert_rule``: the accuracy rule of a bf16 result against that yardstick (below);
* ``analytic``: the same formulas in a chosen dtype (float32: what shows that the reference alone stays within the rule's caps).

The rule, for a bf16 tensor ``got`` and its float64 yardstick ``ref`` (n elements):
  (a) every element of ``got`` is bfloat16(ref) or one of its two bf16 neighbours (one ulp);
  (b) at most ceil(1e-3 * n) elements differ from bfloat16(ref) at all: a different summation order changes an fp32 result by a few
      1e-7, which crosses a bf16 rounding boundary for about that share of elements divided by 2^-8; the float32 analytic result on the
      CPU differs in at most 8.5e-5 of the elements (many_planes dx) and the cap is some ten times that;
  (c) E = max |got - ref| / max |ref| <= 2^-8 + 4 * max(E32, 2^-21): one round-to-nearest at 8 significand bits, plus the project's rule
      (tests/test_gpu_spade_backward.py) for the same terms added in another order, E32 being the same quantity for an fp32 evaluation
      of the same values.
"""
import functools
import math

import torch

import spade_reference as R

EPS = R.EPS
SLOPES = R.SLOPES
FLOOR = 2.0 ** -21
NAMES = ("out", "dx", "dgamma", "dbeta")
MARGIN, NUDGE = 0.04, 0.0625      # the kink margin, and the step that restores it: 2^-4, exact in bf16
# name -> shape.  The smallest shapes at which each path of the bf16 kernels can go wrong:
OP_CASES = {"ragged": (3, 5, 7, 9),             # scalar path, odd hw: planes start at odd 2-byte offsets; plane [1, 2] is constant with beta 0
            "one_element": (1, 1, 1, 1),
            "hw4": (1, 2, 2, 2),                # a multiple of 4 but not of 8: the scalar path
            "one_vector": (1, 2, 2, 4),         # hw = 8: one 16-byte vector, seven empty chunks
            "partial_trip": (1, 2, 136, 128),   # 2176 vectors, a chunk of 272: the second 256-thread trip is partial
            "many_planes": (64, 160, 2, 4),     # 10240 planes: the apply pass's workgroup cap is 1 and it strides
            "unaligned2": (2, 4, 8, 8),         # the tensors start one bf16 element into their buffers: scalar path
            "unaligned8": (2, 4, 8, 8)}         # ... four elements (8 bytes) in: hw % 8 == 0, not 16-byte aligned: scalar path
OFFSET = {"unaligned2": 1, "unaligned8": 4}     # elements between the buffer's start and the tensor's
# Rule (a) is per element, and an element of dx that cancels to ~1e-5 of its plane's scale carries an fp32 summation error of several of
# its OWN bf16 ulps however the sum is ordered (seed 2001 of many_planes has one: 14 ulps in the float32 reference itself).  The draws are
# therefore ones on which the float32 analytic result meets the rule under four summation orders (torch's, sequential, reversed, and
# eight-wide partial sums): 2000 + the case's index, plus 100 until that holds -- a property of the inputs, found without the kernels.
SEEDS = {"hw4": 2000, "many_planes": 2301, "one_element": 2002, "one_vector": 2003, "partial_trip": 2104, "ragged": 2005,
         "unaligned2": 2006, "unaligned8": 2007}


def _forward64(x, gamma, beta):
    """The pre-activation y in float64 on the given values (torch_modulate with slope 1)."""
    return R.torch_modulate(x.double(), gamma.double(), beta.double(), slope=1.0)


def op_case_bf16(name, slope):
    """bfloat16 CPU tensors x, gamma, beta, g of OP_CASES[name], the same for every caller (and every slope: y does not depend on it).
    beta is nudged by +-0.0625 and re-rounded until |y| >= 0.04 wherever y is not exactly 0: no comparison then hinges on which side of
    the kink a value fell (one round suffices for every case here)."""
    assert slope in SLOPES
    return _op_case(name)


@functools.lru_cache(maxsize=None)
def _op_case(name):
    shape = OP_CASES[name]
    gen = torch.Generator().manual_seed(SEEDS[name])
    x = (torch.randn(shape, generator=gen) * 3 + 1).bfloat16()
    gamma, beta, g = (torch.randn(shape, generator=gen).bfloat16() for _ in range(3))
    if name == "ragged":
        x[1, 2], beta[1, 2] = 0.25, 0.0
    for _ in range(4):
        y = _forward64(x, gamma, beta)
        near = (y != 0) & (y.abs() < MARGIN)
        if not bool(near.any()):
            break
        beta = torch.where(near, (beta.double() + torch.sign(y) * NUDGE).bfloat16(), beta)
    return x, gamma, beta, g


def analytic(x, gamma, beta, g, slope, dtype):
    """out, dx, dgamma, dbeta by the formulas of the fused kernels, evaluated in ``dtype`` on the CPU; the mask from the output."""
    x, gamma, beta, g = (t.detach().cpu().to(dtype) for t in (x, gamma, beta, g))
    hw = x.shape[2] * x.shape[3]
    mean = x.sum((2, 3), keepdim=True) / hw
    r = 1.0 / torch.sqrt(((x - mean) ** 2).sum((2, 3), keepdim=True) / hw + EPS)
    xh = (x - mean) * r
    y = xh * (1 + gamma) + beta
    out = torch.where(y > 0, y, slope * y)
    dy = g * torch.where(out > 0, torch.ones_like(g), torch.full_like(g, slope))
    dxh = dy * (1 + gamma)
    dx = r * (dxh - dxh.sum((2, 3), keepdim=True) / hw - xh * ((dxh * xh).sum((2, 3), keepdim=True) / hw))
    return out, dx, dy * xh, dy


@functools.lru_cache(maxsize=None)
def reference(name, slope):
    """The float64 yardstick on the bf16 values -> (out, dx, dgamma, dbeta); computed once, never modified."""
    x, gamma, beta, g = op_case_bf16(name, slope)
    y = _forward64(x, gamma, beta)
    out = torch.where(y > 0, y, slope * y)
    return (out,) + tuple(R.analytic_backward(x, gamma, beta, g, slope=slope))


def _ordered(t):
    """bf16 -> integers in which neighbouring values differ by 1 (and -0 is 0)."""
    bits = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(bits < 0, -(bits & 0x7FFF), bits)


def figures(got, ref):
    """got: a bfloat16 tensor, ref: float64 -> (largest distance from bfloat16(ref) in ulps, elements that differ from it, E)."""
    got = got.detach().cpu()
    assert got.dtype == torch.bfloat16 and ref.dtype == torch.float64 and got.shape == ref.shape
    d = (_ordered(got) - _ordered(ref.to(torch.bfloat16))).abs()
    return int(d.max()), int((d != 0).sum()), R.rel_max(got, ref)


def rule(got, ref, e32):
    """-> (ok, text): the three parts of the rule and their figures."""
    ulps, differ, e = figures(got, ref)
    cap, bound = math.ceil(1e-3 * ref.numel()), 2.0 ** -8 + 4.0 * max(e32, FLOOR)
    text = "ulp %d differ %d/%d (cap %d) E %.2e (E32 %.1e, bound %.2e)" % (ulps, differ, ref.numel(), cap, e, e32, bound)
    return ulps <= 1 and differ <= cap and e <= bound, text
