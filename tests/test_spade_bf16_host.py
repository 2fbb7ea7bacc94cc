"""The bf16 form of the fused SPADE modulation, the parts a CPU can check: that the op-level cases are a usable yardstick (every
pre-activation is 0 or at least 0.04 from the kink), that the accuracy rule of tests/spade_bf16_reference.py has caps the reference alone
stays within (the float32 analytic result, rounded once to bf16, meets it), that the header, the ctypes table and the built library agree
on the two new entry points and that these refuse before any launch, the dtype rule of ``ops.spade_modulate`` as far as it is decided
without a GPU, ``refine_step``'s new keyword, and ``TiledCodeMap.nearest`` on a bf16 code (what the Conv1d stack hands it under autocast).

Measured here over the 8 shapes x 3 slopes (float32 analytic, rounded to bf16, against the float64 yardstick): never more than one ulp
from bfloat16(ref); elements that differ from it at all: at most 7 of 81920 (8.5e-5: many_planes dx, slope 0; the cap is 1e-3 rounded up),
2 of 34816 (partial_trip dx) and 1 of 945 (ragged dx, slope 0.2: the cap); E at most 3.4e-3 against 2^-8 = 3.9e-3."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import spade_bf16_reference as B
import spade_reference as R
from conftest import REPO, pkg

NEW = ("sahs_spade_modulate_bf16", "sahs_spade_modulate_backward_bf16")


@pytest.mark.parametrize("case", sorted(B.OP_CASES))
def test_cases_keep_the_kink_margin(case):
    x, gamma, beta, g = B.op_case_bf16(case, 0.2)
    assert all(t.dtype == torch.bfloat16 and tuple(t.shape) == B.OP_CASES[case] for t in (x, gamma, beta, g))
    y = R.torch_modulate(x.double(), gamma.double(), beta.double(), slope=1.0)
    assert bool(((y == 0) | (y.abs() >= B.MARGIN)).all()), float(y[y != 0].abs().min())
    if case == "ragged":
        assert bool((y[1, 2] == 0).all()) and bool((y != 0).any())
    for slope in B.SLOPES:      # the same tensors for every slope
        assert all(a is b for a, b in zip(B.op_case_bf16(case, slope), (x, gamma, beta, g)))


@pytest.mark.parametrize("slope", B.SLOPES)
@pytest.mark.parametrize("case", sorted(B.OP_CASES))
def test_float32_reference_rounded_once_meets_the_rule(case, slope):
    """The rule's caps are ones the reference alone stays within; and ``analytic`` in float64 IS the yardstick."""
    inputs, ref = B.op_case_bf16(case, slope), B.reference(case, slope)
    for name, a, r in zip(B.NAMES, B.analytic(*inputs, slope, torch.float64), ref):
        assert R.rel_max(a, r) <= 1e-12, name
    for name, a, r in zip(B.NAMES, B.analytic(*inputs, slope, torch.float32), ref):
        ok, text = B.rule(a.bfloat16(), r, R.rel_max(a, r))
        print("%s slope %g %s: %s" % (case, slope, name, text))
        assert ok, (name, text)


def test_rule_notices_a_wrong_result():
    """One ulp everywhere, two ulps in one element, an error of 1e-2 of scale: each part of the rule fails on its own."""
    inputs, ref = B.op_case_bf16("partial_trip", 0.2), B.reference("partial_trip", 0.2)
    good = ref[1].to(torch.bfloat16)
    assert B.figures(good, ref[1])[:2] == (0, 0) and B.rule(good, ref[1], 0.0)[0]
    up = lambda t, k: (t.view(torch.int16) + k).view(torch.bfloat16)
    assert B.figures(up(good, 1), ref[1])[0] == 1 and not B.rule(up(good, 1), ref[1], 0.0)[0]      # (b): every element differs
    two = good.clone()
    two.view(-1)[:1] = up(two.view(-1)[:1].clone(), 2)
    assert B.figures(two, ref[1])[:2] == (2, 1) and not B.rule(two, ref[1], 0.0)[0]                  # (a)
    x, gamma, beta, g = inputs
    shifted = B.analytic(x, gamma, beta, g, 0.2, torch.float64)[1] + 1e-2 * float(ref[1].abs().max())
    assert B.figures(shifted.bfloat16(), ref[1])[2] > 2.0 ** -8 and not B.rule(shifted.bfloat16(), ref[1], 0.0)[0]      # (c)


def test_header_ctypes_table_and_library_agree_on_the_bf16_entries():
    """Fails without the feature on a machine with no GPU."""
    lib = pkg("_lib")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "sahs_nerf.h")).read(), flags=re.S)
    so = ctypes.CDLL(lib.LIB_PATH)
    for new in NEW:
        old = new[:-len("_bf16")]
        decl = {n: re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % n, text) for n in (new, old)}
        assert decl[new] is not None, "include/sahs_nerf.h does not declare %s" % new
        assert new in lib.SIGNATURES and hasattr(so, new)
        # the fp32 entry's argument list with the tensor pointers as unsigned short *; stats and work stay float *
        args = lambda m: [" ".join(a.split()) for a in m.group(1).split(",")]
        want = [a if re.search(r"\b(stats|work)$", a) else a.replace("float *", "unsigned short *") for a in args(decl[old])]
        assert args(decl[new]) == want
        assert lib.SIGNATURES[new] == lib.SIGNATURES[old]


def test_bf16_entries_refuse_before_any_launch():
    """Every call here is answered by argument validation (fabricated addresses, never dereferenced) -- with or without a GPU."""
    L = pkg("_lib").lib()
    A = 1 << 20
    fwd = lambda planes=6, hw=16, x=A, out=A, stats=A, eps=1e-5: L.sahs_spade_modulate_bf16(planes, hw, x, A, A, eps, 0.2, out, stats, None)
    bwd = lambda planes=6, hw=16, out=A, slope=0.2, dx=A, dgamma=A, dbeta=A, work=A, eps=1e-5: L.sahs_spade_modulate_backward_bf16(
        planes, hw, A, A, out, A, A, eps, slope, dx, dgamma, dbeta, work, None)
    for call, name in ((fwd, b"sahs_spade_modulate_bf16"), (bwd, b"sahs_spade_modulate_backward_bf16")):
        assert call(planes=0) == 0 and call(hw=0) == 0                      # nothing to do: success without a launch
        assert call(planes=65536) == 1                                      # gridDim.y: refused by name, not an opaque HIP error
        assert b"65535" in L.sahs_last_error() and name in L.sahs_last_error()
        assert call(planes=-1) == 1 and call(hw=-1) == 1 and call(eps=0.0) == 1
    assert fwd(x=None) == 1 and fwd(out=None) == 1 and fwd(stats=None) == 1
    assert bwd(out=None) == 1                                               # the mask is read from out unless slope == 1
    assert bwd(slope=-0.1) == 1 and bwd(slope=float("nan")) == 1
    assert bwd(dx=None, dgamma=None, dbeta=None) == 1
    assert bwd(work=None) == 1                                              # dx needs the workspace


def test_dtype_rule_without_a_gpu():
    """Unsupported dtypes are refused by name before anything else is looked at; supported ones still have no CPU path."""
    ops, lib = pkg("ops"), pkg("_lib")
    z = torch.zeros(1, 2, 2, 2)
    for bad in (torch.float16, torch.float64):
        with pytest.raises(lib.SahsError, match=r"torch\.float32 or torch\.bfloat16"):
            ops.spade_modulate(z.to(bad), z.to(bad), z.to(bad))
        with pytest.raises(lib.SahsError, match=r"torch\.float32 or torch\.bfloat16"):
            ops.spade_modulate(z.bfloat16(), z.to(bad), z)
    for x, gamma in ((z.bfloat16(), z.bfloat16()), (z.bfloat16(), z)):
        with pytest.raises(lib.SahsError, match="GPU tensor"):
            ops.spade_modulate(x, gamma, z.to(gamma.dtype))


def test_refine_step_keyword():
    S = pkg("spade")
    p = inspect.signature(S.refine_step).parameters
    assert list(p)[-1] == "autocast_dtype" and p["autocast_dtype"].default is None
    with pytest.raises(ValueError, match="bfloat16"):
        S.refine_step(None, None, None, None, None, autocast_dtype=torch.float16)


def test_tiled_code_map_nearest_on_a_bf16_code():
    """Under autocast the Conv1d stack hands TiledCodeMap a bf16 code: ``nearest`` is an index and a copy, so it stays exact in any dtype."""
    S = pkg("spade")
    code = (torch.arange(64, dtype=torch.float32) * 0.37 - 7.0).bfloat16()
    m = S.TiledCodeMap(code, channels=2, height=64, tiles=64)
    big = m.materialise()
    for size in ((6, 10), (12, 20), (64, 64), (7, 97)):
        got = m.nearest(size)
        assert got.dtype == torch.bfloat16 and got.is_contiguous()
        assert torch.equal(got.float(), torch.nn.functional.interpolate(big.float(), size=size, mode="nearest")), size
