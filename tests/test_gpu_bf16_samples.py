"""The plain-bf16 field kernel (field_forward_bf16w_kernel, SAHS_BF16) held to float64, sample by sample.

Every plain-bf16 evaluation that exists, both levels, both LeakyReLU forms (ops.bf16_exact_leaky):
  audio           the whole kernel, ops.field_forward(..., debug=True): raw and the debug taps dx, w
  nerface         ops.field_forward_split(FIELD_RADIANCE) at SAHS_BF16 on the xw of the fp32 FIELD_DEFORM launch, through a per-ray
                  permutation src (xw rows wider than S, a column offset)
  nerface_static  ops.field_forward (the whole network is the radiance net)

EXPECTED VALUE: oracle/torch_eager.py::EagerField in float64.  MEASURE: tests/bf16_reference.py::Bf16Field, the same network with the
kernel's documented rounding points, exactly as the reference's fp32 run is the measure of the fp32 kernels.  RULE: conftest.yardstick
with its defaults, got = HIP, ref32 = emulation, ref64 = float64: max |HIP - f64| <= 3 x max |emulation - f64|, rms <= 2 x, plus 32 fp32
ulps of the tensor's scale.

Two seams, so that the 2^9 / 2^14 amplification of x' round-off in the encodings never enters a per-sample comparison:
  deformation seam (audio)  the kernel's dx, w against EagerField's float64 taps at the same points; measure: the emulation's dx, w.
  radiance seam (all three) the kernel's raw against float64 EagerField(given=...) AT THE KERNEL'S OWN x', w (audio: x + dx and w of the
                            taps; nerface: the xw rows fed in; nerface_static: x); sigma, rgb logits, seg logits are separate tensors;
                            measure: the emulation at the same x', w.
x' rebuilt as x + dx from the tap (and x rebuilt as o + d z in torch where the kernel uses a fused multiply-add) differs from the kernel's
register value by at most an fp32 ulp, 6e-8 here: amplified by 2^9 that is 3e-5 in an encoding argument, a hundredth of the bf16 step
(2^-9 relative) that every encoding is rounded with next.

Sizes N x S (256-sample tiles, four 64-sample waves, 32-sample halves): 1 x 1, 1 x 33 (one past a half), 11 x 7 = 77 (a whole wave and
13 samples), 4 x 64 = 256 (one tile), 257 x 1 (one sample in a second tile), 65 x 13 = 845 (MAIN: three tiles and a ragged 77).  The
main case carries the statistics and is also held over its edge rows alone (the last 64 samples, the first and last sample of every
32-sample half of the last tile, the first row of every tile: 68 rows).  Sizes below 256 samples have too few values for a maximum of their
own: they are held to the main case's emulation errors with the same factors (bf16_reference.hold_to).  Outputs are the leading slice of
a NaN-filled buffer whose guard rows must stay untouched.

Negative controls on the main case's HIP output, values only: (a) row P-1 exchanged with a row of another ray, (b) row P-1 copied over
row P-257, (c) 6 x the emulation's max error added to one colour logit of row P-1 (away from float64).  Each must fail the rule in the
tensor group named; for (a), (b) the partner's float64 row differs from row P-1's by more than 10 x the emulation's max error in a column
of that group (a condition on the inputs, proven for the seeded scenes on the host: tests/test_bf16_reference_host.py).

Observed on a 256-CU MI355X, main case (845 samples; 68 edge rows): max |HIP - f64| / max |emulation - f64| and the ratio of the two rms
errors, over the whole launch and over the edge rows.  The rule allows 3 (max) and 2 (rms); every negative control failed it.  The kernel
and the emulation agree this closely because they make the same roundings sample by sample (the test prints max |HIP - emulation| beside
each line, not asserted: the kernel sums in fp32 inside the MFMA in an order of its own, so a pre-activation near a bf16 tie may round
the other way).
  model          L form     tensor  max |HIP-f64| / max |emu-f64| = ratio   rms ratio   edge rows: max ratio   rms ratio
  audio          0 pattern  sigma   3.81e-01 / 3.81e-01 = 1.00           0.99        3.67e-01 / 3.67e-01 = 1.00  0.98
  audio          0 pattern  rgb     6.99e-02 / 6.99e-02 = 1.00           1.00        6.27e-02 / 6.27e-02 = 1.00  1.01
  audio          0 pattern  seg     8.15e-02 / 8.15e-02 = 1.00           1.00        7.92e-02 / 7.92e-02 = 1.00  1.00
  audio          0 pattern  dx      2.46e-04 / 2.46e-04 = 1.00           1.00        1.89e-04 / 1.89e-04 = 1.00  1.00
  audio          0 pattern  w       4.38e-03 / 4.38e-03 = 1.00           1.00        3.36e-03 / 3.36e-03 = 1.00  1.00
  audio          0 exact    sigma   3.90e-01 / 3.90e-01 = 1.00           0.99        2.98e-01 / 2.98e-01 = 1.00  1.01
  audio          0 exact    rgb     6.23e-02 / 6.23e-02 = 1.00           0.99        5.13e-02 / 5.13e-02 = 1.00  0.99
  audio          0 exact    seg     9.48e-02 / 9.48e-02 = 1.00           1.00        6.61e-02 / 6.61e-02 = 1.00  0.99
  audio          0 exact    dx      2.46e-04 / 2.46e-04 = 1.00           1.00        1.89e-04 / 1.89e-04 = 1.00  1.00
  audio          0 exact    w       4.38e-03 / 4.38e-03 = 1.00           1.00        3.36e-03 / 3.36e-03 = 1.00  1.00
  audio          1 pattern  sigma   4.23e-01 / 4.23e-01 = 1.00           1.00        3.03e-01 / 3.20e-01 = 0.95  0.99
  audio          1 pattern  rgb     7.53e-02 / 7.53e-02 = 1.00           1.00        4.43e-02 / 4.43e-02 = 1.00  1.01
  audio          1 pattern  seg     6.50e-02 / 6.50e-02 = 1.00           1.00        5.74e-02 / 5.74e-02 = 1.00  1.01
  audio          1 pattern  dx      2.46e-04 / 2.46e-04 = 1.00           1.00        1.89e-04 / 1.89e-04 = 1.00  1.00
  audio          1 pattern  w       4.38e-03 / 4.38e-03 = 1.00           1.00        3.36e-03 / 3.36e-03 = 1.00  1.00
  audio          1 exact    sigma   4.16e-01 / 4.16e-01 = 1.00           0.99        2.97e-01 / 2.97e-01 = 1.00  1.00
  audio          1 exact    rgb     5.91e-02 / 5.91e-02 = 1.00           1.01        5.50e-02 / 5.50e-02 = 1.00  1.00
  audio          1 exact    seg     6.62e-02 / 6.62e-02 = 1.00           1.00        5.94e-02 / 5.94e-02 = 1.00  1.00
  audio          1 exact    dx      2.46e-04 / 2.46e-04 = 1.00           1.00        1.89e-04 / 1.89e-04 = 1.00  1.00
  audio          1 exact    w       4.38e-03 / 4.38e-03 = 1.00           1.00        3.36e-03 / 3.36e-03 = 1.00  1.00
  nerface        0 pattern  sigma   2.02e-02 / 2.02e-02 = 1.00           1.00        1.75e-02 / 1.75e-02 = 1.00  1.00
  nerface        0 pattern  rgb     1.76e-04 / 1.76e-04 = 1.00           1.00        1.48e-04 / 1.48e-04 = 1.00  1.00
  nerface        0 pattern  seg     2.28e-04 / 2.28e-04 = 1.00           1.00        1.67e-04 / 1.67e-04 = 1.00  1.00
  nerface        0 exact    sigma   2.18e-02 / 2.18e-02 = 1.00           1.00        2.07e-02 / 2.07e-02 = 1.00  1.00
  nerface        0 exact    rgb     1.80e-04 / 1.80e-04 = 1.00           1.00        1.43e-04 / 1.43e-04 = 1.00  1.00
  nerface        0 exact    seg     2.16e-04 / 2.16e-04 = 1.00           1.00        1.72e-04 / 1.72e-04 = 1.00  1.00
  nerface        1 pattern  sigma   1.85e-02 / 1.85e-02 = 1.00           1.00        1.68e-02 / 1.68e-02 = 1.00  1.00
  nerface        1 pattern  rgb     1.65e-04 / 1.65e-04 = 1.00           1.00        1.65e-04 / 1.65e-04 = 1.00  1.01
  nerface        1 pattern  seg     2.53e-04 / 2.53e-04 = 1.00           1.00        1.78e-04 / 1.78e-04 = 1.00  1.00
  nerface        1 exact    sigma   1.79e-02 / 1.79e-02 = 1.00           1.00        1.45e-02 / 1.45e-02 = 1.00  1.00
  nerface        1 exact    rgb     1.53e-04 / 1.53e-04 = 1.00           1.00        1.53e-04 / 1.53e-04 = 1.00  1.00
  nerface        1 exact    seg     2.78e-04 / 2.78e-04 = 1.00           1.00        1.99e-04 / 1.99e-04 = 1.00  1.00
  nerface_static 0 pattern  sigma   1.57e-02 / 1.57e-02 = 1.00           1.00        1.29e-02 / 1.29e-02 = 1.00  0.99
  nerface_static 0 pattern  rgb     2.07e-04 / 2.07e-04 = 1.00           1.00        1.75e-04 / 1.75e-04 = 1.00  0.99
  nerface_static 0 pattern  seg     2.17e-04 / 2.17e-04 = 1.00           1.00        1.78e-04 / 1.78e-04 = 1.00  1.00
  nerface_static 0 exact    sigma   1.61e-02 / 1.61e-02 = 1.00           1.00        1.44e-02 / 1.44e-02 = 1.00  1.00
  nerface_static 0 exact    rgb     2.02e-04 / 1.96e-04 = 1.03           1.00        1.61e-04 / 1.61e-04 = 1.00  1.00
  nerface_static 0 exact    seg     1.95e-04 / 1.95e-04 = 1.00           1.00        1.51e-04 / 1.51e-04 = 1.00  1.00
  nerface_static 1 pattern  sigma   1.64e-02 / 1.64e-02 = 1.00           1.00        1.24e-02 / 1.24e-02 = 1.00  1.00
  nerface_static 1 pattern  rgb     1.75e-04 / 1.75e-04 = 1.00           1.00        1.38e-04 / 1.38e-04 = 1.00  1.00
  nerface_static 1 pattern  seg     2.87e-04 / 2.87e-04 = 1.00           1.00        2.36e-04 / 2.36e-04 = 1.00  1.00
  nerface_static 1 exact    sigma   1.61e-02 / 1.61e-02 = 1.00           1.00        1.13e-02 / 1.13e-02 = 1.00  1.00
  nerface_static 1 exact    rgb     1.74e-04 / 1.74e-04 = 1.00           1.00        1.43e-04 / 1.43e-04 = 1.00  1.00
  nerface_static 1 exact    seg     2.67e-04 / 2.67e-04 = 1.00           1.00        2.41e-04 / 2.41e-04 = 1.00  1.00
Other sizes, all three models, both levels and forms: 4 x 64 and 257 x 1 against their own emulation: max ratio 0.93 .. 1.07, rms ratio
0.99 .. 1.02 (88 tensors); 1 x 1, 1 x 33, 11 x 7 against the main case's emulation errors: max ratio <= 1.04, rms ratio <= 1.84 (132 tensors;
the largest is the single sigma value of nerface_static 1 x 1, level 1, exact form: one sample's error against the rms of 845).
"""
import pytest
import torch

import bf16_reference as BR
import field_reference as FR
from conftest import pkg

pytestmark = pytest.mark.gpu

_CACHE = {}
GUARD_ROWS = 512
XW_PAD, XW_COL0 = 5, 3
ARCHS = ("audio", "nerface", "nerface_static")
FORM = {False: "pattern", True: "exact"}


def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def nan(*shape):
    return torch.full(shape, float("nan"), device=dev())


def model(arch):
    if ("model", arch) not in _CACHE:
        ops, W = pkg("ops"), pkg("weights")
        sd_np = FR.state_dict_np(W, arch)
        flat = torch.from_numpy(W.flatten_state_dict(sd_np, model=arch)).to(dev())
        frame = ops.fold_conditioning(flat, FR.driving_input(arch, dev()), FR.pose_of(arch, dev()), arch=arch)
        packs = dict(bf16=ops.pack_weights(flat, ops.SAHS_BF16, arch=arch))
        if arch == "nerface":
            packs["fp32"] = ops.pack_weights(flat, ops.SAHS_F32, arch=arch)
        _CACHE[("model", arch)] = dict(sd=BR.tensors(sd_np, dev()), frame=frame, packs=packs, drv=frame[0:76].clone(), p36=frame[80:116].clone())
    return _CACHE[("model", arch)]


def launch(arch, level, exact, N, S):
    """One evaluation -> dict: raw (P, 16), the seam it was evaluated at (xp (P, 3), w (P, AMB) or None), x6, and the taps dx, w (audio)"""
    ops, m = pkg("ops"), model(arch)
    rays, z, x6 = FR.build_scene(arch, N, S, dev())
    P = N * S
    buf = nan((P + GUARD_ROWS) * 16)
    out = buf[:P * 16].view(N, S, 16)
    what = "%s %dx%d L%d %s" % (arch, N, S, level, FORM[exact])
    res = dict(x6=x6, what=what)
    assert ops.bf16_exact_leaky() is False
    try:
        assert ops.bf16_exact_leaky(exact) is exact
        if arch == "audio":
            _, dx, w, _ = ops.field_forward(m["packs"]["bf16"], m["frame"], level, rays, z, precision=ops.SAHS_BF16, debug=True, out=out, arch=arch)
            res.update(dx=dx.reshape(P, 3), tap_w=w.reshape(P, 2), xp=x6[:, :3] + dx.reshape(P, 3), w=w.reshape(P, 2))
        elif arch == "nerface":
            xw = nan(N, S + XW_PAD, 8)
            ops.field_forward_split(m["packs"]["fp32"], m["frame"], level, ops.FIELD_DEFORM, rays, xw, z=z, xw_col0=XW_COL0, arch=arch,
                                    precision=ops.SAHS_F32)
            src = (FR.ray_permutation(N, S, dev()) + XW_COL0).contiguous()
            ops.field_forward_split(m["packs"]["bf16"], m["frame"], level, ops.FIELD_RADIANCE, rays, xw, src=src, out=out, arch=arch,
                                    precision=ops.SAHS_BF16, validate_src=True)
            fed = torch.gather(xw, 1, src.long()[..., None].expand(N, S, 8)).reshape(P, 8)
            assert bool(torch.isfinite(fed[:, :5]).all()), what + ": the deformation launch left x', w unwritten"
            res.update(xp=fed[:, 0:3], w=fed[:, 3:4])
        else:
            ops.field_forward(m["packs"]["bf16"], m["frame"], level, rays, z, precision=ops.SAHS_BF16, out=out, arch=arch)
            res.update(xp=x6[:, :3], w=None)
        torch.cuda.synchronize()
    finally:
        ops.bf16_exact_leaky(False)
    assert bool(torch.isfinite(buf[:P * 16]).all()), what + ": raw[:P] is not finite (a row was never written)"
    assert FR.same_bits(buf[P * 16:], nan(GUARD_ROWS * 16)), what + ": rows behind P were written"
    res["raw"] = out.reshape(P, 16).clone()
    return res


def references(arch, level, exact, hip):
    """float64 and the emulation for one launch -> {tensor name: (HIP, emulation, float64)}: sigma, rgb, seg at the kernel's own seam, and
    for the AudioFaceModel dx, w at the launch's points"""
    m = model(arch)
    args = (m["sd"], arch, level, hip["x6"], m["drv"], m["p36"])
    given = (hip["xp"], hip["w"])
    r64 = BR.evaluate(*args, rounding=False, given=given)["raw"]
    emu = BR.evaluate(*args, rounding=True, exact_leaky=exact, given=given)["raw"]
    out = {name: (g, e, r) for (name, g), (_, e), (_, r) in zip(BR.groups(hip["raw"]), BR.groups(emu), BR.groups(r64))}
    out["_raw"] = (hip["raw"], emu, r64)
    if arch == "audio":
        d64, demu = BR.evaluate(*args, rounding=False), BR.evaluate(*args, rounding=True, exact_leaky=exact)
        out["dx"], out["w"] = (hip["dx"], demu["dx"], d64["dx"]), (hip["tap_w"], demu["w"], d64["w"])
    return out


def main_case(arch, level, exact):
    key = ("main", arch, level, exact)
    if key not in _CACHE:
        hip = launch(arch, level, exact, *BR.MAIN)
        _CACHE[key] = (hip, references(arch, level, exact, hip))
    return _CACHE[key]


def emu_errors(t):
    """(max, rms) of |emulation - float64| of one tensor triple"""
    e = (t[1] - t[2]).abs()
    return float(e.max()), float((e ** 2).mean().sqrt())


@pytest.mark.parametrize("exact", [False, True], ids=["pattern", "exact"])
@pytest.mark.parametrize("arch", ARCHS)
def test_main_case(arch, exact):
    """65 x 13 = 845 samples, both levels: every tensor group held to the rule over the whole launch and over the 68 edge rows; the three
    negative controls fail it."""
    N, S = BR.MAIN
    P = N * S
    rows = BR.edge_rows(P)
    lines = []
    for level in (0, 1):
        hip, ref = main_case(arch, level, exact)
        recs = {}
        for name, (g, e, r) in ref.items():
            if name.startswith("_"):
                continue
            recs[name] = FR.held(g, e, r, "bf16 samples %s %s" % (hip["what"], name))
            lines.append(BR.line(recs[name]) + "  max |HIP - emulation| %.2e (not asserted)" % float((g.double() - e).abs().max()))
            lines.append(BR.line(FR.held(g, e, r, "bf16 samples %s %s, %d edge rows" % (hip["what"], name, len(rows)), rows)))
            assert recs[name][2] > 0.0 and recs[name][4] > 0.0, "%s %s: the emulation's error is zero: the rule is vacuous" % (hip["what"], name)
        # negative controls, values only
        raw, emu, r64 = ref["_raw"]
        partner = BR.swap_partner(r64, emu, N, S)
        assert partner is not None and partner // S != (P - 1) // S, hip["what"] + ": no separated row of another ray"
        controls = [("(a) rows P-1 and %d exchanged" % partner, BR.swapped(raw, P - 1, partner), BR.separated(r64, emu, P - 1, partner)),
                    ("(b) row P-1 copied over row P-257", BR.stale(raw), BR.separated(r64, emu, P - 1, P - 257)),
                    ("(c) 6 x the emulation's max error on colour logit 0 of row P-1", BR.nudged(raw, r64, emu, P - 1, 0), [("rgb", 0)])]
        for fault, bad, where in controls:
            assert where, "%s: %s: the two rows are not separated by 10 x the emulation's max error in any column" % (hip["what"], fault)
            for name in sorted({n for n, _ in where}):
                sl = dict(BR.GROUPS)[name]
                assert FR.would_fail(bad[:, sl], emu[:, sl], r64[:, sl], None), "%s: %s passes the rule on %s" % (hip["what"], fault, name)
                if not fault.startswith("(b)"):      # (row P-1 is an edge row; row P-257, where (b) lands, is not)
                    assert FR.would_fail(bad[:, sl], emu[:, sl], r64[:, sl], rows), "%s: %s passes the edge-row rule on %s" % (hip["what"], fault, name)
    print("\n".join(lines))


@pytest.mark.parametrize("exact", [False, True], ids=["pattern", "exact"])
@pytest.mark.parametrize("arch", ARCHS)
def test_small_sizes(arch, exact):
    """1 x 1, 1 x 33, 11 x 7 (held to the main case's emulation errors), 4 x 64, 257 x 1 (their own), both levels"""
    lines = []
    for N, S in BR.SIZES[:-1]:
        for level in (0, 1):
            hip = launch(arch, level, exact, N, S)
            ref = references(arch, level, exact, hip)
            main = main_case(arch, level, exact)[1]
            for name, (g, e, r) in ref.items():
                if name.startswith("_"):
                    continue
                what = "bf16 samples %s %s" % (hip["what"], name)
                if N * S < BR.TILE:
                    lines.append(BR.line(BR.hold_to(g, r, *emu_errors(main[name]), what + " (main case's measure)")))
                else:
                    lines.append(BR.line(FR.held(g, e, r, what)))
    print("\n".join(lines))
