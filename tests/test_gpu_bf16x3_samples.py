"""The split-operand field kernels (field_radiance_bf16x3_kernel, field_deform_bf16x3_kernel, SAHS_BF16X3) held to float64, sample by sample.

Every bf16x3 forward evaluation that exists, both levels:
  audio           ops.field_forward_split(FIELD_DEFORM) at SAHS_BF16X3 into xw (rows wider than S, a column offset), then FIELD_RADIANCE at
                  SAHS_BF16X3 on that xw through a per-ray permutation src; FIELD_ALL (xw_col0 == 0) once at the main size
  nerface         the deformation kernel at SAHS_BF16X3 (the deformation launch of the model's mixed precision too: at the main size the
                  FIELD_DEFORM launch of the SAHS_BF16 pack must leave the same bits); FIELD_RADIANCE at SAHS_BF16X3 on the xw of an fp32
                  FIELD_DEFORM launch, through src; FIELD_ALL once at the main size
  nerface_static  ops.field_forward(..., precision=SAHS_BF16X3): the whole network is the radiance kernel
  saving forms    (SAVE = true instances, main size) ops.field_forward_split_save(FIELD_DEFORM, FIELD_RADIANCE) and, nerface_static,
                  ops.field_forward_save at SAHS_BF16X3: their raw and the dx, x', w planes they write (field_reference.act_table)

EXPECTED VALUE: oracle/torch_eager.py::EagerField in float64.  MEASURE: tests/bf16x3_reference.py::Bf16x3Field, the same network with
the kernels' rounding points, each cited to its line there.  RULE: conftest.yardstick with its defaults through field_reference.held,
got = HIP, ref32 = emulation, ref64 = float64: max |HIP - f64| <= 3 x max |emulation - f64|, rms <= 2 x, plus 32 fp32 ulps of the tensor's
scale.  The factors and the ulps are the same for every tensor; tests/test_bf16x3_reference_host.py proves on the host that the rule with
this measure rejects the loss of one cross term in any one dense layer.

Two seams, so that the 2^9 / 2^14 amplification of x' round-off in the encodings never enters a per-sample comparison:
  deformation seam (audio, nerface)  the kernel's x' - x and w, read back from xw, against EagerField's float64 taps at the launch's
                                     points; measure: the emulation's dx, w.
  radiance seam (all three)          the kernel's raw against float64 EagerField(given=...) AT THE KERNEL'S OWN x', w (the xw rows fed in;
                                     nerface_static: x); sigma, rgb logits, seg logits are separate tensors; measure: the emulation there.
The launch's points are bf16x3_reference.points: x = o + d z as the kernels form it, a rounded product and a rounded sum (the library is
built with -ffp-contract=off).  One fp32 ulp of x, amplified by 2^14 in the NeRFaceModel's encoding, is ten times the split-operand
error of dx (measured: a fused multiply-add in the test's x put the NeRFaceModel's dx at 1.1e-5 from float64 against the emulation's
1.3e-6), so the saving forms assert that these are the kernels' points bit for bit (the first three columns of the saved encoding
plane are the raw coordinates).

Sizes N x S (128-sample tiles, four 32-sample waves): 1 x 1, 1 x 33 (one past a wave), 11 x 7 = 77 (two waves and 13 samples), 4 x 32 = 128
(one tile), 129 x 1 (one sample in a second tile), 65 x 13 = 845 (MAIN: six tiles and a ragged 77).  The main case carries the statistics
and is also held over its edge rows alone (the last 32 samples, the first and last sample of every wave of the last tile, the first row
of every tile: 41 rows).  Sizes below 128 samples have too few values for a maximum of their own: they are held to the main case's
emulation errors with the same factors (bf16_reference.hold_to).  Outputs are the leading slice of a NaN-filled buffer whose guard rows
(two tiles' worth) must keep their bits, and so must every xw slot a deformation launch does not own.

FIELD_ALL is asserted BIT FOR BIT: its xw equals the FIELD_DEFORM launch's, its raw the FIELD_RADIANCE launch's on the same x', w
(through the permutation) -- the stronger of the two statements the rule would allow; being equal, it is held to the rule with them.
The saving forms are NOT assumed equal to the non-saving ones: they are held to the rule on their own, and the test prints whether the
bits agree.

Negative controls on the main case's HIP output, values only: (a) row P-1 exchanged with the separated row of another ray, (b) row P-1
copied over row P-129, (c) colour logit 0 of row P-1 moved away from float64 by twice the rule's allowance, 2 x (3 emu_max + eps).  Each
must fail the rule in the tensor group named, (a) and (c) on the edge rows as well; for (a), (b) the partner's float64 row differs from
row P-1's by more than 10 x the emulation's max error in a column of that group (proven for the seeded scenes on the host).

Observed on a 256-CU MI355X, main case (845 samples; 41 edge rows): max |HIP - f64| / max |emulation - f64| and the ratio of the two rms
errors, over the whole launch and over the edge rows.  The rule allows 3 (max) and 2 (rms); every negative control failed it.  No kernel
fault was found.  Unlike the plain-bf16 kernel, this one does not follow its emulation sample by sample: max |HIP - emulation| (printed
beside each line, not asserted) is about 0.6 x the emulation's own error, e.g. 2.1e-5 against 3.5e-5 in the static model's sigma.  What
the kernel does in fp32 in an order of its own (the accumulation inside the MFMA, the fold, the lookup) is no longer swamped by the
operand rounding; the difference was not attributed further.  The statistics agree.  dx and w do not depend on the level.
  model          L tensor max |HIP-f64| / max |emu-f64| = ratio  rms ratio   edge rows: max ratio       rms ratio
  audio          0 sigma  6.95e-04 / 7.00e-04 = 0.99   0.96        4.57e-04 / 6.06e-04 = 0.75  1.00
  audio          0 rgb    1.36e-04 / 1.17e-04 = 1.17   0.99        7.49e-05 / 7.55e-05 = 0.99  1.00
  audio          0 seg    2.23e-04 / 1.75e-04 = 1.28   1.00        1.04e-04 / 1.21e-04 = 0.86  1.00
  audio          0 dx     5.25e-07 / 5.50e-07 = 0.95   1.00        2.88e-07 / 4.32e-07 = 0.67  0.95
  audio          0 w      8.71e-06 / 8.46e-06 = 1.03   1.02        6.45e-06 / 5.51e-06 = 1.17  0.97
  audio          1 sigma  7.80e-04 / 9.56e-04 = 0.82   0.98        5.34e-04 / 5.48e-04 = 0.97  0.87
  audio          1 rgb    1.19e-04 / 1.24e-04 = 0.97   1.02        7.18e-05 / 6.68e-05 = 1.08  0.97
  audio          1 seg    1.33e-04 / 1.23e-04 = 1.08   0.99        1.09e-04 / 1.12e-04 = 0.97  1.03
  audio          1 dx     5.25e-07 / 5.50e-07 = 0.95   1.00        2.88e-07 / 4.32e-07 = 0.67  0.95
  audio          1 w      8.71e-06 / 8.46e-06 = 1.03   1.02        6.45e-06 / 5.51e-06 = 1.17  0.97
  nerface        0 sigma  3.51e-05 / 3.59e-05 = 0.98   1.03        1.99e-05 / 1.84e-05 = 1.08  0.97
  nerface        0 rgb    4.08e-07 / 4.18e-07 = 0.98   1.00        2.98e-07 / 2.99e-07 = 1.00  0.98
  nerface        0 seg    4.40e-07 / 4.60e-07 = 0.96   1.00        4.40e-07 / 4.60e-07 = 0.96  1.00
  nerface        0 dx     1.36e-06 / 1.13e-06 = 1.21   1.01        1.00e-06 / 9.00e-07 = 1.12  0.99
  nerface        0 w      1.31e-06 / 1.26e-06 = 1.04   1.00        7.83e-07 / 8.16e-07 = 0.96  1.00
  nerface        1 sigma  5.10e-05 / 5.19e-05 = 0.98   1.03        3.05e-05 / 3.21e-05 = 0.95  1.07
  nerface        1 rgb    3.91e-07 / 3.91e-07 = 1.00   1.01        2.98e-07 / 2.58e-07 = 1.15  1.10
  nerface        1 seg    4.75e-07 / 4.75e-07 = 1.00   1.01        4.75e-07 / 4.75e-07 = 1.00  1.03
  nerface        1 dx     1.36e-06 / 1.13e-06 = 1.21   1.01        1.00e-06 / 9.00e-07 = 1.12  0.99
  nerface        1 w      1.31e-06 / 1.26e-06 = 1.04   1.00        7.83e-07 / 8.16e-07 = 0.96  1.00
  nerface_static 0 sigma  3.64e-05 / 3.51e-05 = 1.04   1.03        2.31e-05 / 2.29e-05 = 1.01  0.97
  nerface_static 0 rgb    5.09e-07 / 4.90e-07 = 1.04   1.01        3.77e-07 / 4.15e-07 = 0.91  1.00
  nerface_static 0 seg    3.92e-07 / 4.17e-07 = 0.94   1.01        3.20e-07 / 3.30e-07 = 0.97  0.98
  nerface_static 1 sigma  2.68e-05 / 2.78e-05 = 0.97   1.04        1.81e-05 / 2.05e-05 = 0.88  1.10
  nerface_static 1 rgb    4.06e-07 / 3.79e-07 = 1.07   1.00        2.65e-07 / 2.77e-07 = 0.96  0.93
  nerface_static 1 seg    4.97e-07 / 4.84e-07 = 1.03   1.00        4.01e-07 / 4.02e-07 = 1.00  1.00
Other sizes, all three models, both levels: 4 x 32 and 129 x 1 against their own emulation: max ratio 0.75 .. 1.27, rms ratio 0.91 .. 1.11
(52 tensors); 1 x 1, 1 x 33, 11 x 7 against the main case's emulation errors: max ratio <= 1.29, rms ratio <= 1.88 (78 tensors; the largest
rms ratio is the three colour logits of the AudioFaceModel's single 1 x 1 sample, level 1: one sample's error against the rms of 845).  Saving forms
(raw, dx read back from xw, the dx plane, w; whole launch and edge rows, 60 tensors): max ratio 0.67 .. 1.28, rms ratio 0.83 .. 1.10; every
saving launch left the bits of the non-saving launch (xw of both deforming models, raw of the AudioFaceModel and the static NeRFaceModel;
the NeRFaceModel's two radiance launches read different x', w).  The hardware sine (v_sin_f32 after the exact reduction), read from the
saved fp32 encoding planes against float64 sin / cos of the same fp32 inputs: worst absolute error 3.7e-7 (PE(x), PE(x')), 2.1e-7 (PE(d)) --
a twentieth of the split's 2^-17 on a value near 1, so the emulation rounds an exact sine and models no error of the instruction.
"""
import pytest
import torch

import bf16x3_reference as X3
import field_reference as FR
from conftest import pkg

pytestmark = pytest.mark.gpu

_CACHE = {}
GUARD_ROWS = 256                 # two tiles
XW_PAD, XW_COL0 = 5, 3
ARCHS = ("audio", "nerface", "nerface_static")
DEFORMS = ("audio", "nerface")


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
        packs = dict(x3=ops.pack_weights(flat, ops.SAHS_BF16X3, arch=arch))
        if arch == "nerface":
            packs["fp32"] = ops.pack_weights(flat, ops.SAHS_F32, arch=arch)
            packs["mixed"] = ops.pack_weights(flat, ops.SAHS_BF16, arch=arch)
        _CACHE[("model", arch)] = dict(sd=X3.tensors(sd_np, dev()), frame=frame, packs=packs, drv=frame[0:76].clone(), p36=frame[80:116].clone())
    return _CACHE[("model", arch)]


def scene(arch, N, S):
    """-> rays, z, x6 (the kernels' points), src: a per-ray permutation of the owned xw columns"""
    rays, z, _ = FR.build_scene(arch, N, S, dev())
    return rays, z, X3.points(rays, z), (FR.ray_permutation(N, S, dev()) + XW_COL0).contiguous()


def guarded(P):
    buf = nan((P + GUARD_ROWS) * 16)
    return buf, buf[:P * 16]


def check_guard(buf, P, what):
    assert bool(torch.isfinite(buf[:P * 16]).all()), what + ": raw[:P] is not finite (a row was never written)"
    assert FR.same_bits(buf[P * 16:], nan(GUARD_ROWS * 16)), what + ": rows behind P were written"


def check_xw(xw, S, col0, what):
    """a deformation launch wrote x', w of its own slots (the row's three pad floats as zeros) and no other slot"""
    own = xw[:, col0:col0 + S]
    assert bool(torch.isfinite(own).all()) and bool((own[..., 5:] == 0).all()), what + ": x', w of the launch's own slots"
    for rest in (xw[:, :col0], xw[:, col0 + S:]):
        assert FR.same_bits(rest.contiguous(), torch.full_like(rest, float("nan")).contiguous()), what + ": an xw slot outside the launch's columns was written"


def fed_rows(xw, src, amb):
    """the (x', w) rows a radiance launch reads through src -> (P, 3), (P, amb)"""
    N, S = src.shape
    fed = torch.gather(xw, 1, src.long()[..., None].expand(N, S, 8)).reshape(N * S, 8)
    assert bool(torch.isfinite(fed[:, :5]).all()), "the deformation launch left x', w unwritten"
    return fed[:, 0:3], fed[:, 3:3 + amb]


def deform_taps(xw, x6, S, col0, amb):
    """what a reader of xw finds: dx = x' - x (exact in float64) and w, in sample order"""
    own = xw[:, col0:col0 + S].reshape(-1, 8)
    return own[:, 0:3].double() - x6[:, 0:3].double(), own[:, 3:3 + amb].clone()


def launch(arch, level, N, S):
    """One evaluation of every non-saving form -> dict: raw (P, 16), the seam it was evaluated at (xp (P, 3), w (P, AMB) or None), x6, and
    with deformation nets dx, tap_w of the split-operand deformation launch and its xw"""
    ops, m = pkg("ops"), model(arch)
    rays, z, x6, src = scene(arch, N, S)
    P, amb, fr, x3 = N * S, FR.ARCH_DIMS[arch]["amb"], m["frame"], ops.SAHS_BF16X3
    buf, flat = guarded(P)
    out = flat.view(N, S, 16)
    what = "%s %dx%d L%d" % (arch, N, S, level)
    res = dict(x6=x6, what=what, rays=rays, z=z, src=src)
    if arch in DEFORMS:
        xw = nan(N, S + XW_PAD, 8)
        ops.field_forward_split(m["packs"]["x3"], fr, level, ops.FIELD_DEFORM, rays, xw, z=z, xw_col0=XW_COL0, arch=arch, precision=x3)
        check_xw(xw, S, XW_COL0, what + " FIELD_DEFORM")
        res["dx"], res["tap_w"] = deform_taps(xw, x6, S, XW_COL0, amb)
        res["xw"] = xw
        seam_xw = xw
        if arch == "nerface":
            seam_xw = nan(N, S + XW_PAD, 8)
            ops.field_forward_split(m["packs"]["fp32"], fr, level, ops.FIELD_DEFORM, rays, seam_xw, z=z, xw_col0=XW_COL0, arch=arch, precision=ops.SAHS_F32)
        ops.field_forward_split(m["packs"]["x3"], fr, level, ops.FIELD_RADIANCE, rays, seam_xw, src=src, out=out, arch=arch, precision=x3, validate_src=True)
        res["xp"], res["w"] = fed_rows(seam_xw, src, amb)
    else:
        ops.field_forward(m["packs"]["x3"], fr, level, rays, z, precision=x3, out=out, arch=arch)
        res.update(xp=x6[:, :3], w=None)
    torch.cuda.synchronize()
    check_guard(buf, P, what)
    res["raw"] = out.reshape(P, 16).clone()
    return res


def references(arch, level, hip):
    """float64 and the emulation for one launch -> {tensor name: (HIP, emulation, float64)}: sigma, rgb, seg at the kernel's own seam, and
    with deformation nets dx, w at the launch's points"""
    m = model(arch)
    args = (m["sd"], arch, level, hip["x6"], m["drv"], m["p36"])
    given = (hip["xp"], hip["w"])
    r64 = X3.evaluate(*args, rounding=False, given=given)["raw"]
    emu = X3.evaluate(*args, rounding=True, given=given)["raw"]
    out = {name: (g, e, r) for (name, g), (_, e), (_, r) in zip(X3.groups(hip["raw"]), X3.groups(emu), X3.groups(r64))}
    out["_raw"] = (hip["raw"], emu, r64)
    if arch in DEFORMS:
        d64, demu = deform_references(arch, level, hip["x6"])
        out["dx"], out["w"] = (hip["dx"], demu["dx"], d64["dx"]), (hip["tap_w"], demu["w"], d64["w"])
    return out


def deform_references(arch, level, x6):
    """(float64, emulation) of the deformation nets at the points x6; they do not depend on the level's radiance nets, so one evaluation
    per scene serves both levels"""
    key = ("deform", arch, x6.shape[0])
    if key not in _CACHE:
        m = model(arch)
        _CACHE[key] = tuple(X3.evaluate(m["sd"], arch, level, x6, m["drv"], m["p36"], rounding=rd) for rd in (False, True))
    return _CACHE[key]


def main_case(arch, level):
    key = ("main", arch, level)
    if key not in _CACHE:
        hip = launch(arch, level, *X3.MAIN)
        _CACHE[key] = (hip, references(arch, level, hip))
    return _CACHE[key]


def table_row(arch, level, name, whole, edge):
    r = lambda a, b: a / b if b else float("inf")
    return "TABLE  %-14s %d %-6s %.2e / %.2e = %4.2f   %4.2f        %.2e / %.2e = %4.2f  %4.2f" % (
        arch, level, name, whole[1], whole[2], r(whole[1], whole[2]), r(whole[3], whole[4]), edge[1], edge[2], r(edge[1], edge[2]), r(edge[3], edge[4]))


def hold_all(ref, what, rows, lines, arch=None, level=None):
    """every tensor of `ref` over the whole launch and over the edge rows"""
    for name, (g, e, r) in ref.items():
        if name.startswith("_"):
            continue
        whole = FR.held(g, e, r, "bf16x3 samples %s %s" % (what, name))
        lines.append(X3.line(whole) + "  max |HIP - emulation| %.2e (not asserted)" % float((g.double() - e).abs().max()))
        edge = FR.held(g, e, r, "bf16x3 samples %s %s, %d edge rows" % (what, name, len(rows)), rows)
        lines.append(X3.line(edge))
        assert whole[2] > 0.0 and whole[4] > 0.0, "%s %s: the emulation's error is zero: the rule is vacuous" % (what, name)
        if arch is not None:
            lines.append(table_row(arch, level, name, whole, edge))


@pytest.mark.parametrize("arch", ARCHS)
def test_main_case(arch):
    """65 x 13 = 845 samples, both levels: every tensor held to the rule over the whole launch and over the 41 edge rows; the three
    negative controls fail it; FIELD_ALL leaves the bits of the two launches; the mixed-precision pack's deformation launch leaves the
    bits of the SAHS_BF16X3 pack's"""
    ops = pkg("ops")
    N, S = X3.MAIN
    P = N * S
    rows = X3.edge_rows(P)
    lines = []
    for level in (0, 1):
        hip, ref = main_case(arch, level)
        hold_all(ref, hip["what"], rows, lines, arch, level)
        # negative controls, values only
        raw, emu, r64 = ref["_raw"]
        partner = X3.swap_partner(r64, emu, N, S)
        assert partner is not None and partner // S != (P - 1) // S, hip["what"] + ": no separated row of another ray"
        controls = [("(a) rows P-1 and %d exchanged" % partner, X3.swapped(raw, P - 1, partner), X3.separated(r64, emu, P - 1, partner)),
                    ("(b) row P-1 copied over row P-129", X3.stale(raw), X3.separated(r64, emu, P - 1, P - 1 - X3.TILE)),
                    ("(c) twice the allowance on colour logit 0 of row P-1", X3.nudged(raw, r64, emu, P - 1, 0), [("rgb", 0)])]
        for fault, bad, where in controls:
            assert where, "%s: %s: the two rows are not separated by 10 x the emulation's max error in any column" % (hip["what"], fault)
            for name in sorted({n for n, _ in where}):
                sl = dict(X3.GROUPS)[name]
                assert FR.would_fail(bad[:, sl], emu[:, sl], r64[:, sl], None), "%s: %s passes the rule on %s" % (hip["what"], fault, name)
                if not fault.startswith("(b)"):      # (row P-1 is an edge row; row P-129, where (b) lands, is not)
                    assert FR.would_fail(bad[:, sl], emu[:, sl], r64[:, sl], rows), "%s: %s passes the edge-row rule on %s" % (hip["what"], fault, name)
        if arch not in DEFORMS:
            continue
        # FIELD_ALL (the split chain: xw_col0 == 0): the deformation launch's xw and the radiance launch's raw, bit for bit
        m, rays, z, x3 = model(arch), hip["rays"], hip["z"], ops.SAHS_BF16X3
        buf, flat = guarded(P)
        xw_all = nan(N, S + XW_PAD, 8)
        ops.field_forward_split(m["packs"]["x3"], m["frame"], level, ops.FIELD_ALL, rays, xw_all, z=z, xw_col0=0, out=flat.view(N, S, 16), arch=arch, precision=x3)
        torch.cuda.synchronize()
        check_guard(buf, P, hip["what"] + " FIELD_ALL")
        check_xw(xw_all, S, 0, hip["what"] + " FIELD_ALL")
        FR.assert_same_bits(xw_all[:, :S].contiguous(), hip["xw"][:, XW_COL0:XW_COL0 + S].contiguous(), hip["what"] + ": xw of FIELD_ALL vs FIELD_DEFORM")
        perm = (hip["src"] - XW_COL0).contiguous()
        two = hip["raw"]
        if arch == "nerface":      # (the main case's radiance launch read an fp32 launch's x', w: one more, on FIELD_ALL's own)
            two = ops.field_forward_split(m["packs"]["x3"], m["frame"], level, ops.FIELD_RADIANCE, rays, xw_all, src=perm, arch=arch, precision=x3,
                                          validate_src=True).reshape(P, 16)
        through = torch.gather(flat.view(N, S, 16), 1, perm.long()[..., None].expand(N, S, 16)).reshape(P, 16)
        FR.assert_same_bits(through, two, hip["what"] + ": raw of FIELD_ALL (through the permutation) vs FIELD_RADIANCE")
        if arch == "nerface" and level == 0:
            xw_mixed = nan(N, S + XW_PAD, 8)
            ops.field_forward_split(m["packs"]["mixed"], m["frame"], level, ops.FIELD_DEFORM, rays, xw_mixed, z=z, xw_col0=XW_COL0, arch=arch, precision=ops.SAHS_BF16)
            FR.assert_same_bits(xw_mixed, hip["xw"], hip["what"] + ": FIELD_DEFORM of the mixed-precision pack vs the SAHS_BF16X3 pack")
    print("\n".join(lines))


def planes_of(arch, act, P, part):
    """{name: (P, width) view} of the planes a save of `part` holds"""
    rows, _ = FR.act_table(arch)
    c0 = FR.act_col0(arch, part)
    return {name: FR.plane(act, P, col - c0, width) for name, col, width, defined, prt, _ in rows
            if defined and (part == FR.FIELD_ALL or prt == part or (name == "xw" and part == FR.FIELD_DEFORM))}


def sine_error(plane, x, L, inc):
    """worst |saved encoding - sin / cos (2^k x) in float64| over the plane's sinusoids (natural feature order: [x |] sin, cos per octave)"""
    D, x = x.shape[1], x.double()
    worst, c = 0.0, D if inc else 0
    for k in range(L):
        for fn in (torch.sin, torch.cos):
            worst = max(worst, float((plane[:, c:c + D].double() - fn(x * 2.0 ** k)).abs().max()))
            c += D
    return worst


@pytest.mark.parametrize("arch", ARCHS)
def test_saving_forms(arch):
    """The SAVE = true instances at the main size, both levels: raw and the dx, x' - x, w planes held to the rule (whole launch and edge
    rows); the planes' x is bf16x3_reference.points bit for bit; x', w of the planes are what the launch wrote to xw; printed: whether the
    saving launches leave the non-saving launches' bits, and the worst error of the saved fp32 encodings against float64 sin / cos."""
    ops, m = pkg("ops"), model(arch)
    N, S = X3.MAIN
    P, amb, x3, fr, pk = N * S, FR.ARCH_DIMS[arch]["amb"], ops.SAHS_BF16X3, m["frame"], m["packs"]["x3"]
    a = X3.BR.TE.EagerField.ARCH[arch]
    rows = X3.edge_rows(P)
    lines = []
    for level in (0, 1):
        main = main_case(arch, level)[0]
        rays, z, x6, src = main["rays"], main["z"], main["x6"], main["src"]
        what = "%s %dx%d L%d saving" % (arch, N, S, level)
        hip = dict(x6=x6)
        if arch in DEFORMS:
            xw = nan(N, S + XW_PAD, 8)
            bits_d, bits_r = (ops.alloc_sign_bits(P, part, arch, dev()) for part in (ops.FIELD_DEFORM, ops.FIELD_RADIANCE))
            _, act_d = ops.field_forward_split_save(pk, fr, level, ops.FIELD_DEFORM, rays, xw, z=z, xw_col0=XW_COL0, arch=arch, bits=bits_d, precision=x3)
            raw, act_r = ops.field_forward_split_save(pk, fr, level, ops.FIELD_RADIANCE, rays, xw, src=src, arch=arch, bits=bits_r, precision=x3)
            torch.cuda.synchronize()
            check_xw(xw, S, XW_COL0, what + " FIELD_DEFORM")
            pd, pr = planes_of(arch, act_d, P, FR.FIELD_DEFORM), planes_of(arch, act_r, P, FR.FIELD_RADIANCE)
            FR.assert_same_bits(pd["pe_x"][:, 0:3].contiguous(), x6[:, 0:3].contiguous(), what + ": the deformation kernel's points vs o + d z rounded once")
            own = xw[:, XW_COL0:XW_COL0 + S].reshape(P, 8)
            FR.assert_same_bits(pd["xw"][:, 0:3].contiguous(), own[:, 0:3].contiguous(), what + ": the x' plane vs xw")
            FR.assert_same_bits(pd["w"][:, 0:amb].contiguous(), own[:, 3:3 + amb].contiguous(), what + ": the w plane vs xw")
            hip["xp"], hip["w"] = fed_rows(xw, src, amb)
            FR.assert_same_bits(pr["xw"][:, 0:3].contiguous(), hip["xp"].contiguous(), what + ": the radiance save's point plane vs the xw rows fed in")
            hip["dx"], hip["tap_w"] = deform_taps(xw, x6, S, XW_COL0, amb)
            sines = [("PE(x), deformation save", sine_error(pd["pe_x"], x6[:, 0:3], a["L"], True)),
                     ("PE(x'), radiance save", sine_error(pr["pe_xw"], hip["xp"], a["L"], True)),
                     ("PE(d), radiance save", sine_error(pr["dir"], x6[:, 3:6], 4, True))]
            same = [("xw", FR.same_bits(xw, main["xw"]))]
            if arch == "audio":      # (the NeRFaceModel's non-saving radiance launch read an fp32 launch's x', w)
                same.append(("raw", FR.same_bits(raw.reshape(P, 16), main["raw"])))
        else:
            bits = ops.alloc_sign_bits(P, ops.FIELD_ALL, arch, dev())
            raw, act = ops.field_forward_save(pk, fr, level, rays, z, arch, bits=bits, precision=x3)
            torch.cuda.synchronize()
            pr = planes_of(arch, act, P, FR.FIELD_ALL)
            for nm in ("xw", "pe_xw"):
                FR.assert_same_bits(pr[nm][:, 0:3].contiguous(), x6[:, 0:3].contiguous(), what + ": the kernel's points (%s plane) vs o + d z rounded once" % nm)
            hip.update(xp=x6[:, :3], w=None)
            sines = [("PE(x)", sine_error(pr["pe_xw"], x6[:, 0:3], a["L"], True)), ("PE(d)", sine_error(pr["dir"], x6[:, 3:6], 4, True))]
            same = [("raw", FR.same_bits(raw.reshape(P, 16), main["raw"]))]
        assert bool(torch.isfinite(raw).all()), what + ": raw is not finite"
        hip["raw"] = raw.reshape(P, 16).clone()
        ref = references(arch, level, hip)
        if arch in DEFORMS:      # the dx plane is tanh(.) itself, before x' = x + dx is rounded
            ref["dx plane"] = (pd["dx"][:, 0:3].clone(), ref["dx"][1], ref["dx"][2])
        hold_all(ref, what, rows, lines)
        lines.append("SAVING %s: same bits as the non-saving launches: %s; saved fp32 encodings, worst |value - float64 sin/cos|: %s" % (
            what, ", ".join("%s %s" % (k, "yes" if v else "NO") for k, v in same), ", ".join("%s %.2e" % s for s in sines)))
    print("\n".join(lines))


@pytest.mark.parametrize("arch", ARCHS)
def test_small_sizes(arch):
    """1 x 1, 1 x 33, 11 x 7 (held to the main case's emulation errors), 4 x 32, 129 x 1 (their own), both levels"""
    lines = []
    for N, S in X3.SIZES[:-1]:
        for level in (0, 1):
            hip = launch(arch, level, N, S)
            ref = references(arch, level, hip)
            main = main_case(arch, level)[1]
            for name, (g, e, r) in ref.items():
                if name.startswith("_"):
                    continue
                what = "bf16x3 samples %s %s" % (hip["what"], name)
                if N * S < X3.TILE:
                    lines.append(X3.line(X3.hold_to(g, r, *X3.errors(main[name][1], main[name][2]), what + " (main case's measure)")))
                else:
                    lines.append(X3.line(FR.held(g, e, r, what)))
    print("\n".join(lines))
