"""tests/bf16x3_reference.py on the host: the emulation that measures the split-operand kernels' per-sample yardstick
(tests/test_gpu_bf16x3_samples.py) is what it says it is, the seeded scenes make that test's rule and controls meaningful, and the rule
with this measure rejects a kernel that loses ONE cross term in ONE dense layer.

The mutant sweep (test_single_layer_mutants_fail_the_rule), on the 65 x 13 main scene, both levels, at the seams of the GPU test: every
dense layer the level evaluates x {no_wlo: W_lo x_hi left out, no_xlo: W_hi x_lo left out, hi_only: both, plain bf16 in that layer}.
Result (printed by the test): every one of them fails the rule in a tensor of its seam -- AudioFaceModel 34 layers per level, NeRFaceModel
30, NeRFaceModel without deformation nets 16; 480 mutants, none missed, with build_scene's seeded scene as it is.  The smallest
single-layer mutant (W_lo x_hi left out of nerf_mlps.coarse.layers_seg.0 of the NeRFaceModel without deformation nets) moves raw by
0.012 x (6e-5 of raw's scale), the bound tests/test_gpu_nerface_bf16x3.py holds the kernels to against the fp32 kernel; the smallest of
the NeRFaceModel 0.014 x, of the AudioFaceModel 4.7 x.  That bound cannot see the NeRFaceModels' mutants; the rule here sees all.
"""
import numpy as np
import pytest
import torch

import bf16x3_reference as X3
import field_reference as FR
from conftest import pkg

ARCHS = ("audio", "nerface", "nerface_static")
_CACHE = {}


def setup(arch):
    if arch not in _CACHE:
        _CACHE[arch] = X3.conditioning(pkg("weights"), arch, torch.device("cpu"))
    return _CACHE[arch]


def seam(arch, level, x6):
    """the (x', w) a radiance launch of the GPU test is evaluated at, as fp32 values: the emulation's own (audio: the split-operand kernel
    deforms), the float64 taps rounded to fp32 (nerface: an fp32 launch deforms), the point itself (nerface_static)"""
    sd, drv, p36 = setup(arch)
    if arch == "nerface_static":
        return x6[:, :3], None
    t = X3.evaluate(sd, arch, level, x6, drv, p36, rounding=(arch == "audio"))
    return X3.r32(t["xp"]).float(), X3.r32(t["w"]).float()


def main_case(arch, level):
    """-> x6, seam, and {tensor: (emulation, float64)} of the GPU test's main case: sigma, rgb, seg at the seam, dx, w of the deformation nets"""
    key = ("main", arch, level)
    if key not in _CACHE:
        sd, drv, p36 = setup(arch)
        _, _, x6 = FR.build_scene(arch, *X3.MAIN, torch.device("cpu"))
        given = seam(arch, level, x6)
        r64 = X3.evaluate(sd, arch, level, x6, drv, p36, rounding=False, given=given)["raw"]
        emu = X3.evaluate(sd, arch, level, x6, drv, p36, rounding=True, given=given)["raw"]
        t = {name: (e, r) for (name, e), (_, r) in zip(X3.groups(emu), X3.groups(r64))}
        t["_raw"] = (emu, r64)
        if arch != "nerface_static":
            d64, demu = (X3.evaluate(sd, arch, level, x6, drv, p36, rounding=rd) for rd in (False, True))
            t["dx"], t["w"] = (demu["dx"], d64["dx"]), (demu["w"], d64["w"])
        _CACHE[key] = (x6, given, t)
    return _CACHE[key]


@pytest.mark.parametrize("arch", ARCHS)
def test_rounding_off_is_eager_field_in_float64(arch):
    """every rounding off: EagerField in float64 to 1e-12 of scale, both levels, whole network and radiance nets at a given seam"""
    sd, drv, p36 = setup(arch)
    _, _, x6 = FR.build_scene(arch, 11, 7, torch.device("cpu"))
    for level in (0, 1):
        for given in (None, seam(arch, level, x6)):
            raw, taps = X3.eager_f64(sd, arch, level, x6, drv, p36, given=given)
            layers = []
            off = X3.evaluate(sd, arch, level, x6, drv, p36, rounding=False, given=given, layers=layers)
            pairs = [("raw", off["raw"], raw)]
            if given is None and "warped" in taps:
                pairs += [("x'", off["xp"], taps["warped"]), ("w", off["w"], taps["amb"])]
            for name, a, b in pairs:
                assert a.dtype == torch.float64 and a.shape == b.shape
                err, scale = float((a - b).abs().max()), float(b.abs().max())
                assert err <= 1e-12 * scale, "%s L%d given=%s %s: %.3e on a scale of %.3e" % (arch, level, given is not None, name, err, scale)
            deform, radiance = X3.layer_names(arch, level)      # (the mutant sweep's list IS what a forward evaluates)
            assert layers == (radiance if given is not None else deform + radiance), layers
            if given is not None and arch != "nerface_static":      # the seam is what was given, and it is used
                assert torch.equal(taps["warped"], given[0].double()) and torch.equal(taps["amb"], given[1].double())
                moved = X3.eager_f64(sd, arch, level, x6, drv, p36, given=(given[0] + 0.01, given[1]))[0]
                assert float((moved - raw).abs().max()) > 1e-6 * float(raw.abs().max())


def test_split_is_split_pair():
    """hi = bf16_rne(x) and lo = bf16_rne(x - hi), bit for bit against torch's own bfloat16 conversion, on random values over +-60
    binades, ties, values one ulp from a tie, subnormals and specials; hi + lo within 2^-16 relative of x for normal numbers (hi keeps 8
    significant bits, the remainder |x - hi| <= 2^-9 |x| keeps 8 more: 2^-9 x 2^-8 x (1 + 2^-8) < 2^-16)."""
    gen = torch.Generator().manual_seed(0)
    rnd = torch.randn(1 << 16, generator=gen) * torch.exp2(torch.randint(-60, 60, (1 << 16,), generator=gen).float())
    hi16 = torch.randint(0, 1 << 16, (4096,), generator=gen, dtype=torch.int64)
    ties = (hi16 << 16) | 0x8000
    near = torch.cat([ties - 1, ties + 1])
    sub = torch.cat([torch.arange(0, 1 << 12, dtype=torch.int64) << 11, torch.tensor([1, 0x7FFF, 0x8000, 0x8001, 0x7FFFFF, 0x807FFFFF])])
    special = torch.tensor([0x00000000, 0x80000000, 0x7F7FFFFF, 0xFF7FFFFF, 0x3F808000, 0x3F818000, 0x7F000000], dtype=torch.int64)
    pat = torch.cat([ties, near, sub, special])
    pat = pat[(pat >> 23) & 0xFF != 0xFF]                                  # finite patterns (infinities and NaN below)
    vals = torch.cat([rnd, torch.where(pat >= 2 ** 31, pat - 2 ** 32, pat).to(torch.int32).view(torch.float32)])
    for v in (vals, vals.double()):
        hi, lo = X3.split(v)
        assert hi.dtype == v.dtype and lo.dtype == v.dtype
        want_hi = v.float().bfloat16().float()
        assert torch.equal(hi.float().view(torch.int32), X3.bf16_round(v).float().view(torch.int32))
        assert torch.equal(hi.float().view(torch.int32), want_hi.view(torch.int32))
        ok = torch.isfinite(want_hi)                                       # (the largest fp32 numbers round up to infinity: no remainder)
        want_lo = (v.float() - want_hi).bfloat16().float()
        assert torch.equal(lo.float()[ok].view(torch.int32), want_lo[ok].view(torch.int32))
        assert torch.equal(lo.float()[ok].view(torch.int32), X3.bf16_round(v.float() - want_hi)[ok].view(torch.int32))
        assert bool(((v.double() - hi.double()).float().double() == v.double() - hi.double())[ok].all()), "x - hi is exact in fp32"
        normal = ok & (v.float().abs() >= 2.0 ** -126 * 2.0 ** 17)         # (lo of a smaller x may be subnormal)
        rel = ((hi.double() + lo.double() - v.double()).abs() / v.double().abs())[normal]
        assert float(rel.max()) <= 2.0 ** -16, float(rel.max())
    inf = torch.tensor([float("inf"), -float("inf")])
    assert torch.equal(X3.split(inf)[0], inf) and bool(torch.isnan(X3.split(torch.tensor([float("nan")]))[0]).all())


@pytest.mark.parametrize("arch", ARCHS)
def test_main_scene_measure_and_controls(arch):
    """The seeded 65 x 13 scene, both levels, every tensor group at its seam: the emulation's own error is non-zero and finite (a zero
    measure would make the GPU rule vacuous); eps / emu_max is printed, and the tensors in which the 32-ulp term leads (ratio > 1) are
    named; the negative controls' partner rows exist -- a row of another ray, and row P-129, whose float64 outputs differ from row P-1's by
    more than 10 x the emulation's max error in some column -- and the three controls, applied to the emulation's own output, fail the
    rule."""
    N, S = X3.MAIN
    P = N * S
    rows = X3.edge_rows(P)
    leads = []
    for level in (0, 1):
        what = "%s L%d" % (arch, level)
        _, _, t = main_case(arch, level)
        for name, (e, r) in t.items():
            if name.startswith("_"):
                continue
            assert bool(torch.isfinite(e).all()) and bool(torch.isfinite(r).all()), what + " " + name
            (emax, erms), (allow, _, eps), scale = X3.errors(e, r), X3.allowance(e, r), float(r.abs().max())
            print("%-18s %-6s |emulation - f64| max %.3e (%.2e of scale) rms %.3e  eps %.3e  eps / emu_max %6.2f" % (what, name, emax, emax / scale, erms, eps, eps / emax))
            assert emax > 0.0 and erms > 0.0 and np.isfinite(emax), what + " " + name
            assert emax < 1e-3 * scale, "%s %s: the emulation is not near float64" % (what, name)
            if eps > emax:
                leads.append("%s %s (%.1f)" % (what, name, eps / emax))
        emu, r64 = t["_raw"]
        partner = X3.swap_partner(r64, emu, N, S)
        assert partner is not None and partner // S != (P - 1) // S, what + ": control (a) has no partner row"
        assert X3.separated(r64, emu, P - 1, P - 1 - X3.TILE), what + ": control (b): rows P-1 and P-129 are not separated"
        for fault, bad, where in (("(a)", X3.swapped(emu, P - 1, partner), X3.separated(r64, emu, P - 1, partner)),
                                  ("(b)", X3.stale(emu), X3.separated(r64, emu, P - 1, P - 1 - X3.TILE)),
                                  ("(c)", X3.nudged(emu, r64, emu, P - 1, 0), [("rgb", 0)])):
            for name in sorted({n for n, _ in where}):
                sl = dict(X3.GROUPS)[name]
                assert not FR.would_fail(emu[:, sl], emu[:, sl], r64[:, sl], None)
                assert FR.would_fail(bad[:, sl], emu[:, sl], r64[:, sl], None), "%s: control %s passes the rule on %s" % (what, fault, name)
                if fault != "(b)":
                    assert FR.would_fail(bad[:, sl], emu[:, sl], r64[:, sl], rows), "%s: control %s passes the edge-row rule on %s" % (what, fault, name)
    print("%s: the 32-ulp term leads the allowance (eps / emu_max > 1) in: %s" % (arch, ", ".join(leads) if leads else "no tensor"))


@pytest.mark.parametrize("arch", ARCHS)
def test_single_layer_mutants_fail_the_rule(arch):
    """Every dense layer of both levels x {no_wlo, no_xlo, hi_only}: the mutant's output as `got`, the true emulation as the measure, float64
    as the expected value -> conftest.yardstick rejects it in a tensor of the layer's seam (deformation layers: dx or w at the launch's
    points; radiance layers: sigma, rgb or seg at the given seam).  None may pass, and hi_only fails wherever no_xlo does."""
    sd, drv, p36 = setup(arch)
    missed, smallest, count = [], None, 0
    for level in (0, 1):
        x6, given, t = main_case(arch, level)
        deform, radiance = X3.layer_names(arch, level)
        for name in deform + radiance:
            failed = {}
            for kind in X3.MUTANTS:
                if name in radiance:
                    raw = X3.evaluate(sd, arch, level, x6, drv, p36, rounding=True, given=given, mutant=(name, kind))["raw"]
                    got = dict(X3.groups(raw))
                    whole = (raw, t["_raw"][0], t["_raw"][1])
                else:
                    got = X3.evaluate(sd, arch, level, x6, drv, p36, rounding=True, mutant=(name, kind))
                    whole = None
                ratios = {}
                for tensor in X3.judged_on(name):
                    e, r = t[tensor]
                    assert not FR.would_fail(e, e, r, None)
                    allow = X3.allowance(e, r)[0]
                    ratios[tensor] = float((got[tensor] - r).abs().max()) / allow
                    if FR.would_fail(got[tensor], e, r, None):
                        failed.setdefault(kind, []).append(tensor)
                count += 1
                if kind not in failed:
                    missed.append("%s L%d %s %s: max |mutant - f64| / allowance = %s" % (arch, level, name, kind, ratios))
                if kind != "hi_only":      # how far the mutant moves its output, in units of the bound the fp32-kernel comparison uses
                    g, e, r = whole if whole is not None else max(((got[k], *t[k]) for k in X3.judged_on(name)), key=lambda a: float((a[0] - a[1]).abs().max() / a[2].abs().max()))
                    moved = float((g - e).abs().max() / r.abs().max()) / 6e-5
                    if smallest is None or moved < smallest[0]:
                        smallest = (moved, "%s L%d %s %s" % (arch, level, name, kind))
            assert set(failed.get("no_xlo", [])) <= set(failed.get("hi_only", [])), "%s L%d %s: hi_only passes where no_xlo fails" % (arch, level, name)
    print("%s: %d single-layer mutants, %d pass the rule; the smallest (no_wlo / no_xlo) moves its output by %.3f x (6e-5 of scale): %s"
          % (arch, count, len(missed), smallest[0], smallest[1]))
    assert not missed, "mutants the rule does not see:\n" + "\n".join(missed)


def test_edge_rows_and_allowance():
    rows = X3.edge_rows(845)
    assert set(range(813, 845)) <= set(rows) and {0, 128, 256, 384, 512, 640, 768, 799, 800, 831, 832, 844} <= set(rows) and rows.max() == 844
    assert len(rows) == 7 + 2 + 32 and list(X3.edge_rows(1)) == [0] and list(X3.edge_rows(129)) == [0] + list(range(97, 129))
    assert list(X3.edge_rows(128)) == [0, 31, 32, 63, 64, 95] + list(range(96, 128))
    ref = torch.linspace(-1, 1, 30).reshape(10, 3).double()
    emu = ref + 1e-3
    allow, emax, eps = X3.allowance(emu, ref)
    assert abs(emax - 1e-3) < 1e-12 and eps == 32 * 2.0 ** -24 and allow == 3 * emax + eps
    one = ref.clone()                                                          # (one entry: the max term alone decides)
    one[3, 1] += 0.999 * allow
    assert not FR.would_fail(one, emu, ref, None)
    one[3, 1] = ref[3, 1] + 1.001 * allow
    assert FR.would_fail(one, emu, ref, None)
    # control (c) leaves the allowance also where eps leads it by far
    raw64 = torch.linspace(-2, 2, 64).reshape(4, 16).double()
    tiny = raw64 + 1e-12
    bad = X3.nudged(raw64.clone(), raw64, tiny, 3, 0)
    assert FR.would_fail(bad[:, 0:3], tiny[:, 0:3], raw64[:, 0:3], None) and not FR.would_fail(tiny[:, 0:3], tiny[:, 0:3], raw64[:, 0:3], None)
