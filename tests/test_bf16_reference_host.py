"""tests/bf16_reference.py on the host: the emulation that measures the plain-bf16 kernel's per-sample yardstick
(tests/test_gpu_bf16_samples.py) is what it says it is, and the seeded scenes make that test's rule and controls meaningful."""
import numpy as np
import pytest
import torch

import bf16_reference as BR
import field_reference as FR
from conftest import pkg

ARCHS = ("audio", "nerface", "nerface_static")
_CACHE = {}


def setup(arch):
    if arch not in _CACHE:
        _CACHE[arch] = BR.conditioning(pkg("weights"), arch, torch.device("cpu"))
    return _CACHE[arch]


def seam(arch, level, x6, exact=False):
    """the (x', w) a radiance launch would be evaluated at, as fp32 values: the emulation's own taps (audio: the bf16 kernel deforms), the
    float64 taps rounded to fp32 (nerface: an fp32 launch deforms), the point itself (nerface_static)"""
    sd, drv, p36 = setup(arch)
    if arch == "nerface_static":
        return x6[:, :3], None
    t = BR.evaluate(sd, arch, level, x6, drv, p36, rounding=(arch == "audio"), exact_leaky=exact)
    return BR.r32(t["xp"]).float(), BR.r32(t["w"]).float()


@pytest.mark.parametrize("arch", ARCHS)
def test_rounding_off_is_eager_field_in_float64(arch):
    """every rounding off: EagerField in float64 to 1e-12 of scale, both levels, whole network and radiance nets at a given seam"""
    sd, drv, p36 = setup(arch)
    _, _, x6 = FR.build_scene(arch, 11, 7, torch.device("cpu"))
    for level in (0, 1):
        for given in (None, seam(arch, level, x6)):
            raw, taps = BR.eager_f64(sd, arch, level, x6, drv, p36, given=given)
            off = BR.evaluate(sd, arch, level, x6, drv, p36, rounding=False, given=given)
            pairs = [("raw", off["raw"], raw)]
            if given is None and "warped" in taps:
                pairs += [("x'", off["xp"], taps["warped"]), ("w", off["w"], taps["amb"])]
            for name, a, b in pairs:
                assert a.dtype == torch.float64 and a.shape == b.shape
                err, scale = float((a - b).abs().max()), float(b.abs().max())
                assert err <= 1e-12 * scale, "%s L%d given=%s %s: %.3e on a scale of %.3e" % (arch, level, given is not None, name, err, scale)
            if given is not None and arch != "nerface_static":      # the seam is what was given, and it is used
                assert torch.equal(taps["warped"], given[0].double()) and torch.equal(taps["amb"], given[1].double())
                moved = BR.eager_f64(sd, arch, level, x6, drv, p36, given=(given[0] + 0.01, given[1]))[0]
                assert float((moved - raw).abs().max()) > 1e-6 * float(raw.abs().max())


def test_bf16_round_is_round_to_nearest_even_bit_for_bit():
    gen = torch.Generator().manual_seed(0)
    rnd = torch.randn(1 << 16, generator=gen) * torch.exp2(torch.randint(-60, 60, (1 << 16,), generator=gen).float())
    hi = torch.randint(0, 1 << 16, (4096,), generator=gen, dtype=torch.int64)
    ties = ((hi << 16) | 0x8000)                                           # exactly half way: to the even pattern
    near = torch.cat([ties - 1, ties + 1])                                 # one fp32 ulp to either side of a tie
    sub = torch.cat([torch.arange(0, 1 << 12, dtype=torch.int64) << 11, torch.tensor([1, 0x7FFF, 0x8000, 0x8001, 0x7FFFFF, 0x807FFFFF])])
    special = torch.tensor([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x3F808000, 0x3F818000], dtype=torch.int64)
    pat = torch.cat([ties, near, sub, special])
    pat = pat[((pat >> 23) & 0xFF != 0xFF) | ((pat & 0x7FFFFF) == 0)]      # no NaN patterns here (below)
    vals = torch.cat([rnd, torch.where(pat >= 2 ** 31, pat - 2 ** 32, pat).to(torch.int32).view(torch.float32)])
    for v in (vals, vals.double()):
        got = BR.bf16_round(v)
        assert got.dtype == v.dtype
        want = v.float().bfloat16().float()
        assert torch.equal(got.float().view(torch.int32), want.view(torch.int32))
    assert torch.equal(BR.bf16_round(torch.tensor([0.0, -0.0])).view(torch.int32), torch.tensor([0.0, -0.0]).view(torch.int32))
    assert bool(torch.isnan(BR.bf16_round(torch.tensor([float("nan")]))).all())


def test_leaky_pattern_slope():
    """pack_tick's LeakyReLU on bit patterns, every negative bf16 pattern: the slope applied.  Subtracting K = 850 = 6 x 128 + 82 from
    the pattern of -2^e (1 + m / 128) gives -2^(e-6) (1 + (m - 82) / 128) for m >= 82 and -2^(e-7) (1 + (m + 46) / 128) below, so the
    slope runs from 2^-6 / (1 + 82/128) = 0.0095238 (m = 82) to 2^-7 (1 + 46/128) = 0.0106201 (m = 0): the kernel's comment gives these two
    as "0.0095 .. 0.0106".  Asserted to that precision -- [0.0095, 0.0106 + 5e-5) -- and the two extremes exactly."""
    mag = torch.arange(0, 0x7F80, dtype=torch.int64)                       # every finite magnitude
    to_f = lambda p: torch.where(p >= 2 ** 31, p - 2 ** 32, p).to(torch.int32).view(torch.float32)
    neg, pos = to_f((0x8000 | mag) << 16), to_f(mag << 16)
    assert torch.equal(BR.leaky_pattern(pos).view(torch.int32), pos.view(torch.int32)), "positive patterns and +0 pass"
    out = BR.leaky_pattern(neg)
    assert torch.equal(out[:BR.LEAKY_K + 1].view(torch.int32), torch.full((BR.LEAKY_K + 1,), -2 ** 31, dtype=torch.int32)), "saturates at -0.0"
    assert bool((out <= 0).all()) and bool((out.view(torch.int32) < 0).all()), "the sign stays"
    # the result is a normal number from magnitude pattern K + 128 on (exponent field >= 1 after the subtraction)
    n = BR.LEAKY_K + 128
    slope = (out[n:].double() / neg[n:].double())
    print("pattern LeakyReLU: slope %.7f .. %.7f over %d negative patterns" % (float(slope.min()), float(slope.max()), slope.numel()))
    assert 0.0095 <= float(slope.min()) and float(slope.max()) < 0.0106 + 5e-5
    assert float(slope.min()) == 2.0 ** -6 / (1 + 82 / 128) and float(slope.max()) == 2.0 ** -7 * (1 + 46 / 128)
    # below that the result is subnormal or zero: the magnitude only shrinks further
    assert bool((out[:n].double().abs() <= 0.0106201 * neg[:n].double().abs()).all())
    # both dtypes, and the exact form for comparison: max(v, 0.01f v) rounded
    v = torch.tensor([-3.0, -1.0, -0.0, 0.0, 2.5], dtype=torch.float64)
    assert BR.leaky_pattern(v).dtype == torch.float64
    ex = BR.leaky_exact(v)
    assert torch.equal(ex[2:], v[2:]) and abs(float(ex[1]) + 0.01) < 0.01 * 2.0 ** -8 and abs(float(ex[0]) + 0.03) < 0.03 * 2.0 ** -8


@pytest.mark.parametrize("arch", ARCHS)
def test_main_scene_measure_and_controls(arch):
    """The seeded 65 x 13 scene: the emulation's own error is non-zero and finite in every tensor group (a zero measure would make the GPU
    rule vacuous), and the negative controls' partner rows exist: a row of another ray, and row P-257, whose float64 outputs differ from
    row P-1's by more than 10 x the emulation's max error in some column."""
    sd, drv, p36 = setup(arch)
    N, S = BR.MAIN
    P = N * S
    _, _, x6 = FR.build_scene(arch, N, S, torch.device("cpu"))
    for level in (0, 1):
        for exact in (False, True):
            what = "%s L%d %s" % (arch, level, "exact" if exact else "pattern")
            given = seam(arch, level, x6, exact)
            r64 = BR.evaluate(sd, arch, level, x6, drv, p36, rounding=False, given=given)["raw"]
            emu = BR.evaluate(sd, arch, level, x6, drv, p36, rounding=True, exact_leaky=exact, given=given)["raw"]
            triples = [(name, e, r) for (name, e), (_, r) in zip(BR.groups(emu), BR.groups(r64))]
            if arch == "audio":
                d64, demu = (BR.evaluate(sd, arch, level, x6, drv, p36, rounding=rd, exact_leaky=exact) for rd in (False, True))
                triples += [("dx", demu["dx"], d64["dx"]), ("w", demu["w"], d64["w"])]
            for name, e, r in triples:
                err = (e - r).abs()
                assert bool(torch.isfinite(e).all()) and bool(torch.isfinite(r).all()), what + " " + name
                emax, erms, scale = float(err.max()), float((err ** 2).mean().sqrt()), float(r.abs().max())
                print("%-28s %-6s |emulation - f64| max %.3e rms %.3e on a scale of %.3e" % (what, name, emax, erms, scale))
                assert emax > 0.0 and erms > 0.0 and np.isfinite(emax), what + " " + name
                assert emax < 0.1 * scale, "%s %s: the emulation is not near float64" % (what, name)
            partner = BR.swap_partner(r64, emu, N, S)
            assert partner is not None and partner // S != (P - 1) // S, what + ": control (a) has no partner row"
            assert BR.separated(r64, emu, P - 1, P - 257), what + ": control (b): rows P-1 and P-257 are not separated"
            # the controls, applied to the emulation's own output (it passes the rule against itself), fail it
            for fault, bad, where in (("(a)", BR.swapped(emu, P - 1, partner), BR.separated(r64, emu, P - 1, partner)),
                                      ("(b)", BR.stale(emu), BR.separated(r64, emu, P - 1, P - 257)),
                                      ("(c)", BR.nudged(emu, r64, emu, P - 1, 0), [("rgb", 0)])):
                for name in sorted({n for n, _ in where}):
                    sl = dict(BR.GROUPS)[name]
                    assert not FR.would_fail(emu[:, sl], emu[:, sl], r64[:, sl], None)
                    assert FR.would_fail(bad[:, sl], emu[:, sl], r64[:, sl], None), "%s: control %s passes the rule on %s" % (what, fault, name)


def test_edge_rows_and_borrowed_rule():
    rows = BR.edge_rows(845)
    assert set(range(781, 845)) <= set(rows) and {0, 256, 512, 768, 799, 800, 831, 832, 844} <= set(rows) and rows.max() == 844
    assert list(BR.edge_rows(1)) == [0] and list(BR.edge_rows(257)) == [0] + list(range(193, 257))
    ref = torch.linspace(-1, 1, 30).reshape(10, 3).double()
    BR.hold_to(ref + 2.9e-3, ref, 1e-3, 2e-3, "inside")
    with pytest.raises(AssertionError):
        BR.hold_to(ref + 3.1e-3, ref, 1e-3, 2e-3, "max")
    with pytest.raises(AssertionError):
        BR.hold_to(ref + 2.1e-3, ref, 1e-3, 1e-3, "rms")
