"""Host checks behind tests/test_gpu_render_tails.py: the references that file holds the HIP render stages to, and its inputs.

 * The float64 compositor (tests/render_reference.py: composite64) against the two fp32 references -- the C oracle and the torch-eager
   restatement -- on every regime, size and option of the GPU test.  Each fp32 reference must meet the yardstick with the OTHER one's
   error as the allowance: that is what makes "as close to float64 as the reference's own fp32" a bound a correct fp32 compositor meets.
 * Sensitivity: composite64's deliberately wrong results, rounded to fp32 and fed to the yardstick as ``got``, must be rejected -- for
   every size, option and applicable fault by at least one regime -- so that an edit of the inputs cannot make the GPU test blind.
 * The C oracle's sample_pdf_2 / resample against ATen itself, bit for bit, over the GPU test's size and weight sweep, and the sweep's
   branch coverage (which row-sum form, which cumsum path, how many scan blocks): conditions on the inputs, asserted here and there.
"""
import numpy as np
import pytest
import torch

import conftest
import render_reference as rr
from conftest import yardstick
from oracle import oracle, torch_eager


def rejected(got, r32, r64, what):
    """True if the yardstick (defaults, scale_floor=1, no ray left out) rejects ``got`` on any of the five outputs."""
    n = len(conftest.YARDSTICK_LOG)
    hit = False
    for nm, g, a, b in zip(rr.OUTPUTS, got, r32, r64):
        try:
            yardstick(np.asarray(g, np.float32), a, b, what + " " + nm, scale_floor=1.0)
        except AssertionError:
            hit = True
    del conftest.YARDSTICK_LOG[n:]          # probes, not results: keep them out of the terminal summary
    return hit


@pytest.mark.parametrize("opt", list(rr.OPTIONS))
@pytest.mark.parametrize("S", rr.COMPOSITE_S)
def test_composite_references_and_sensitivity(S, opt):
    worst = 0.0
    caught = {f: [] for f in rr.FAULTS if rr.fault_applies(f, S, opt)}
    for regime in rr.REGIMES:
        case = rr.composite_case(regime, S, opt)
        r32, r64 = rr.composite_refs(case, oracle)
        t32 = rr.torch_volume_render(case, torch_eager)
        what = "%s S=%d %s" % (regime, S, opt)
        n = len(conftest.YARDSTICK_LOG)
        for nm, a, t, b in zip(rr.OUTPUTS, r32, t32, r64):
            assert np.all(np.isfinite(b)), what + " " + nm
            worst = max(worst, yardstick(a, t, b, what + " oracle " + nm, scale_floor=1.0)[1] / max(1.0, np.abs(b).max()))
            yardstick(t, a, b, what + " torch " + nm, scale_floor=1.0)
        del conftest.YARDSTICK_LOG[n:]
        assert not rejected(r64, r32, r64, what), what + ": the float64 result itself does not pass"
        for f in caught:
            if rejected(rr.composite64(case["raw"], case["z"], case["rd"], case["noise"], case["bg"], case["white"], fault=f), r32, r64, what):
                caught[f].append(regime)
    assert worst < 4e-6, worst         # the C oracle within a few fp32 ulps of the exact value, relative to max(1, scale)
    blind = [f for f, regs in caught.items() if not regs]
    assert not blind, "S=%d %s: no regime makes the yardstick reject fault(s) %s" % (S, opt, blind)
    if "extra_factor" in caught:       # a leaked factor of the last sample (~1e-10) wipes every later weight: no regime hides that
        assert caught["extra_factor"] == list(rr.REGIMES), caught


def test_faults_listed_where_they_apply():
    assert not rr.fault_applies("carry", 64, "plain") and rr.fault_applies("carry", 65, "plain")
    assert not rr.fault_applies("extra_factor", 1, "plain") and rr.fault_applies("extra_factor", 2, "plain")
    assert rr.fault_applies("prior", 1, "prior") and not rr.fault_applies("prior", 1, "white")
    case = rr.composite_case("thin", 129, "prior")
    clean = rr.composite64(case["raw"], case["z"], case["rd"], None, case["bg"])
    for f in rr.FAULTS:
        bad = rr.composite64(case["raw"], case["z"], case["rd"], None, case["bg"], fault=f)
        assert any(not np.array_equal(a, b) for a, b in zip(clean, bad)), f


def sweep():
    for S in rr.RESAMPLE_S:
        for nf in rr.RESAMPLE_NF:
            for rand_u in (False, True):
                yield S, nf, rand_u


def test_resample_oracle_is_aten_bit_for_bit_and_sweep_covers_every_branch():
    cov = rr.Coverage()
    for S, nf, rand_u in sweep():
        z, w, u, fam = rr.resample_case(S, nf, rand_u)
        bins, wm = 0.5 * (z[:, 1:] + z[:, :-1]), np.ascontiguousarray(w[:, 1:-1])
        ts, ti, small = rr.torch_sample_pdf(bins, wm, nf, u)
        what = "S=%d nf=%d %s" % (S, nf, "rand" if rand_u else "det")
        te = torch_eager.sample_pdf_2(torch.from_numpy(bins), torch.from_numpy(wm), nf, u=None if u is None else torch.from_numpy(u)).numpy()
        assert np.array_equal(rr.bits(te), rr.bits(ts)), what        # (torch_sample_pdf is torch_eager's, also returning inds and the denom count)
        os_, oi = oracle.sample_pdf_2(bins, wm, nf, u=u)
        assert np.array_equal(oi, ti) and np.array_equal(rr.bits(os_), rr.bits(ts)), what
        zs, zo, inds = oracle.resample(z, w, nf, u=u)
        assert np.array_equal(inds, ti) and np.array_equal(rr.bits(zs), rr.bits(ts)), what
        assert np.array_equal(rr.bits(zo), rr.bits(rr.torch_merge(z, ts)[0])), what
        if rand_u:
            assert (u == 0.0).any() and (u == np.float32(rr.U_LAST)).any() and u.max() < 1.0
        cov.add(rr.branch_rows(w, oracle), fam, small)
    assert not cov.missing(), cov.missing()


@pytest.mark.parametrize("S,nf", [(64, 64), (64, 63), (65, 64), (13, 7), (4, 4)])
def test_resample_oracle_merges_as_torch_sort_on_unsorted_and_tied_rows(S, nf):
    z, w, u, kind = rr.merge_case(S, nf)
    zs, zo, _ = oracle.resample(z, w, nf, u=u)
    v, src = rr.torch_merge(z, zs)
    assert np.array_equal(rr.bits(zo), rr.bits(v))
    cat = np.concatenate([z, zs], axis=1)
    assert np.array_equal(np.sort(src, axis=1), np.broadcast_to(np.arange(S + nf), src.shape))
    assert np.array_equal(rr.bits(np.take_along_axis(cat, src, 1)), rr.bits(v))
    ties = (np.diff(v, axis=1) == 0)
    assert ties[kind == 2].all() and ties[kind == 3].any()
    assert np.all(np.diff(src, axis=1)[ties] > 0)          # torch's stable order: equal values keep ascending source index


def test_branch_helper():
    """branch_rows on rows whose branch is known by construction."""
    w = np.zeros((4, 12), np.float32)                       # np = 10: vector form, remainder 2, no group of four
    w[1, 3] = 1.0                                           # quotients 1e-5/1.00009 and ~1: exponents 17 binades apart
    w[2, 3] = np.float32(2.0 ** 21 * 1e-5)                  # ~2^21 x the others
    w[3, 5] = np.nan
    rows = rr.branch_rows(w, oracle)
    assert [r["form"] for r in rows] == ["vector"] * 4 and rows[0]["rem"] == 2 and rows[0]["groups"] == 0 and rows[0]["blocks"] == 1
    assert rows[0]["span"] == 0 and rows[0]["path"] == "scan"
    assert rows[1]["span"] in (16, 17) and rows[1]["path"] == "scan"
    assert rows[2]["span"] >= 21 and rows[2]["path"] == "sequential"
    assert rows[3]["span"] == 255 and rows[3]["path"] == "sequential"
    small = rr.branch_rows(np.ones((1, 9), np.float32), oracle)[0]
    assert small["form"] == "scalar" and small["np"] == 7
    big = rr.branch_rows(np.ones((1, 256), np.float32), oracle)[0]
    assert big["groups"] == 7 and big["rem"] == 6 and big["blocks"] == 4
    cov = rr.Coverage()
    cov.add(rows, [0] * 4, [0] * 4)
    assert "row sum, np < 8 form" in cov.missing() and "lane scan over 2 blocks of 64" in cov.missing()
