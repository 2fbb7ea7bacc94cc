"""The render stages around the field kernel (csrc/render_ops.hip) at their wave, branch and size edges, on the MI355X.

 * composite_forward_kernel against the reference's formulas in FLOAT64 (tests/render_reference.py: composite64) under the float64
   yardstick -- as close to the exact value as the reference's own fp32 result (the C oracle) is, every ray counted -- at every sample
   count around its 64-sample blocks, in five density regimes (moderate; opaque mid-ray, transmittance denormal then zero; empty, the
   weight on the last sample; saturated colour logits; thin, the weight on the tail samples) and four option sets, N = 67 rays (not a
   multiple of the 4 rays of a workgroup).  tests/test_render_reference_host.py asserts that these inputs make the yardstick reject a
   compositor with a reset carry, a missing far distance or prior, a dropped last sample or a leaked factor.  The row-block form is
   bit-identical to the dense one and touches no column it does not own.
 * resample_kernel bit for bit against the C oracle (= ATen, bit for bit, on the same sweep: the host file) on every branch.  Branches,
   decided per row on the host as the kernel decides them (render_reference.branch_rows) and ASSERTED covered:
     - the row sum's np < 8 form (np = S - 2 pdf entries);
     - its np >= 8 form with every np % 8 in 0..7 and with 0, 1 and >= 2 groups of four 8-lane vectors;
     - the float64 cumsum as a lane scan (quotient exponents span <= 20) with the span exactly 20, and over 1, 2, 3 and 4 blocks of 64;
     - the sequential cumsum (span >= 21), over 1, 2, 3 and 4 blocks;
     - denom < 1e-5 -> 1 on at least one draw of every weight family.
 * the merge sort's two paths (sorted row with S % 4 == 0 and nf % 4 == 0 | general count) on sorted, unsorted, flat and tied rows mixed
   in one launch: sorted values, the permutation src, and the stable order of ties.
 * non-finite coarse weights: src stays a permutation, every slot is written, NaNs sort last in index order (torch.sort's order).
 * route_xw_grad against a numpy scatter, bit for bit, including its grid-stride loop; the ray-stride loops of composite and resample;
   stratified depths at S = 3, 255, 256, near == far, lindisp with S = 1; uniform draws in [0, 1).
"""
import ctypes

import numpy as np
import pytest
import torch

import render_reference as rr
from conftest import pkg, yardstick
from test_gpu_parity import T, close, dev

pytestmark = pytest.mark.gpu

from oracle import oracle, torch_eager  # noqa: E402,F401  (checkers only)


@pytest.fixture(scope="module")
def ops():
    return pkg("ops")


def hip_composite(ops, case):
    return ops.composite_forward(T(case["raw"]), T(case["z"]), T(case["rays"]), noise=None if case["noise"] is None else T(case["noise"]),
                                 bg=None if case["bg"] is None else T(case["bg"]), white_background=case["white"])


@pytest.mark.parametrize("opt", list(rr.OPTIONS))
@pytest.mark.parametrize("regime", rr.REGIMES)
@pytest.mark.parametrize("S", rr.COMPOSITE_S)
def test_composite_forward_vs_float64(ops, S, regime, opt):
    case = rr.composite_case(regime, S, opt)
    r32, r64 = rr.composite_refs(case, oracle)
    outs = hip_composite(ops, case)
    recs = [(nm, np.abs(o.cpu().numpy().astype(np.float64).reshape(b.shape) - b).max(), np.abs(a - b).max()) for nm, o, a, b in zip(rr.OUTPUTS, outs, r32, r64)]
    print("composite %s S=%d %s: " % (regime, S, opt) + "  ".join("%s %.2e (ref %.2e)" % r for r in recs))
    for nm, o, a, b in zip(rr.OUTPUTS, outs, r32, r64):
        yardstick(o, a, b, "composite %s S=%d %s %s" % (regime, S, opt, nm), scale_floor=1.0, outlier_rays=0)


@pytest.mark.parametrize("S", [1, 65, 256])
def test_composite_forward_rows(ops, S):
    """The row-block form (strides 36 / 36, w_last): the columns a pass owns are the dense call's outputs bit for bit, w_bg is
    weights[:, -1], and every other column of the NaN-prefilled block is still NaN."""
    case = rr.composite_case("thin", S, "prior_noise", N=67, seed=3)
    args = (T(case["raw"]), T(case["z"]), T(case["rays"]))
    kw = dict(noise=T(case["noise"]), bg=T(case["bg"]))
    rgb, disp, acc, w, depth = (o.cpu().numpy() for o in ops.composite_forward(*args, **kw))
    for fine in (False, True):
        rows = torch.full((67, 36), float("nan"), device=dev())
        wr = ops.composite_forward_rows(*args, rows, fine, **kw).cpu().numpy()
        rows = rows.cpu().numpy()
        assert np.array_equal(rr.bits(wr), rr.bits(w))
        c0 = 17 if fine else 0
        assert np.array_equal(rr.bits(rows[:, c0:c0 + 15]), rr.bits(rgb))
        assert np.array_equal(rr.bits(rows[:, c0 + 15]), rr.bits(disp)) and np.array_equal(rr.bits(rows[:, c0 + 16]), rr.bits(acc))
        owned = np.zeros(36, bool)
        owned[c0:c0 + 17] = True
        if fine:
            assert np.array_equal(rr.bits(rows[:, 34]), rr.bits(w[:, -1])) and np.array_equal(rr.bits(rows[:, 35]), rr.bits(depth))
            owned[34:36] = True
        assert np.isnan(rows[:, ~owned]).all() and not np.isnan(rows[:, owned]).any()


def test_resample_every_branch_bit_exact(ops):
    cov = rr.Coverage()
    for S in rr.RESAMPLE_S:
        for nf in rr.RESAMPLE_NF:
            for rand_u in (False, True):
                z, w, u, fam = rr.resample_case(S, nf, rand_u)
                what = "S=%d nf=%d %s" % (S, nf, "rand" if rand_u else "det")
                zs, zo, inds = oracle.resample(z, w, nf, u=u)
                g_zo, g_zs, g_inds = ops.resample(T(z), T(w), nf, u=None if u is None else T(u), want_aux=True)
                assert np.array_equal(g_inds.cpu().numpy(), inds), what
                assert np.array_equal(g_zs.cpu().numpy(), zs), what
                assert np.array_equal(g_zo.cpu().numpy(), zo), what
                bins, wm = 0.5 * (z[:, 1:] + z[:, :-1]), np.ascontiguousarray(w[:, 1:-1])      # the plain sample_pdf_2 seam: nb = S - 1 < 256 bins
                s2, i2 = ops.sample_pdf(T(bins), T(wm), nf, u=None if u is None else T(u), want_inds=True)
                assert np.array_equal(i2.cpu().numpy(), inds) and np.array_equal(s2.cpu().numpy(), zs), what + " (seam)"
                cov.add(rr.branch_rows(w, oracle), fam, rr.torch_sample_pdf(bins, wm, nf, u)[2])
    assert not cov.missing(), cov.missing()


@pytest.mark.parametrize("S,nf", [(64, 64), (64, 63), (65, 64), (13, 7), (4, 4), (256, 256), (66, 128), (128, 5)])
def test_resample_merge_sort_and_permutation(ops, S, nf):
    """(S % 4 == 0) x (nf % 4 == 0) in every combination; only sorted rows of the first kind take the fast path, and they share their
    workgroups with unsorted, flat and tied rows."""
    z, w, u, kind = rr.merge_case(S, nf)
    z_sorted, z_new, src = (o.cpu().numpy() for o in ops.resample_merge(T(z), T(w), nf, u=T(u)))
    zs, zo, _ = oracle.resample(z, w, nf, u=u)
    assert np.array_equal(rr.bits(z_new), rr.bits(zs))
    v, tsrc = rr.torch_merge(z, z_new)
    assert np.array_equal(rr.bits(z_sorted), rr.bits(v)) and np.array_equal(rr.bits(z_sorted), rr.bits(zo))
    assert np.array_equal(np.sort(src, axis=1), np.broadcast_to(np.arange(S + nf), src.shape)), "src is not a permutation"
    assert np.array_equal(rr.bits(np.take_along_axis(np.concatenate([z, z_new], 1), src.astype(np.int64), 1)), rr.bits(z_sorted))
    ties = np.diff(z_sorted, axis=1) == 0
    assert ties[kind == 2].all() and ties[kind == 3].any()
    assert np.all(np.diff(src, axis=1)[ties] > 0), "equal values do not keep index order"
    assert np.array_equal(src, tsrc)                     # (what the four assertions above add up to: torch's stable argsort)


SENTINEL_Z = 0x7FC0BEEF          # a quiet NaN with a payload no arithmetic produces


@pytest.mark.parametrize("S,nf", [(64, 64), (13, 7)])
def test_resample_with_non_finite_weights(ops, S, nf):
    """A NaN or inf among a ray's coarse weights makes (some of) its new samples NaN.  The merge must still write every slot of z_out and
    src, with src a permutation, finite depths first in order and the NaNs last in index order -- torch.sort's order -- because the next
    launch gathers xw[ray, src] without a range check.  Stops at the resample stage: src is only read back.  Called through the C ABI with
    caller-made buffers prefilled with sentinels."""
    L, check = pkg("_lib").lib(), pkg("_lib").check
    N = 11
    rng = np.random.default_rng([S, nf])
    z = np.sort(rng.uniform(0.48, 1.08, (N, S)).astype(np.float32), axis=1)
    w = (rng.uniform(0, 1, (N, S)) ** 6).astype(np.float32)
    u = rng.uniform(0, 1, (N, nf)).astype(np.float32)
    w[1, S // 2] = np.nan                    # one NaN weight: the row sum is NaN, every new sample NaN
    w[2, S // 3] = np.inf                    # one inf: the quotients are 0 and one NaN, the cdf 0 ... 0 NaN ... NaN, and every draw lands on its first NaN knot
    w[5, :] = np.nan                         # a whole row
    w[6, 1] = np.inf                         # first pdf column: every knot NaN
    u[9, [0, nf // 2]] = np.nan              # and a row that MIXES finite and NaN samples (two NaN draws): the finite ones must keep their ranks
    bad = np.array([1, 2, 5, 6, 9])          # rays 0, 3 share their workgroup with bad rays; 4, 7 sit beside 5, 6; 8, 10 beside 9
    good = np.setdiff1d(np.arange(N), bad)
    zt, wt, ut = T(z), T(w), T(u)
    M = S + nf
    z_new = torch.from_numpy(np.full((N, nf), SENTINEL_Z, np.uint32).view(np.float32)).to(dev())
    z_out = torch.from_numpy(np.full((N, M), SENTINEL_Z, np.uint32).view(np.float32)).to(dev())
    src = torch.full((N, M), -1, dtype=torch.int32, device=dev())
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    check(L.sahs_resample_merge(N, S, nf, p(zt), p(wt), p(ut), p(z_new), p(z_out), p(src), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
          "sahs_resample_merge")
    torch.cuda.synchronize()
    z_new, z_out, src = z_new.cpu().numpy(), z_out.cpu().numpy(), src.cpu().numpy()
    nan_new = np.isnan(z_new)
    print("non-finite weights S=%d nf=%d: NaN samples per bad ray %s; unwritten z_out slots %d, unwritten src slots %d"
          % (S, nf, nan_new[bad].sum(1).tolist(), int((rr.bits(z_out) == SENTINEL_Z).sum()), int((src == -1).sum())))
    assert not (rr.bits(z_new) == SENTINEL_Z).any()
    assert nan_new[[1, 2, 5, 6]].all() and nan_new[9].sum() == 2 and not nan_new[good].any()
    zs, zo, _ = oracle.resample(z[good], w[good], nf, u=u[good])
    assert np.array_equal(rr.bits(z_new[good]), rr.bits(zs)) and np.array_equal(rr.bits(z_out[good]), rr.bits(zo))
    assert not (rr.bits(z_out) == SENTINEL_Z).any(), "z_out has slots the kernel never wrote"
    assert not (src == -1).any(), "src has slots the kernel never wrote"
    assert np.array_equal(np.sort(src, axis=1), np.broadcast_to(np.arange(M), src.shape)), "src is not a permutation"
    v, tsrc = rr.torch_merge(z, z_new)
    assert np.array_equal(rr.bits(z_out), rr.bits(v))                 # finite depths first, in order, then the NaNs ...
    assert np.array_equal(src, tsrc)                                   # ... in index order
    for r in bad:
        k = int(nan_new[r].sum())
        assert np.isnan(z_out[r, M - k:]).all() and not np.isnan(z_out[r, :M - k]).any() and np.all(np.diff(z_out[r, :M - k]) >= 0)
        assert np.all(np.diff(src[r, M - k:]) > 0) and np.all(src[r, M - k:] >= S)


def numpy_route(src, g_fine, Sc):
    N, Sf = src.shape
    nf = Sf - Sc
    g = g_fine.reshape(N, Sf, 8)
    both = np.full((N, Sf, 8), np.nan, np.float32)           # row src[r, s] of ray r <- row s of its sorted-order gradient
    np.put_along_axis(both, np.broadcast_to(src[:, :, None].astype(np.int64), g.shape), g, axis=1)
    return np.ascontiguousarray(both[:, :Sc]).reshape(N * Sc, 8), np.ascontiguousarray(both[:, Sc:]).reshape(N * nf, 8)


@pytest.mark.parametrize("N,Sc,nf", [(1, 1, 1), (5, 3, 5), (37, 64, 64), (130, 64, 128), (3, 128, 128), (17000, 64, 64)])
def test_route_xw_grad(ops, N, Sc, nf):
    """Random per-ray permutations and the ones resample_merge makes; N = 17000: 2 * N * (Sc + nf) float4 > 16384 * 256 threads, so the
    grid-stride loop runs."""
    rng = np.random.default_rng([N, Sc, nf])
    Sf = Sc + nf
    perms = [np.argsort(rng.uniform(size=(N, Sf)), axis=1).astype(np.int32)]
    if Sc >= 3:
        z = np.sort(rng.uniform(0.48, 1.08, (N, Sc)).astype(np.float32), axis=1)
        w = (rng.uniform(0, 1, (N, Sc)) ** 6).astype(np.float32)
        src = ops.resample_merge(T(z), T(w), nf, u=T(rng.uniform(0, 1, (N, nf)).astype(np.float32)))[2].cpu().numpy()
        assert np.array_equal(np.sort(src, axis=1), np.broadcast_to(np.arange(Sf), src.shape))
        perms.append(src)
    if N == 17000:
        assert N * Sf * 2 > 16384 * 256
    for src in perms:
        g = rng.standard_normal((N * Sf, 8)).astype(np.float32)
        g_c, g_n = ops.route_xw_grad(T(src), T(g), Sc)
        r_c, r_n = numpy_route(src, g, Sc)
        assert np.array_equal(rr.bits(g_c.cpu().numpy()), rr.bits(r_c)) and np.array_equal(rr.bits(g_n.cpu().numpy()), rr.bits(r_n))


def test_ray_stride_loops(ops):
    """More rays than one launch's workgroups hold (8192 workgroups x 4 rays): composite and resample walk the rest in a stride loop;
    the last 7 rays are held to the same bounds as the first 7."""
    N, S, nf = 4 * 8192 + 7, 8, 4
    case = rr.composite_case("thin", S, "prior", N=N, seed=5)
    r32, r64 = rr.composite_refs(case, oracle)
    outs = hip_composite(ops, case)
    for nm, o, a, b in zip(rr.OUTPUTS, outs, r32, r64):
        o = o.cpu().numpy()
        yardstick(o, a, b, "composite stride loop %s" % nm, scale_floor=1.0)
        yardstick(o[:7], a[:7], b[:7], "composite stride loop %s, first 7 rays" % nm, scale_floor=1.0)
        yardstick(o[-7:], a[-7:], b[-7:], "composite stride loop %s, last 7 rays" % nm, scale_floor=1.0)
    rng = np.random.default_rng(N)
    w = (rng.uniform(0, 1, (N, S)) ** 6).astype(np.float32)
    u = rng.uniform(0, 1, (N, nf)).astype(np.float32)
    zs, zo, inds = oracle.resample(case["z"], w, nf, u=u)
    g_zo, g_zs, g_inds = ops.resample(T(case["z"]), T(w), nf, u=T(u), want_aux=True)
    assert np.array_equal(g_inds.cpu().numpy(), inds) and np.array_equal(g_zs.cpu().numpy(), zs) and np.array_equal(g_zo.cpu().numpy(), zo)
    z_sorted, z_new, src = (o.cpu().numpy() for o in ops.resample_merge(T(case["z"]), T(w), nf, u=T(u)))
    assert np.array_equal(z_sorted, zo) and np.array_equal(z_new, zs)
    assert np.array_equal(src, rr.torch_merge(case["z"], zs)[1])


@pytest.mark.parametrize("lindisp", [False, True])
@pytest.mark.parametrize("perturb", [False, True])
@pytest.mark.parametrize("S,flat", [(3, False), (255, False), (256, False), (64, True), (1, True), (1, False)])
def test_stratified_depths_edges(ops, S, flat, lindisp, perturb):
    """train_utils.py:93-113 at S = 3 and at the largest sample counts, with near == far, and with one sample (lindisp included)."""
    rng = np.random.default_rng([S, int(flat), int(lindisp), int(perturb)])
    rays = np.zeros((33, 8), np.float32)
    rays[:, 6] = rng.uniform(0.2, 0.5, 33)
    rays[:, 7] = rays[:, 6] if flat else rng.uniform(0.8, 1.2, 33)
    t_rand = rng.uniform(0, 1, (33, S)).astype(np.float32) if perturb else None
    z = ops.stratified_depths(T(rays), S, lindisp, None if t_rand is None else T(t_rand))
    close(z, oracle.stratified_depths(rays[:, 6], rays[:, 7], S, lindisp, t_rand), 2e-7, 0.0, "depths")


@pytest.mark.parametrize("N,S,ray0", [(1, 1, 0), (67, 5, 3), (1000, 64, 2 ** 33 + 1), (3, 256, 0)])
def test_ray_uniforms_range(ops, N, S, ray0):
    """Draws are 24-bit uniforms in [0, 1) -- never 1 -- and the oracle's, bit for bit, also where S is not a multiple of the four
    words of a Philox block and where the global ray index needs its high word."""
    u = ops.ray_uniforms(1234567, 2, ray0, N, S, dev()).cpu().numpy()
    assert u.min() >= 0.0 and u.max() < 1.0 and u.max() <= np.float32(rr.U_LAST)
    assert np.array_equal(u, oracle.ray_uniforms(1234567, 2, ray0, N, S))
    assert np.array_equal(u * 2.0 ** 24, np.round(u * 2.0 ** 24))
