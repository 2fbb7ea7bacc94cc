"""Sparse branches of the fp32 inference render (include/sahs_nerf.h: sahs_model_render_rays_rows_sparse; csrc/field_f32.hip:
FIELD_ALL_FUSED for the coarse pass and the plain chain's fine pass, FIELD_RADIANCE_FUSED for the shared-deformation fine pass): the
colour and seg branches run only for the samples the composite can give a non-zero weight.  Everything is compared bit for bit against
the dense launches (ops.sparse_branches(False)) with the recipe of tests/sparse_reference.py: the 36 outputs per ray, the depths, the
weights and the raw rows of the live samples; a zero-weight sample keeps its sigma and finite columns 0..14; the live count is exact.
Small passes: up to 300 rays, at most 450 tiles -- under two per workgroup on a 256-CU device."""
import pytest
import torch

from conftest import pkg
from sparse_reference import NC, compare, live_mask, render, scene, setup

pytestmark = pytest.mark.gpu


CASES = [(a, n, f, s) for a in ("audio", "nerface", "nerface_static") for n in (1, 7, 129, 300) for f in (64, 128) for s in (False, True)
         if not (a == "nerface_static" and s)]


@pytest.mark.parametrize("arch,N,nf,share", CASES)
def test_rows_dense_against_sparse(arch, N, nf, share):
    rays, kw = scene(arch, N, nf)
    dense, sparse = render(arch, rays, nf, kw, False, share), render(arch, rays, nf, kw, True, share)
    live = compare(dense, sparse, None, True, "%s N=%d nf=%d share=%s" % (arch, N, nf, share))
    dead = 1.0 - float(live.float().mean())
    print("dead fraction %s N=%d nf=%d: %.3f, live records %d" % (arch, N, nf, dead, sparse[4]))
    assert sparse[4] == int(live.sum())
    assert 0.2 <= dead <= 0.8, "the dense raw has %.1f %% dead samples: the comparison would be vacuous" % (100 * dead)


@pytest.mark.parametrize("density_bias,with_bg,N,per_ray", [(-1e4, True, 129, 0), (-1e4, False, 7, 1), (-1e4, False, 129, 1),
                                                           (1e4, True, 129, NC + 64 - 1), (1e4, False, 7, NC + 64)])
def test_live_count_edges(density_bias, with_bg, N, per_ray):
    """nothing live (no branch pass, nothing to drain), one sample per ray, everything live; live counts that are no multiple of 16 or of
    128 (7, 129, 129 * 127) and one that is (7 * 128)"""
    rays, kw = scene("audio", N, 64, with_bg=with_bg)
    dense = render("audio", rays, 64, kw, False, density_bias=density_bias)
    sparse = render("audio", rays, 64, kw, True, density_bias=density_bias)
    compare(dense, sparse, None, with_bg, "bias %g bg %s" % (density_bias, with_bg))
    assert sparse[4] == N * per_ray


@pytest.mark.parametrize("arch,share", [("audio", True), ("audio", False), ("nerface_static", False)])
def test_noise_flips_liveness(arch, share):
    rays, kw = scene(arch, 129, 64, noise_std=5.0)
    dense, sparse = render(arch, rays, 64, kw, False, share), render(arch, rays, 64, kw, True, share)
    live = compare(dense, sparse, kw["noise_f"], True, arch + " with noise")
    flipped = live != live_mask(dense[3], None, True)
    assert float(flipped.float().mean()) > 0.05, "the noise should decide the liveness of many samples"
    assert sparse[4] == int(live.sum())


def test_workspace_refusals():
    """a record workspace one byte short of the fine pass's rings is refused with a message, before anything is launched: the rows, the
    depths and the workspace's head stay as they were; the selector is validated"""
    ops, lib = pkg("ops"), pkg("_lib")
    L = lib.lib()
    rays, kw = scene("audio", 7, 128)
    ws = {}
    render("audio", rays, 128, kw, True, ws=ws)
    packed, frame = setup("audio", 2.0)
    need = int(L.sahs_model_render_sparse_fused_workspace_bytes(0, 7 * (NC + 128)))
    assert ws["sparse"].numel() == need
    p = lambda t: None if t is None else t.data_ptr()
    rows = torch.full((7, 36), float("nan"), device=rays.device)
    ws["z_c"].fill_(-1.0)
    ws["sparse"][:8] = 7
    torch.cuda.synchronize()
    code = L.sahs_model_render_rays_rows_sparse(0, p(packed), p(frame), ops.SAHS_F32, 7, p(rays), 8, NC, 128, 0, 0, p(kw["bg"]), p(kw["t_rand"]), None,
                                                p(kw["u"]), None, p(ws["z_c"]), p(ws["z_f"]), p(ws["raw"]), p(ws["weights"]), p(rows), 36, p(ws["xw"]),
                                                p(ws["src"]), p(ws["z_new"]), p(ws["sparse"]), need - 1, None)
    torch.cuda.synchronize()
    assert code == 5 and b"sahs_model_render_sparse_fused_workspace_bytes" in L.sahs_last_error()
    assert bool(torch.isnan(rows).all()) and bool((ws["z_c"] == -1.0).all()) and bool((ws["sparse"][:8] == 7).all())
    with pytest.raises(lib.SahsError):
        ops.sparse_branches("yes")
    with pytest.raises(TypeError):
        ops.sparse_branches(workspace_bytes=0)


def test_two_sparse_runs_are_equal():
    """two renders of one scene, each through a fresh workspace: the same rows, depths, weights, raw and live count"""
    rays, kw = scene("audio", 300, 64, noise_std=5.0)
    a, b = render("audio", rays, 64, kw, True), render("audio", rays, 64, kw, True)
    for x, y, nm in zip(a[:4], b[:4], ("rows", "z_fine", "weights", "raw")):
        assert torch.equal(x, y), nm
    assert a[4] == b[4]


@pytest.mark.parametrize("arch,share", [("audio", True), ("audio", False), ("nerface_static", False)])
def test_probe_records_are_the_dense_ones(arch, share):
    ops = pkg("ops")
    rays, kw = scene(arch, 129, 64)
    recs = {}
    for sparse in (False, True):
        with ops.LaunchProbe(capacity=64) as probe:
            render(arch, rays, 64, kw, sparse, share)
            recs[sparse] = [(r["model"], r["level"], r["part"], r["precision"], r["samples"]) for r in probe.records()]
    assert recs[False] == recs[True] and len(recs[True]) == (3 if share else 2)
