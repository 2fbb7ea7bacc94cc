"""Sparse branches of the fp32 inference render (include/sahs_nerf.h: sahs_model_render_rays_rows_sparse; csrc/field_f32.hip:
FIELD_ALL_TRUNK / FIELD_RADIANCE_TRUNK / FIELD_BRANCH): the colour and seg branches run only for the samples the composite can give a
non-zero weight.  Everything is compared bit for bit against the dense launches (ops.sparse_branches(False)): the 36 outputs per ray,
the depths, the weights and the raw rows of the live samples; a zero-weight sample keeps its sigma and finite columns 0..14."""
import pytest
import torch

from conftest import pkg

pytestmark = pytest.mark.gpu

NC = 64
_CACHE = {}


def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def setup(arch, density_bias=2.0):
    """packed fp32 weights and the folded frame of hash_state_dict(0, density_bias, 30.0, hdr=True), once per (arch, bias)"""
    key = (arch, float(density_bias))
    if key not in _CACHE:
        ops, W = pkg("ops"), pkg("weights")
        d = dev()
        flat = torch.from_numpy(W.flatten_state_dict(W.hash_state_dict(0, density_bias, 30.0, model=arch, hdr=True), model=arch)).to(d)
        g = torch.Generator(device=d).manual_seed(5)
        drv = torch.randn(16, 29, device=d, generator=g) if arch == "audio" else torch.randn(76, device=d, generator=g) * 0.5
        cam = 0.8 if arch == "audio" else 0.5
        pose = torch.tensor([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, cam]], device=d)
        _CACHE[key] = (ops.pack_weights(flat, ops.SAHS_F32, arch=arch), ops.fold_conditioning(flat, drv, pose, arch=arch), cam)
    return _CACHE[key]


# density_bias of the NeRFaceModels' cases: 2.0 minus the median sigma of the dense fine pass (selector off: the launches as they were before
# the sparse branches existed) of scene(arch, 129, 64) with density_bias 2.0, measured once on MI355X: 19.1422 and -14.4984
CENTRED_BIAS = {"nerface": -17.1422, "nerface_static": 16.4984}


def default_bias(arch):
    """density_bias of a case.  AudioFaceModel: 2.0 -- hash_state_dict(0, 2.0, 30.0, hdr=True) centres that model's density logit, so 35-65 %
    of its samples are dead.  The NeRFaceModels' synthetic weights are not centred (weights.py does it for the audio model only): with 2.0
    every sigma is positive and only the last sample of a ray is dead (1.6 % measured), so a dense-against-sparse comparison would compare
    the dense path with itself.  sigma is affine in fc_alpha.bias, so for them the bias is moved by the median sigma of a dense render
    (CENTRED_BIAS): the same weights otherwise (seed 0, gain 30, hdr), and the same 20-80 % assertion on the dead fraction as for the audio
    model."""
    return 2.0 if arch == "audio" else CENTRED_BIAS[arch]


def scene(arch, N, nf, noise_std=0.0, with_bg=True):
    d = dev()
    cam = 0.8 if arch == "audio" else 0.5
    g = torch.Generator(device=d).manual_seed(1000 * N + nf)
    near, far = (0.483771, 1.083771) if arch == "audio" else (0.2, 0.8)
    rays = torch.zeros(N, 8, device=d)
    rays[:, 2] = cam
    rays[:, 3:6] = torch.randn(N, 3, device=d, generator=g) * 0.15 + torch.tensor([0, 0, -1.0], device=d)
    rays[:, 6], rays[:, 7] = near, far
    kw = dict(t_rand=torch.rand(N, NC, device=d, generator=g), u=torch.rand(N, nf, device=d, generator=g))
    if with_bg:
        kw["bg"] = torch.cat([torch.rand(N, 3, device=d, generator=g), torch.ones(N, 1, device=d), torch.zeros(N, 11, device=d)], 1)
    if noise_std > 0.0:
        kw["noise_c"] = torch.randn(N, NC, device=d, generator=g) * noise_std
        kw["noise_f"] = torch.randn(N, NC + nf, device=d, generator=g) * noise_std
    return rays, kw


def render(arch, rays, nf, kw, sparse, share=True, density_bias=None):
    """-> rows, z_f, weights, raw of the fine pass, live records of the fine pass's last slab (sparse only)"""
    ops = pkg("ops")
    packed, frame, _ = setup(arch, default_bias(arch) if density_bias is None else density_bias)
    rows = torch.full((rays.shape[0], 36), float("nan"), device=rays.device)
    ws = {}
    was = ops.sparse_branches()
    ops.sparse_branches(sparse)
    try:
        ops.render_rays_rows(packed, frame, rays, NC, nf, rows, workspace=ws, arch=arch, share_deformation=share, **kw)
    finally:
        ops.sparse_branches(was)
    assert ("sparse" in ws) == sparse
    return rows, ws["z_f"].clone(), ws["weights"].clone(), ws["raw"].clone(), (ops.sparse_last_count(ws) if sparse else None)


def live_mask(raw, noise, with_bg):
    """the samples whose colour and seg logits the composite can use (render_ops.hip: sg = max(sigma + noise, 0); the last sample always has
    a weight, but a background prior replaces its channels)"""
    sg = raw[..., 15] + (noise if noise is not None else 0.0)
    live = sg > 0.0
    live[:, -1] = not with_bg
    return live


def compare(dense, sparse, noise, with_bg, what):
    for a, b, nm in zip(dense[:3], sparse[:3], ("rows", "z_fine", "weights")):
        assert torch.equal(a, b), "%s: %s differs (max %.3e)" % (what, nm, float((a - b).abs().max()))
    rd, rs = dense[3], sparse[3]
    live = live_mask(rd, noise, with_bg)
    assert torch.equal(rd[live], rs[live]), what + ": raw rows of live samples differ"
    assert torch.equal(rd[..., 15], rs[..., 15]), what + ": sigma differs"
    assert bool(torch.isfinite(rs).all()), what + ": raw is not finite"
    assert sparse[4] is None or sparse[4] <= int(live.sum())      # (equal when the pass was one slab)
    return live


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
    """nothing live (the branch launch runs zero tiles), one sample per ray, everything live; live counts that are no multiple of 16 or of
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


@pytest.mark.parametrize("share,tiles", [(True, 3), (False, 3), (True, 5)])
def test_slabs(share, tiles):
    """A record workspace of 3 (5) x 128 slots and 301 rays: the fine pass (192 samples per ray) runs in 151 (101) slabs of 2 (3) rays and
    the coarse pass (64 per ray) in 51 (31) slabs of 6 (10), each with a ragged last slab of one ray -- 192 or 64 samples, no whole number
    of 128-sample tiles -- so the slab offsets into rays, depths, raw, xw, src and the noise are exercised (noise on, both chains).  The
    result equals the one-slab result and, as everywhere, the dense render."""
    ops, lib = pkg("ops"), pkg("_lib")
    rays, kw = scene("audio", 301, 128, noise_std=5.0)
    dense, one = render("audio", rays, 128, kw, False, share), render("audio", rays, 128, kw, True, share)
    was = ops.sparse_workspace_bytes()
    try:
        ops.sparse_branches(workspace_bytes=int(lib.lib().sahs_model_render_sparse_workspace_bytes(0, tiles * 128)))
        many = render("audio", rays, 128, kw, True, share)
    finally:
        ops.sparse_branches(workspace_bytes=was)
    for a, b, nm in zip(one[:4], many[:4], ("rows", "z_fine", "weights", "raw")):
        assert torch.equal(a, b), nm
    live = compare(dense, many, kw["noise_f"], True, "%d-tile slabs" % tiles)
    assert one[4] == int(live.sum()) and 0 < many[4] <= 192      # (many: the last slab is one ray)


def test_workspace_refusals():
    """less than one tile of records, or less than one ray's samples, is refused with a message; the selector is validated"""
    ops, lib = pkg("ops"), pkg("_lib")
    rays, kw = scene("audio", 7, 128)
    was = ops.sparse_workspace_bytes()
    try:
        ops.sparse_branches(workspace_bytes=int(lib.lib().sahs_model_render_sparse_workspace_bytes(0, 128)) - 1)
        with pytest.raises(lib.SahsError, match="less than one tile"):
            render("audio", rays, 128, kw, True)
        ops.sparse_branches(workspace_bytes=int(lib.lib().sahs_model_render_sparse_workspace_bytes(0, 128)))      # one tile, but a ray has 192 samples
        with pytest.raises(lib.SahsError, match="one ray has 192 samples"):
            render("audio", rays, 128, kw, True)
    finally:
        ops.sparse_branches(workspace_bytes=was)
    with pytest.raises(lib.SahsError):
        ops.sparse_branches("yes")
    with pytest.raises(lib.SahsError):
        ops.sparse_branches(workspace_bytes=0)


def test_two_sparse_runs_are_equal():
    """the slot a record lands in depends on the order of the waves' atomics; the outputs do not"""
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
