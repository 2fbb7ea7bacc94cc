"""The sparse instances of the fp32 field kernel (csrc/field_f32.hip: FIELD_ALL_TRUNK / FIELD_RADIANCE_TRUNK / FIELD_BRANCH) at the shapes
where work carried from one tile of a persistent workgroup to the next could go wrong: workgroups that run several tiles and end in a ragged
one, exactly one tile (or one sample) more than there are workgroups, record counts of 128 k and 128 k + 1, slabs of several tiles per
workgroup, and the 4-layer trunks of the NeRFaceModels.  tests/test_gpu_sparse_branches.py stops at 300 rays -- at most 450 tiles, under
two per workgroup on a 256-CU device.  Everything is compared bit for bit against the dense launches (ops.sparse_branches(False)) with that
file's recipe (copied, not imported: test files stay independent).

Tiles per workgroup: a launch over T tiles of 128 samples starts min(T, CUs) workgroups and workgroup g runs tiles g, g + CUs, ...; the
least any of them runs is T // CUs (when T >= CUs), the most ceil(T / CUs)."""
import pytest
import torch

from conftest import pkg

pytestmark = pytest.mark.gpu

NC = 64
TILE = 128
_CACHE = {}
CENTRED_BIAS = {"nerface": -17.1422, "nerface_static": 16.4984}      # (tests/test_gpu_sparse_branches.py: 2.0 minus the median dense sigma)


def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def cus():
    return torch.cuda.get_device_properties(dev()).multi_processor_count


def tiles(samples):
    return (samples + TILE - 1) // TILE


def setup(arch, density_bias):
    key = (arch, float(density_bias))
    if key not in _CACHE:
        ops, W = pkg("ops"), pkg("weights")
        d = dev()
        flat = torch.from_numpy(W.flatten_state_dict(W.hash_state_dict(0, density_bias, 30.0, model=arch, hdr=True), model=arch)).to(d)
        g = torch.Generator(device=d).manual_seed(5)
        drv = torch.randn(16, 29, device=d, generator=g) if arch == "audio" else torch.randn(76, device=d, generator=g) * 0.5
        cam = 0.8 if arch == "audio" else 0.5
        pose = torch.tensor([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, cam]], device=d)
        _CACHE[key] = (ops.pack_weights(flat, ops.SAHS_F32, arch=arch), ops.fold_conditioning(flat, drv, pose, arch=arch))
    return _CACHE[key]


def default_bias(arch):
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
    packed, frame = setup(arch, default_bias(arch) if density_bias is None else density_bias)
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
    sg = raw[..., 15] + (noise if noise is not None else 0.0)
    live = sg > 0.0
    live[:, -1] = not with_bg
    return live


def compare(dense, sparse, noise, with_bg, what, one_slab=True):
    for a, b, nm in zip(dense[:3], sparse[:3], ("rows", "z_fine", "weights")):
        assert torch.equal(a, b), "%s: %s differs (max %.3e)" % (what, nm, float((a - b).abs().max()))
    rd, rs = dense[3], sparse[3]
    live = live_mask(rd, noise, with_bg)
    assert torch.equal(rd[live], rs[live]), what + ": raw rows of live samples differ"
    assert torch.equal(rd[..., 15], rs[..., 15]), what + ": sigma differs"
    assert bool(torch.isfinite(rs).all()), what + ": raw is not finite"
    if one_slab:
        assert sparse[4] == int(live.sum()), what + ": %d records, %d live samples" % (sparse[4], int(live.sum()))
    return live


def check_steady(arch, N, nf, share, noise_std, what):
    rays, kw = scene(arch, N, nf, noise_std=noise_std)
    dense, sparse = render(arch, rays, nf, kw, False, share), render(arch, rays, nf, kw, True, share)
    live = compare(dense, sparse, kw.get("noise_f"), True, what)
    dead = 1.0 - float(live.float().mean())
    t_fine, t_branch = tiles(N * (NC + nf)), tiles(sparse[4])
    print("%s: dead %.3f, fine trunk %d tiles (every workgroup >= %d), branch launch %d tiles (busiest workgroup %d), %d CUs"
          % (what, dead, t_fine, t_fine // cus(), t_branch, -(-t_branch // cus()), cus()))
    assert 0.2 <= dead <= 0.8, "the dense raw has %.1f %% dead samples: the comparison would be vacuous" % (100 * dead)
    assert t_fine // cus() >= 3, "every workgroup of the fine trunk should run at least 3 tiles (%d tiles, %d CUs)" % (t_fine, cus())
    assert -(-t_branch // cus()) >= 2, "a workgroup of the branch launch should run at least 2 tiles (%d tiles, %d CUs)" % (t_branch, cus())


@pytest.mark.parametrize("nf,share,noise_std", [(64, True, 0.0), (64, False, 0.0), (128, True, 0.0), (128, False, 5.0)])
def test_steady_state(nf, share, noise_std):
    """1031 rays: 1,031 / 1,547 fine-trunk tiles (192 samples per ray are no whole number of tiles: a ragged last one) and 516 coarse ones"""
    check_steady("audio", 1031, nf, share, noise_std, "audio N=1031 nf=%d share=%s noise=%g" % (nf, share, noise_std))


@pytest.mark.parametrize("arch", ["nerface", "nerface_static"])
def test_steady_state_nerface(arch):
    """the 4-layer trunk: no rolled layer loop, another count of weight chunks per tile"""
    check_steady(arch, 1031, 64, arch == "nerface", 0.0, "%s N=1031 nf=64" % arch)


def test_one_sample_past_the_workgroups():
    """CUs x 128 + 1 samples in the fine pass: one workgroup has a second tile, and that tile holds one sample.  The samples per ray
    64 + nf are chosen so that they divide that count (256 CUs: 331 rays of 64 + 35)."""
    target = cus() * TILE + 1
    nf = next((f for f in range(1, 129) if target % (NC + f) == 0), None)
    assert nf is not None, "no 64 + nf divides %d" % target
    N = target // (NC + nf)
    for share in (True, False):
        rays, kw = scene("audio", N, nf)
        dense, sparse = render("audio", rays, nf, kw, False, share), render("audio", rays, nf, kw, True, share)
        compare(dense, sparse, None, True, "N=%d nf=%d (%d samples) share=%s" % (N, nf, target, share))
    assert tiles(N * (NC + nf)) == cus() + 1 and N * (NC + nf) % TILE == 1


def test_one_tile_past_the_workgroups():
    """(CUs + 1) whole tiles in the fine pass"""
    N = cus() + 1
    rays, kw = scene("audio", N, 64)
    dense, sparse = render("audio", rays, 64, kw, False), render("audio", rays, 64, kw, True)
    compare(dense, sparse, None, True, "N=%d nf=64" % N)
    assert N * (NC + 64) == (cus() + 1) * TILE


@pytest.mark.parametrize("extra", [0, 1])
def test_record_counts_at_a_tile_edge(extra):
    """density bias +1e4 and a background prior: every sample but a ray's last is live, 127 records per ray in the fine pass.  127 N is a
    multiple of 128 for N = 128 m and one more than a multiple for N = 128 m - 1; m = 3 puts the branch launch past one tile per workgroup
    on 256 CUs (381 tiles, or 380 and a tile of one record)."""
    N = 384 - extra
    rays, kw = scene("audio", N, 64)
    dense = render("audio", rays, 64, kw, False, density_bias=1e4)
    sparse = render("audio", rays, 64, kw, True, density_bias=1e4)
    compare(dense, sparse, None, True, "bias 1e4 N=%d" % N)
    assert sparse[4] == 127 * N and sparse[4] % TILE == extra


def test_two_slabs_of_several_tiles():
    """record workspace of 774 tiles against the fine pass's 1,547: two slabs of 516 and 515 rays (the second ends in half a tile), three
    tiles per workgroup each on 256 CUs; noise on.  Equal to the one-slab render and to the dense one."""
    ops, lib = pkg("ops"), pkg("_lib")
    N, nf = 1031, 128
    rays, kw = scene("audio", N, nf, noise_std=5.0)
    dense, one = render("audio", rays, nf, kw, False), render("audio", rays, nf, kw, True)
    cap = tiles(N * (NC + nf)) // 2 * TILE + TILE
    was = ops.sparse_workspace_bytes()
    try:
        ops.sparse_branches(workspace_bytes=int(lib.lib().sahs_model_render_sparse_workspace_bytes(0, cap)))
        two = render("audio", rays, nf, kw, True)
    finally:
        ops.sparse_branches(workspace_bytes=was)
    for a, b, nm in zip(one[:4], two[:4], ("rows", "z_fine", "weights", "raw")):
        assert torch.equal(a, b), nm
    live = compare(dense, two, kw["noise_f"], True, "two slabs", one_slab=False)
    per = cap // (NC + nf)
    assert per < N <= 2 * per, "the workspace should make two slabs"
    step = (N + 1) // 2
    assert two[4] == int(live[step:].sum()), "the second slab's records are the live samples of its rays"
    assert tiles(step * (NC + nf)) // cus() >= 3 or cus() > 256
