"""The fused sparse instances of the fp32 field kernel (csrc/field_f32.hip: FIELD_ALL_FUSED / FIELD_RADIANCE_FUSED): one launch per pass, every
persistent workgroup appending its live samples to a private record ring and running the branch layers itself whenever the ring held a
tile's worth when a tile started, then draining the ring.  Everything is compared bit for bit against the dense launches
(ops.sparse_branches(False)) with the recipe of tests/test_gpu_sparse_pipeline.py (copied, not imported: test files stay independent), at
64 coarse + 64 fine samples -- one fine tile of 128 samples per ray -- so that with C compute units a pass over N rays gives workgroup g
the tiles g, g + C, ...: N = 3 C + 1 is three tiles for every workgroup and a fourth for one.

What can go wrong is in the ring: the slot arithmetic across its end, the carried count (a branch pass at every tile when everything is
live, none before the drain when little is), the partial last drain pass, records of the previous tile read by another wave, and the
count and path words of the workspace head."""
import pytest
import torch

from conftest import pkg

pytestmark = pytest.mark.gpu

NC = 64
NF = 64
TILE = 128
_CACHE = {}
CENTRED_BIAS = {"nerface": -17.1422, "nerface_static": 16.4984}      # (tests/test_gpu_sparse_branches.py: 2.0 minus the median dense sigma)
# density bias of the drain-only case: chosen on the first run so that the fine pass of 3 C + 1 rays has fewer than 128 live records per
# workgroup, i.e. under a third of its samples live (256 CUs, 98,432 samples: bias -2 gave 32.3 % live, -4 22.3 %, -6 14.7 % = 14,517 records
# against the 32,768 allowed, -8 9.0 %)
DRAIN_ONLY_BIAS = -6.0


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


def scene(arch, N, nf, noise_std=0.0, with_bg=True, nc=NC):
    d = dev()
    cam = 0.8 if arch == "audio" else 0.5
    g = torch.Generator(device=d).manual_seed(1000 * N + nf)
    near, far = (0.483771, 1.083771) if arch == "audio" else (0.2, 0.8)
    rays = torch.zeros(N, 8, device=d)
    rays[:, 2] = cam
    rays[:, 3:6] = torch.randn(N, 3, device=d, generator=g) * 0.15 + torch.tensor([0, 0, -1.0], device=d)
    rays[:, 6], rays[:, 7] = near, far
    kw = dict(t_rand=torch.rand(N, nc, device=d, generator=g))
    if nf > 0:
        kw["u"] = torch.rand(N, nf, device=d, generator=g)
    if with_bg:
        kw["bg"] = torch.cat([torch.rand(N, 3, device=d, generator=g), torch.ones(N, 1, device=d), torch.zeros(N, 11, device=d)], 1)
    if noise_std > 0.0:
        kw["noise_c"] = torch.randn(N, nc, device=d, generator=g) * noise_std
        if nf > 0:
            kw["noise_f"] = torch.randn(N, nc + nf, device=d, generator=g) * noise_std
    return rays, kw


def render(arch, rays, nf, kw, sparse, share=True, density_bias=None, nc=NC, ws=None):
    """-> rows, depths, weights, raw of the last pass, live count of the last pass and the path it took (sparse only)"""
    ops = pkg("ops")
    packed, frame = setup(arch, default_bias(arch) if density_bias is None else density_bias)
    rows = torch.full((rays.shape[0], 36), float("nan"), device=rays.device)
    ws = {} if ws is None else ws
    was = ops.sparse_branches()
    ops.sparse_branches(sparse)
    try:
        ops.render_rays_rows(packed, frame, rays, nc, nf, rows, workspace=ws, arch=arch, share_deformation=share, **kw)
    finally:
        ops.sparse_branches(was)
    assert ("sparse" in ws) == sparse
    if nf == 0:      # (no fine pass: columns 17..33, rgb_f / disp_f / acc_f, are not written and keep their NaN)
        rows = torch.cat([rows[:, :17], rows[:, 34:]], 1)
    assert bool(torch.isfinite(rows).all()), "a rendered row holds a value that was not written"
    z = ws["z_f"] if nf > 0 else ws["z_c"]
    S = nc + nf
    # (without a fine pass the raw and weights workspaces are the coarse pass's: the first nc columns' worth of the flat buffers)
    raw = ws["raw"].reshape(-1)[:rays.shape[0] * S * 16].reshape(rays.shape[0], S, 16)
    wts = ws["weights"].reshape(-1)[:rays.shape[0] * S].reshape(rays.shape[0], S)
    return (rows, z.clone(), wts.clone(), raw.clone(), (ops.sparse_last_count(ws) if sparse else None),
            (ops.sparse_last_path(ws) if sparse else None))


def live_mask(raw, noise, with_bg):
    sg = raw[..., 15] + (noise if noise is not None else 0.0)
    live = sg > 0.0
    live[:, -1] = not with_bg
    return live


def compare(dense, sparse, noise, with_bg, what, fused=True):
    """rows, depths, weights; raw of the live samples; sigma of all samples; the count; the path -> live mask"""
    for a, b, nm in zip(dense[:3], sparse[:3], ("rows", "depths", "weights")):
        assert torch.equal(a, b), "%s: %s differs (max %.3e)" % (what, nm, float((a - b).abs().max()))
    rd, rs = dense[3], sparse[3]
    live = live_mask(rd, noise, with_bg)
    assert torch.equal(rd[live], rs[live]), what + ": raw rows of live samples differ"
    assert torch.equal(rd[..., 15], rs[..., 15]), what + ": sigma differs"
    assert bool(torch.isfinite(rs).all()), what + ": raw is not finite"
    assert sparse[5] == (1 if fused else 0), what + ": the pass ran %s" % ("slabs" if fused else "fused")
    if fused:
        assert sparse[4] == int(live.sum()), what + ": %d records, %d live samples" % (sparse[4], int(live.sum()))
    return live


def report(what, live, samples):
    """the figures of a case: dead fraction, tiles of the last pass per workgroup, live records per workgroup"""
    t, c = tiles(samples), cus()
    dead = 1.0 - float(live.float().mean())
    print("%s: dead %.3f, %d live records, %d tiles on %d CUs (per workgroup %d..%d), %.1f records per workgroup"
          % (what, dead, int(live.sum()), t, c, t // c if t >= c else 0, -(-t // c), float(live.sum()) / min(t, c)))
    return dead


def check(arch, N, nf, what, share=True, noise_std=0.0, with_bg=True, density_bias=None, nc=NC):
    rays, kw = scene(arch, N, nf, noise_std=noise_std, with_bg=with_bg, nc=nc)
    dense = render(arch, rays, nf, kw, False, share, density_bias, nc)
    sparse = render(arch, rays, nf, kw, True, share, density_bias, nc)
    live = compare(dense, sparse, kw.get("noise_f" if nf > 0 else "noise_c"), with_bg, what)
    return live, report(what, live, N * (nc + nf)), dense, sparse


def test_one_tile_alone():
    """the smallest pass: one ray, one fine tile, one workgroup -- append, no branch pass in the tile, one partial drain pass"""
    live, _, _, _ = check("audio", 1, NF, "audio N=1")
    assert 0 < int(live.sum()) < TILE


def test_steady_state():
    """3 C + 1 rays: every workgroup runs at least 3 fine tiles"""
    N = 3 * cus() + 1
    _, dead, _, _ = check("audio", N, NF, "audio N=%d steady" % N)
    assert 0.2 <= dead <= 0.8, "the dense raw has %.1f %% dead samples: the comparison would be vacuous" % (100 * dead)
    assert tiles(N * (NC + NF)) // cus() >= 3


def test_full_ring():
    """every sample live (density bias 1e4, no background prior): from its second tile on a workgroup runs a branch pass at every tile, and
    every workgroup holds 256 records at once"""
    N = 2 * cus() + 1
    live, _, _, sparse = check("audio", N, NF, "audio N=%d all live" % N, with_bg=False, density_bias=1e4)
    assert sparse[4] == N * (NC + NF) and bool(live.all())
    N = 6 * cus() + 1      # (and often enough for the ring of 512 slots to come round its end)
    live, _, _, sparse = check("audio", N, NF, "audio N=%d all live" % N, with_bg=False, density_bias=1e4)
    assert sparse[4] == N * (NC + NF)


def test_nothing_live():
    """density bias -1e4 with the background prior: no record, the drain runs over nothing, and columns 0..14 of every raw row hold the
    output biases (the FINAL tile as fc_alpha leaves it), the same row for every sample"""
    N = 2 * cus() + 1
    live, _, _, sparse = check("audio", N, NF, "audio N=%d nothing live" % N, density_bias=-1e4)
    assert sparse[4] == 0 and not bool(live.any())
    raw = sparse[3]
    assert torch.equal(raw[..., :15], raw[0, 0, :15].expand_as(raw[..., :15]))


def test_drain_only():
    """fewer live records than 128 per workgroup: at least one workgroup of three or four tiles never fills a branch pass and reaches its
    records only in a partial drain pass"""
    N = 3 * cus() + 1
    live, _, _, _ = check("audio", N, NF, "audio N=%d bias %g" % (N, DRAIN_ONLY_BIAS), density_bias=DRAIN_ONLY_BIAS)
    assert 0 < int(live.sum()) < TILE * cus(), "%d live records, %d workgroups" % (int(live.sum()), cus())


def test_one_tile_past_the_workgroups():
    """C + 1 whole fine tiles: one workgroup runs two, the rest one (rings of 256 and of 128 slots)"""
    N = cus() + 1
    check("audio", N, NF, "audio N=%d" % N)


def test_one_sample_past_the_workgroups():
    """C x 128 + 1 coarse samples, no fine pass: the last tile holds one sample.  The samples per ray are a divisor of that count (256 CUs:
    331 rays of 99)."""
    target = cus() * TILE + 1
    nc = next((s for s in range(256, 1, -1) if target % s == 0), None)
    assert nc is not None, "no sample count up to 256 divides %d" % target
    N = target // nc
    check("audio", N, 0, "audio N=%d nc=%d nf=0 (%d samples)" % (N, nc, target), nc=nc)
    assert tiles(N * nc) == cus() + 1 and N * nc % TILE == 1


@pytest.mark.parametrize("nf,share,noise_std,with_bg", [(0, True, 0.0, True), (NF, False, 0.0, True), (NF, True, 1.0, True), (NF, True, 0.0, False),
                                                        (NF, False, 1.0, False)])
def test_modes(nf, share, noise_std, with_bg):
    """coarse pass only (FIELD_ALL_FUSED alone); the plain chain (fine pass through FIELD_ALL_FUSED); noise; no background prior"""
    N = 3 * cus() + 1
    check("audio", N, nf, "audio N=%d nf=%d share=%s noise=%g bg=%s" % (N, nf, share, noise_std, with_bg), share=share, noise_std=noise_std,
          with_bg=with_bg)


@pytest.mark.parametrize("arch", ["nerface", "nerface_static"])
def test_nerface(arch):
    """the 4-layer trunks: another count of weight chunks per tile, no rolled layer loop"""
    N = 3 * cus() + 1
    _, dead, _, _ = check(arch, N, NF, "%s N=%d" % (arch, N), share=arch == "nerface")
    assert 0.2 <= dead <= 0.8, "the dense raw has %.1f %% dead samples: the comparison would be vacuous" % (100 * dead)


def test_workspace_reuse():
    """the same workspace twice, then a smaller scene through it: neither stale ring contents nor the count leak"""
    N = 3 * cus() + 1
    rays, kw = scene("audio", N, NF)
    dense = render("audio", rays, NF, kw, False)
    ws = {}
    first = render("audio", rays, NF, kw, True, ws=ws)
    ring = ws["sparse"]
    second = render("audio", rays, NF, kw, True, ws=ws)
    assert ws["sparse"] is ring
    for s in (first, second):
        compare(dense, s, None, True, "N=%d through one workspace" % N)
    n = cus() // 2 + 1
    rays_s, kw_s = scene("audio", n, NF)
    dense_s = render("audio", rays_s, NF, kw_s, False)
    # (a render takes a record workspace of the size of its own pass: hand it the front of the used one, which is kept as it is)
    front = ring[:int(pkg("_lib").lib().sahs_model_render_sparse_workspace_bytes(0, n * (NC + NF)))]
    ws_s = {"sparse": front}
    small = render("audio", rays_s, NF, kw_s, True, ws=ws_s)
    assert ws_s["sparse"] is front
    compare(dense_s, small, None, True, "N=%d through the used workspace" % n)


def test_fallback_to_slabs():
    """a record workspace of one ray's samples rounded up to a tile: below the rings' need, so the pass runs as trunk + branch launches over
    slabs of one ray -- still bit-equal"""
    ops, lib = pkg("ops"), pkg("_lib")
    N = cus() + 1
    rays, kw = scene("audio", N, NF)
    dense = render("audio", rays, NF, kw, False)
    was = ops.sparse_workspace_bytes()
    try:
        ops.sparse_branches(workspace_bytes=int(lib.lib().sahs_model_render_sparse_workspace_bytes(0, tiles(NC + NF) * TILE)))
        slabs = render("audio", rays, NF, kw, True)
    finally:
        ops.sparse_branches(workspace_bytes=was)
    live = compare(dense, slabs, None, True, "N=%d through slabs" % N, fused=False)
    assert slabs[4] == int(live[-1].sum()), "the last slab is the last ray"
    report("N=%d through slabs" % N, live, N * (NC + NF))


def test_default_workspace_is_the_rings():
    """the default bound is what the fused form needs on this device: 512 slots per CU and the head"""
    ops, lib = pkg("ops"), pkg("_lib")
    L = lib.lib()
    assert ops.sparse_workspace_bytes() == L.sahs_model_render_sparse_workspace_bytes(0, 512 * cus())
    for samples in (1, 128, 129, cus() * TILE, cus() * TILE + 1, 5 * cus() * TILE, 1 << 24):
        need = L.sahs_model_render_sparse_fused_workspace_bytes(0, samples)
        assert need <= L.sahs_model_render_sparse_workspace_bytes(0, samples) and need <= ops.sparse_workspace_bytes()
