"""The fused sparse instances of the fp32 field kernel (csrc/field_f32.hip: FIELD_ALL_FUSED / FIELD_RADIANCE_FUSED): one launch per pass, every
persistent workgroup appending its live samples to a private record ring and running the branch layers itself whenever the ring held a
tile's worth when a tile started, then draining the ring.  Everything is compared bit for bit against the dense launches
(ops.sparse_branches(False)) with the recipe of tests/sparse_reference.py, at 64 coarse + 64 fine samples -- one fine tile of 128 samples
per ray -- so that with C compute units a pass over N rays gives every workgroup one tile of each full row of C tiles: N = 3 C + 1 is
three tiles for every workgroup and a fourth for one.

What can go wrong is in the ring: the slot arithmetic across its end, the carried count (a branch pass at every tile when everything is
live, none before the drain when little is), the partial last drain pass, records of the previous tile read by another wave, a workspace
of exactly the rings' size, and the count and head words of the workspace."""
import pytest
import torch

from conftest import pkg
from sparse_reference import NC, TILE, compare, cus, dev, render, scene, tiles

pytestmark = pytest.mark.gpu

NF = 64
# density bias of the drain-only case: chosen on the first run so that the fine pass of 3 C + 1 rays has fewer than 128 live records per
# workgroup, i.e. under a third of its samples live (256 CUs, 98,432 samples: bias -2 gave 32.3 % live, -4 22.3 %, -6 14.7 % = 14,517 records
# against the 32,768 allowed, -8 9.0 %)
DRAIN_ONLY_BIAS = -6.0


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
    front = ring[:int(pkg("_lib").lib().sahs_model_render_sparse_fused_workspace_bytes(0, n * (NC + NF)))]
    ws_s = {"sparse": front}
    small = render("audio", rays_s, NF, kw_s, True, ws=ws_s)
    assert ws_s["sparse"] is front
    compare(dense_s, small, None, True, "N=%d through the used workspace" % n)


def test_workspace_of_exactly_the_rings():
    """C + 1 whole fine tiles through a caller-kept workspace whose record buffer is exactly what the fused size query asks for the pass:
    rings of 256 slots for one workgroup and 128 for the others, and nothing behind the last one"""
    L = pkg("_lib").lib()
    N = cus() + 1
    rays, kw = scene("audio", N, NF)
    dense = render("audio", rays, NF, kw, False)
    need = int(L.sahs_model_render_sparse_fused_workspace_bytes(0, N * (NC + NF)))
    assert need == 256 + (cus() + 1) * TILE * 1040
    kept = torch.zeros(need, dtype=torch.uint8, device=dev())
    ws = {"sparse": kept}
    sparse = render("audio", rays, NF, kw, True, ws=ws)
    assert ws["sparse"] is kept
    compare(dense, sparse, None, True, "N=%d through a workspace of exactly %d bytes" % (N, need))


def test_default_workspace_is_the_rings():
    """what the fused form needs on this device never exceeds the device-independent bound, nor 512 slots per CU and the head"""
    L = pkg("_lib").lib()
    for samples in (1, 128, 129, cus() * TILE, cus() * TILE + 1, 5 * cus() * TILE, 1 << 24):
        need = L.sahs_model_render_sparse_fused_workspace_bytes(0, samples)
        assert need <= L.sahs_model_render_sparse_workspace_bytes(0, samples) and need <= L.sahs_model_render_sparse_workspace_bytes(0, 512 * cus())
