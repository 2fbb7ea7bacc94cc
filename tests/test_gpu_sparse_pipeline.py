"""The fused sparse instances of the fp32 field kernel (csrc/field_f32.hip: FIELD_ALL_FUSED, and FIELD_RADIANCE_FUSED with its fine trunk
pipelined across tiles -- encodings built once per tile, the next tile's x', w fetched ahead) at the shapes where work carried from one tile
of a persistent workgroup to the next could go wrong: workgroups that run several tiles and end in a ragged one, exactly one tile (or one
sample) more than there are workgroups, record counts of 128 k and 128 k + 1, and the 4-layer trunks of the NeRFaceModels, at 64 + 64 and
64 + 128 samples per ray (the second no whole number of tiles).  tests/test_gpu_sparse_branches.py stops at 300 rays -- at most 450
tiles, under two per workgroup on a 256-CU device.  Everything is compared bit for bit against the dense launches
(ops.sparse_branches(False)) with the recipe of tests/sparse_reference.py.

Tiles per workgroup: a launch over T tiles of 128 samples starts min(T, CUs) workgroups; every workgroup runs one tile of each full row of
CUs tiles, the first T % CUs one more: the least any of them runs is T // CUs (when T >= CUs), the most ceil(T / CUs)."""
import pytest

from sparse_reference import NC, TILE, compare, cus, render, scene, tiles

pytestmark = pytest.mark.gpu


def check_steady(arch, N, nf, share, noise_std, what):
    rays, kw = scene(arch, N, nf, noise_std=noise_std)
    dense, sparse = render(arch, rays, nf, kw, False, share), render(arch, rays, nf, kw, True, share)
    live = compare(dense, sparse, kw.get("noise_f"), True, what)
    dead = 1.0 - float(live.float().mean())
    t_fine, t_branch = tiles(N * (NC + nf)), tiles(sparse[4])
    print("%s: dead %.3f, fine pass %d tiles (every workgroup >= %d), %d tiles of live records (per workgroup up to about %d), %d CUs"
          % (what, dead, t_fine, t_fine // cus(), t_branch, -(-t_branch // cus()), cus()))
    assert 0.2 <= dead <= 0.8, "the dense raw has %.1f %% dead samples: the comparison would be vacuous" % (100 * dead)
    assert t_fine // cus() >= 3, "every workgroup of the fine pass should run at least 3 tiles (%d tiles, %d CUs)" % (t_fine, cus())
    assert -(-t_branch // cus()) >= 2, "the live records should be at least 2 branch passes per workgroup (%d tiles, %d CUs)" % (t_branch, cus())


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
    multiple of 128 for N = 128 m and one more than a multiple for N = 128 m - 1; m = 3 gives 381 tiles of records (or 380 and one
    record) to the 256 workgroups of a 256-CU device, whose rings are drained by partial passes."""
    N = 384 - extra
    rays, kw = scene("audio", N, 64)
    dense = render("audio", rays, 64, kw, False, density_bias=1e4)
    sparse = render("audio", rays, 64, kw, True, density_bias=1e4)
    compare(dense, sparse, None, True, "bias 1e4 N=%d" % N)
    assert sparse[4] == 127 * N and sparse[4] % TILE == extra
