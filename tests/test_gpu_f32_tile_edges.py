"""The tile edges and tile prologues of the fp32 inference forward (csrc/f32_pipe.hpp: BIAS_AHEAD; csrc/field_f32.hip: ENC_ONCE), bit for
bit against kernels that do not have them.

The non-saving instances of field_forward_f32_kernel read a tile's bias four steps before the tile starts, into a ring of two register
quadruples that lives across a layer's chunks, and the whole-network sparse instance keeps the trunk's encodings live instead of building
them twice.  Both are schedule, not arithmetic.  What can go wrong: a ring slot read again before its tile took it, or not read at all (a
tile starts from another tile's bias: the first pair of a layer, the first pair of a later chunk, one-tile layers, layers that accumulate
onto the previous one), encodings that are stale when the skip layer takes them.  The cases are also those that a fetch of the NEXT tile's
inputs and an activation moved one step late would need (both were built with these tests, priced and dropped -- LAB_NOTES.md): a
workgroup without a next tile, a next tile that is the ragged last one, the rotation of the fused tiles, the last tiles of a chunk.

(a) Every dense mode of every architecture, the non-saving instance against the saving one -- which keeps the old step, 32 KB chunks and
    the compiler's order, and has none of the above: an independent schedule of the same arithmetic.  raw and x', w must be the same bits.
      one           P = 1                  one partial tile: the last tile's activation, the clamp, no next tile
      wrap_to_one   P = 128 CUs + 1        one workgroup has a next tile (of one sample), the others none
      three_ragged  P = 3 x 128 CUs + 129  every workgroup fetches ahead at least twice; the last tile is ragged
(b) The sparse render (FIELD_ALL_FUSED, FIELD_DEFORM, FIELD_RADIANCE_FUSED) against the dense render (ops.sparse_branches(False): modes 0,
    1, 2) with the recipe of tests/sparse_reference.py -- rows, depths, weights, live raw rows, every sigma, the record count -- at
    64 + 64 samples and N = 1, CUs + 1, 3 CUs + 1 rays, and one coarse-only pass of CUs x 128 + 1 samples whose samples per ray do not
    divide 128: tiles straddle rays (the ray of a lane's next sample is not the ray of its current one) and the last tile holds one sample.
"""
import pytest
import torch

import field_reference as FR
from conftest import pkg
from sparse_reference import NC, TILE, compare, cus, dev, render, scene, tiles

pytestmark = pytest.mark.gpu

SIZES = {"one": lambda c: 1, "wrap_to_one": lambda c: TILE * c + 1, "three_ragged": lambda c: 3 * TILE * c + TILE + 1}
XW_PAD, XW_COL0 = 5, 3      # xw rows hold S + 5 slots; the launches own columns 3 .. 3 + S - 1
_MODELS = {}


def model(arch):
    if arch not in _MODELS:
        ops, W = pkg("ops"), pkg("weights")
        flat = torch.from_numpy(W.flatten_state_dict(FR.state_dict_np(W, arch), model=arch)).to(dev())
        frame = ops.fold_conditioning(flat, FR.driving_input(arch, dev()), FR.pose_of(arch, dev()), arch=arch)
        _MODELS[arch] = dict(frame=frame, packed=ops.pack_weights(flat, ops.SAHS_F32, arch=arch))
    return _MODELS[arch]


def meaningful(t, what):
    assert bool(torch.isfinite(t).all()), what + ": not finite"
    assert float(t.min()) != float(t.max()), what + ": all values equal"


def same(a, b, what):
    FR.assert_same_bits(a, b, what + ": early bias / late activation / fetch ahead (no save) vs the plain step (saving)")


def split_pair(arch, level, mode, rays, z, xw_in=None, src=None):
    """one mode through the inference forward and through the training forward -> [(raw, xw written)] of each"""
    ops, m = pkg("ops"), model(arch)
    N, S = rays.shape[0], (src if mode == ops.FIELD_RADIANCE else z).shape[1]
    out = []
    for saving in (False, True):
        xw = xw_in if mode == ops.FIELD_RADIANCE else torch.full((N, S + XW_PAD, 8), float("nan"), device=dev())
        kw = dict(z=z, src=src, xw_col0=0 if mode == ops.FIELD_RADIANCE else XW_COL0, arch=arch)
        if saving:
            raw, _ = ops.field_forward_split_save(m["packed"], m["frame"], level, mode, rays, xw, bits=ops.alloc_sign_bits(N * S, mode, arch, dev()), **kw)
        else:
            raw = ops.field_forward_split(m["packed"], m["frame"], level, mode, rays, xw, **kw)
        out.append((raw, None if mode == ops.FIELD_RADIANCE else xw))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("arch", ["audio", "nerface", "nerface_static"])
def test_dense_modes_against_the_saving_instances(arch, size):
    ops = pkg("ops")
    P = SIZES[size](cus())
    N, S = FR.factor(P)
    rays, z, _ = FR.build_scene(arch, N, S, dev())
    print("%s %s: P=%d (N=%d x S=%d), %d tiles on %d CUs" % (arch, size, P, N, S, tiles(P), cus()))
    for level in (0, 1):
        what = "%s %s level %d" % (arch, size, level)
        if not FR.ARCH_DIMS[arch]["deform"]:      # the whole network only
            m = model(arch)
            plain = ops.field_forward(m["packed"], m["frame"], level, rays, z, arch=arch)
            saved, _ = ops.field_forward_save(m["packed"], m["frame"], level, rays, z, arch, bits=ops.alloc_sign_bits(P, ops.FIELD_ALL, arch, dev()))
            torch.cuda.synchronize()
            meaningful(plain, what + " raw")
            same(plain.reshape(P, 16), saved.reshape(P, 16), what + " raw")
            continue
        own = slice(XW_COL0, XW_COL0 + S)
        (raw_a, xw_a), (raw_b, xw_b) = split_pair(arch, level, ops.FIELD_ALL, rays, z)
        meaningful(raw_a, what + " FIELD_ALL raw")
        meaningful(xw_a[:, own, :5], what + " FIELD_ALL x', w")
        same(raw_a.reshape(P, 16), raw_b.reshape(P, 16), what + " FIELD_ALL raw")
        same(xw_a, xw_b, what + " FIELD_ALL xw")
        (_, xd_a), (_, xd_b) = split_pair(arch, level, ops.FIELD_DEFORM, rays, z)
        meaningful(xd_a[:, own, :5], what + " FIELD_DEFORM x', w")
        same(xd_a, xd_b, what + " FIELD_DEFORM xw")
        src = (FR.ray_permutation(N, S, dev()) + XW_COL0).contiguous()
        (rr_a, _), (rr_b, _) = split_pair(arch, level, ops.FIELD_RADIANCE, rays, None, xw_in=xw_a, src=src)
        meaningful(rr_a, what + " FIELD_RADIANCE raw")
        same(rr_a.reshape(P, 16), rr_b.reshape(P, 16), what + " FIELD_RADIANCE raw")


@pytest.mark.parametrize("rays_of", ["one", "cus_plus_1", "three_cus_plus_1"])
def test_sparse_render_against_the_dense_render(rays_of):
    """64 + 64 samples: a fine tile is one ray; the coarse pass (FIELD_ALL_FUSED) and the deformation launch run half as many tiles"""
    N = {"one": 1, "cus_plus_1": cus() + 1, "three_cus_plus_1": 3 * cus() + 1}[rays_of]
    rays, kw = scene("audio", N, 64)
    dense, sparse = render("audio", rays, 64, kw, False), render("audio", rays, 64, kw, True)
    live = compare(dense, sparse, None, True, "audio N=%d 64 + 64" % N)
    print("N=%d: %d live of %d samples, %d coarse and %d fine tiles on %d CUs" % (N, int(live.sum()), live.numel(), tiles(N * NC), tiles(N * (NC + 64)), cus()))
    assert 0 < int(live.sum()) < live.numel()


def test_coarse_tiles_that_straddle_rays():
    """CUs x 128 + 1 coarse samples, no fine pass, samples per ray a divisor of that count (256 CUs: 331 rays of 99)"""
    target = cus() * TILE + 1
    nc = next((s for s in range(256, 1, -1) if target % s == 0), None)
    assert nc is not None, "no sample count up to 256 divides %d" % target
    assert TILE % nc != 0, "%d samples per ray: no tile would straddle two rays" % nc
    N = target // nc
    rays, kw = scene("audio", N, 0, nc=nc)
    dense, sparse = render("audio", rays, 0, kw, False, nc=nc), render("audio", rays, 0, kw, True, nc=nc)
    live = compare(dense, sparse, None, True, "audio N=%d nc=%d nf=0 (%d samples)" % (N, nc, target))
    assert tiles(N * nc) == cus() + 1 and N * nc % TILE == 1
    assert 0 < int(live.sum()) < live.numel()
