"""The field kernels past one tile per workgroup, per sample.

field_forward_f32_kernel (128-sample tiles, 16 samples per wave), field_forward_bf16w_kernel (256 / 64) and the field_*_bf16x3 kernels
(128 / 32) are persistent: a launch over T tiles starts min(T, CUs) workgroups and workgroup g walks tiles g, g + CUs, ...  From one tile
of a workgroup to its next the double-buffered LDS weight ring, the stream offset with its wrap window, the per-tile refresh, stores left in
flight by the saving forward's counted waits and (sparse fine trunk) the prefetched next tile are carried over.  The per-sample tests
elsewhere stop at 31 tiles; here every launch runs two or three tiles per workgroup:

  one_past      P = CUs x TILE + 1           one workgroup gets a second tile, holding one sample
  two_rounds    P = 2 CUs x TILE             every workgroup runs two whole tiles
  ragged_third  P = 2 CUs x TILE + TILE + 77 workgroups 0 and 1 run three tiles; the last holds 77 samples (a partly filled wave, not the first)

MAIN INSTRUMENT, bit for bit: the field is pointwise (a sample is one column of every MFMA tile; columns never mix; nothing but the
weights is shared), so the large launch must equal the same rays evaluated in ray slices of at most half a round, where every workgroup
runs at most one tile -- the regime the oracle tests pin.  torch.equal through an int32 view; outputs are the leading slice of a
NaN-filled buffer whose guard rows must stay untouched.
SECOND INSTRUMENT, fp32 kernels: conftest.yardstick (its defaults) against oracle/torch_eager.py::EagerField in float64 with the eager
fp32 run's own error as the measure, over the whole launch and over the edge rows (last two tiles, first tile of every round, last 16
samples), with a sensitivity check on values only: the HIP rows P-1 / P-2 swapped, or row P-1 copied over row P-TILE-1, must fail it.

Observed on a 256-CU MI355X (the terminal summary's yardstick lines): max |HIP - float64| / max |eager fp32 - float64|, over the whole
launch and over its edge rows (257, 512 and 461 rows at the three sizes); the check is max <= 3 x the reference's + 32 ulps of scale, rms
<= 2 x.  Every bitwise comparison held, in all three kernels and every entry.
  model          size         L   sigma            sigma, edge      rgb/seg          rgb/seg, edge    dx               dx, edge         w                w, edge          grid             grid, edge
  audio          one_past     0   2.6e-04/1.4e-04  9.6e-05/1.1e-04  4.3e-05/2.7e-05  2.2e-05/1.9e-05  8.1e-08/4.3e-08  5.4e-08/2.7e-08  3.5e-07/6.4e-07  2.8e-07/2.6e-07  3.2e-06/3.2e-06  2.8e-06/2.3e-06
  audio          one_past     1   2.3e-04/1.6e-04  1.1e-04/8.4e-05  5.2e-05/2.8e-05  2.2e-05/1.5e-05  8.1e-08/4.3e-08  5.4e-08/2.7e-08  3.5e-07/6.4e-07  2.8e-07/2.6e-07  3.2e-06/3.2e-06  2.8e-06/2.3e-06
  audio          two_rounds   0   2.4e-04/1.6e-04  1.3e-04/9.1e-05  5.0e-05/2.7e-05  2.9e-05/1.4e-05  8.5e-08/4.4e-08  7.0e-08/2.9e-08  3.8e-07/4.5e-07  2.9e-07/2.9e-07  3.5e-06/3.2e-06  3.1e-06/3.1e-06
  audio          two_rounds   1   2.2e-04/1.5e-04  1.1e-04/1.1e-04  5.9e-05/2.6e-05  2.3e-05/1.7e-05  8.5e-08/4.4e-08  7.0e-08/2.9e-08  3.8e-07/4.5e-07  2.9e-07/2.9e-07  3.5e-06/3.2e-06  3.1e-06/3.1e-06
  audio          ragged_third 0   2.4e-04/1.7e-04  1.3e-04/9.1e-05  5.3e-05/2.8e-05  3.2e-05/2.0e-05  7.9e-08/4.5e-08  5.3e-08/4.5e-08  3.9e-07/5.3e-07  3.3e-07/4.3e-07  3.7e-06/3.7e-06  2.3e-06/1.9e-06
  audio          ragged_third 1   2.3e-04/1.6e-04  1.1e-04/9.7e-05  4.2e-05/3.1e-05  2.3e-05/1.8e-05  7.9e-08/4.5e-08  5.3e-08/4.5e-08  3.9e-07/5.3e-07  3.3e-07/4.3e-07  3.7e-06/3.7e-06  2.3e-06/1.9e-06
  nerface        one_past     0   9.0e-04/6.0e-04  5.3e-04/3.7e-04  1.2e-06/8.8e-07  6.5e-07/5.3e-07  1.2e-07/8.6e-08  8.0e-08/6.6e-08  1.1e-07/7.1e-08  5.9e-08/4.2e-08  1.3e-07/1.1e-07  6.9e-08/7.4e-08
  nerface        one_past     1   1.0e-03/6.7e-04  6.5e-04/4.7e-04  1.3e-06/1.0e-06  9.2e-07/4.9e-07  1.2e-07/8.6e-08  8.0e-08/6.6e-08  1.1e-07/7.1e-08  5.9e-08/4.2e-08  1.3e-07/1.1e-07  6.9e-08/7.4e-08
  nerface        two_rounds   0   7.7e-04/6.4e-04  5.0e-04/4.7e-04  1.7e-06/1.0e-06  1.2e-06/5.4e-07  1.4e-07/9.5e-08  1.1e-07/6.4e-08  1.1e-07/7.1e-08  6.8e-08/5.6e-08  1.5e-07/1.2e-07  8.0e-08/7.0e-08
  nerface        two_rounds   1   1.3e-03/7.8e-04  1.3e-03/5.4e-04  1.4e-06/1.1e-06  9.5e-07/7.1e-07  1.4e-07/9.5e-08  1.1e-07/6.4e-08  1.1e-07/7.1e-08  6.8e-08/5.6e-08  1.5e-07/1.2e-07  8.0e-08/7.0e-08
  nerface        ragged_third 0   8.2e-04/6.8e-04  6.0e-04/2.8e-04  1.2e-06/9.7e-07  9.2e-07/6.6e-07  1.4e-07/8.1e-08  9.6e-08/6.1e-08  9.6e-08/7.0e-08  7.2e-08/4.2e-08  1.4e-07/1.2e-07  9.2e-08/7.9e-08
  nerface        ragged_third 1   1.1e-03/7.6e-04  6.3e-04/5.0e-04  1.5e-06/9.4e-07  7.7e-07/6.2e-07  1.4e-07/8.1e-08  9.6e-08/6.1e-08  9.6e-08/7.0e-08  7.2e-08/4.2e-08  1.4e-07/1.2e-07  9.2e-08/7.9e-08
  nerface_static one_past     0   1.8e-05/3.7e-06  1.2e-05/2.6e-06  1.1e-07/3.6e-08  7.5e-08/2.2e-08  exactly 0        exactly 0        exactly 0        exactly 0        1.1e-07/1.1e-07  5.8e-08/5.8e-08
  nerface_static one_past     1   1.4e-05/4.2e-06  9.0e-06/2.8e-06  1.3e-07/4.2e-08  9.4e-08/3.6e-08  exactly 0        exactly 0        exactly 0        exactly 0        1.1e-07/1.1e-07  5.8e-08/5.8e-08
  nerface_static two_rounds   0   1.9e-05/4.0e-06  1.2e-05/2.7e-06  1.1e-07/4.2e-08  8.2e-08/3.0e-08  exactly 0        exactly 0        exactly 0        exactly 0        1.1e-07/1.1e-07  6.9e-08/6.9e-08
  nerface_static two_rounds   1   1.9e-05/3.7e-06  1.0e-05/2.3e-06  1.5e-07/4.4e-08  1.0e-07/3.3e-08  exactly 0        exactly 0        exactly 0        exactly 0        1.1e-07/1.1e-07  6.9e-08/6.9e-08
  nerface_static ragged_third 0   1.6e-05/3.9e-06  1.2e-05/3.1e-06  1.0e-07/4.3e-08  8.8e-08/2.6e-08  exactly 0        exactly 0        exactly 0        exactly 0        1.1e-07/1.1e-07  5.4e-08/5.4e-08
  nerface_static ragged_third 1   1.6e-05/3.4e-06  1.1e-05/2.3e-06  1.4e-07/5.1e-08  1.0e-07/2.7e-08  exactly 0        exactly 0        exactly 0        exactly 0        1.1e-07/1.1e-07  5.4e-08/5.4e-08
  ops.field_forward_split(FIELD_ALL), fp32: raw is bit-identical to the rows above at the same size; x' and w read back from xw:
  audio          ragged_third 0   x' 7.5e-08/4.5e-08  x', edge 5.3e-08/4.5e-08  w 3.9e-07/5.3e-07  w, edge 3.3e-07/4.3e-07
  audio          ragged_third 1   x' 7.5e-08/4.5e-08  x', edge 5.3e-08/4.5e-08  w 3.9e-07/5.3e-07  w, edge 3.3e-07/4.3e-07
  audio          one_past     0   x' 7.8e-08/4.3e-08  x', edge 5.0e-08/2.7e-08  w 3.5e-07/6.4e-07  w, edge 2.8e-07/2.6e-07
  audio          one_past     1   x' 7.8e-08/4.3e-08  x', edge 5.0e-08/2.7e-08  w 3.5e-07/6.4e-07  w, edge 2.8e-07/2.6e-07
  nerface        ragged_third 0   x' 1.4e-07/8.1e-08  x', edge 1.0e-07/6.1e-08  w 9.6e-08/7.0e-08  w, edge 7.2e-08/4.2e-08
  nerface        ragged_third 1   x' 1.4e-07/8.1e-08  x', edge 1.0e-07/6.1e-08  w 9.6e-08/7.0e-08  w, edge 7.2e-08/4.2e-08
  nerface        one_past     0   x' 1.2e-07/8.6e-08  x', edge 8.7e-08/6.6e-08  w 1.1e-07/7.1e-08  w, edge 5.9e-08/4.2e-08
  nerface        one_past     1   x' 1.2e-07/8.6e-08  x', edge 8.7e-08/6.6e-08  w 1.1e-07/7.1e-08  w, edge 5.9e-08/4.2e-08
"""
import time

import pytest
import torch

import field_reference as FR
from conftest import pkg

pytestmark = pytest.mark.gpu

_CACHE = {}
GUARD_ROWS = 512            # NaN rows behind P in a large launch's output: two tiles of the widest kernel
SENTINEL = 0x5A5A5A5A       # prefill of sign-bit buffers (bytes the kernels leave alone compare equal on both sides)
XW_PAD, XW_COL0 = 5, 3      # xw rows hold S + 5 slots; the launch owns columns 3 .. 3 + S - 1
PREC = {"fp32": "SAHS_F32", "bf16": "SAHS_BF16", "bf16x3": "SAHS_BF16X3"}
# (arch, precision) -> how the whole network is evaluated: ops.field_forward, or (the pairs that exist as the split chain only)
# ops.field_forward_split(FIELD_ALL)
WHOLE = {("audio", "fp32"): "forward", ("nerface", "fp32"): "forward", ("nerface_static", "fp32"): "forward", ("audio", "bf16"): "forward",
         ("nerface", "bf16"): "split", ("audio", "bf16x3"): "split", ("nerface_static", "bf16x3"): "forward"}
CHAIN = {("nerface", "bf16"), ("audio", "bf16x3")}      # FIELD_ALL is a deformation + a radiance launch: it takes xw_col0 == 0 only


def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def cus():
    return torch.cuda.get_device_properties(dev()).multi_processor_count


def model(arch):
    if ("model", arch) not in _CACHE:
        ops, W = pkg("ops"), pkg("weights")
        sd_np = FR.state_dict_np(W, arch)
        flat = torch.from_numpy(W.flatten_state_dict(sd_np, model=arch)).to(dev())
        frame = ops.fold_conditioning(flat, FR.driving_input(arch, dev()), FR.pose_of(arch, dev()), arch=arch)
        _CACHE[("model", arch)] = dict(sd_np=sd_np, flat=flat, frame=frame, packs={})
    return _CACHE[("model", arch)]


def pack(arch, prec):
    m, ops = model(arch), pkg("ops")
    if prec not in m["packs"]:
        m["packs"][prec] = ops.pack_weights(m["flat"], getattr(ops, PREC[prec]), arch=arch)
    return m["packs"][prec]


def case(arch, prec, size):
    """-> plan, rays, z, x6, slices; printed once per test"""
    pl = FR.plan(cus(), prec, size)
    key = ("scene", arch, pl["N"], pl["S"])
    if key not in _CACHE:
        for k in [k for k in _CACHE if k[0] in ("scene", "eager")]:      # one scene (and its float64 reference) at a time
            del _CACHE[k]
        _CACHE[key] = FR.build_scene(arch, pl["N"], pl["S"], dev())
    rays, z, x6 = _CACHE[key]
    sl = FR.ray_slices(pl["N"], pl["S"], pl["cus"], pl["tile"])
    print("%s %s %s: %s; %d small launches of at most %d samples" % (arch, prec, size, FR.describe(pl), len(sl), max((b - a) * pl["S"] for a, b in sl)))
    assert all((b - a) * pl["S"] <= pl["cus"] * pl["tile"] // 2 for a, b in sl)
    return pl, rays, z, x6, sl


def nan(*shape):
    return torch.full(shape, float("nan"), device=dev())


def guarded(N, S):
    """-> (buffer, out): out (N, S, 16) is the leading slice of a NaN-filled buffer with GUARD_ROWS rows behind it"""
    buf = nan((N * S + GUARD_ROWS) * 16)
    return buf, buf[:N * S * 16].view(N, S, 16)


def check_guard(buf, P, what):
    assert bool(torch.isfinite(buf[:P * 16]).all()), what + ": raw[:P] is not finite (a row was never written)"
    assert FR.same_bits(buf[P * 16:], nan(GUARD_ROWS * 16)), what + ": rows behind P were written"


def cat(parts):
    return {k: torch.cat([p[k] for p in parts], 0) for k in parts[0]}


def compare(big, small, what):
    for k in big:
        FR.assert_same_bits(big[k].reshape(big[k].shape[0], -1), small[k].reshape(small[k].shape[0], -1), "%s: %s, large launch vs small launches" % (what, k))


# ---------------------------------------------------------------------------------------------------------------------------------
# launches
# ---------------------------------------------------------------------------------------------------------------------------------
def whole_network(arch, prec, level, rays, z, guard=False):
    """-> dict of per-ray tensors: raw, and dx / w / grid (ops.field_forward with debug planes) or xw (the split chain)"""
    ops, m = pkg("ops"), model(arch)
    N, S = z.shape
    buf, out = guarded(N, S) if guard else (None, None)
    p = getattr(ops, PREC[prec])
    if WHOLE[(arch, prec)] == "forward":
        debug = prec == "fp32" or (arch, prec) == ("audio", "bf16")
        r = ops.field_forward(pack(arch, prec), m["frame"], level, rays, z, precision=p, debug=debug, out=out, arch=arch)
        res = dict(raw=r[0], dx=r[1], w=r[2], grid=r[3]) if debug else dict(raw=r)
    else:
        xw = nan(N, S, 8)
        raw = ops.field_forward_split(pack(arch, prec), m["frame"], level, ops.FIELD_ALL, rays, xw, z=z, out=out, arch=arch, precision=p)
        res = dict(raw=raw, xw=xw)
    torch.cuda.synchronize()
    if guard:
        check_guard(buf, N * S, "%s %s level %d" % (arch, prec, level))
    return res


def split_modes(arch, prec, level, rays, z, perm, guard=False, xw_from=None):
    """FIELD_ALL, FIELD_DEFORM and FIELD_RADIANCE over the same rays: xw rows of S + XW_PAD slots prefilled with NaN, the launches own
    columns XW_COL0 .. (0 for the FIELD_ALL of a split chain, which takes no other), src = a within-ray permutation of those columns.
    -> raw_all, xw_all, xw_deform, raw_radiance (read from xw_from, default this call's xw_all)"""
    ops = pkg("ops")
    N, S = z.shape
    p, pk, fr = getattr(ops, PREC[prec]), pack(arch, prec), model(arch)["frame"]
    col_all = 0 if (arch, prec) in CHAIN else XW_COL0
    bufs = [guarded(N, S) if guard else (None, None) for _ in range(2)]
    xw_all, xw_def = nan(N, S + XW_PAD, 8), nan(N, S + XW_PAD, 8)
    raw_all = ops.field_forward_split(pk, fr, level, ops.FIELD_ALL, rays, xw_all, z=z, xw_col0=col_all, out=bufs[0][1], arch=arch, precision=p)
    ops.field_forward_split(pk, fr, level, ops.FIELD_DEFORM, rays, xw_def, z=z, xw_col0=XW_COL0, arch=arch, precision=p)
    src = (perm + col_all).contiguous()
    raw_rad = ops.field_forward_split(pk, fr, level, ops.FIELD_RADIANCE, rays, xw_all if xw_from is None else xw_from, src=src, out=bufs[1][1],
                                      arch=arch, precision=p, validate_src=True)
    torch.cuda.synchronize()
    if guard:
        for (buf, _), nm in zip(bufs, ("FIELD_ALL", "FIELD_RADIANCE")):
            check_guard(buf, N * S, "%s %s level %d %s" % (arch, prec, level, nm))
    return dict(raw_all=raw_all, xw_all=xw_all, xw_deform=xw_def, raw_radiance=raw_rad)


# ---------------------------------------------------------------------------------------------------------------------------------
# the float64 yardstick (fp32 kernels)
# ---------------------------------------------------------------------------------------------------------------------------------
def eager(arch, level, x6):
    key = ("eager", arch, level, x6.shape[0])
    if key not in _CACHE:
        m = model(arch)
        _CACHE[key] = {dt: FR.eager_field(m["sd_np"], arch, level, x6, m["frame"][0:76], m["frame"][80:116], dt) for dt in (torch.float32, torch.float64)}
    return _CACHE[key]


def yardstick_case(arch, level, pl, x6, got, what):
    """got: {name: (P, k) HIP tensor} with names among raw, dx, xp, w, grid.  Each held over the whole launch and over the edge rows, raw
    as rgb/seg and sigma separately; then the sensitivity of the edge-set check, on values only."""
    ref = eager(arch, level, x6)
    r32, r64 = ref[torch.float32], ref[torch.float64]
    P, amb = pl["P"], FR.ARCH_DIMS[arch]["amb"]
    rows = FR.edge_rows(P, pl["cus"], pl["tile"])
    parts = []
    for k, g in got.items():
        g = g.reshape(P, -1)
        if k == "raw":
            parts += [("rgb/seg", g[:, :15], r32[k][:, :15], r64[k][:, :15]), ("sigma", g[:, 15], r32[k][:, 15], r64[k][:, 15])]
        elif r64[k] is None:      # no deformation nets: the point is not moved and there is no ambient coordinate
            assert float(g.abs().max()) == 0.0, "%s: %s must be exactly zero" % (what, k)
        else:
            parts.append((k, g[:, :amb] if k == "w" else g, r32[k], r64[k]))
    edge = {}
    for name, g, a, b in parts:
        FR.held(g, a, b, "%s %s" % (what, name))
        edge[name] = FR.held(g, a, b, "%s %s, %d edge rows" % (what, name, len(rows)), rows)
    # sensitivity: a misplaced row among the last ones must fail the edge-set check that has just passed
    raw = got["raw"].reshape(P, 16)
    sig = raw[:, 15]
    bound = FR.yardstick_bound(edge["sigma"])
    es = sig[torch.from_numpy(rows).to(sig.device)]
    spread = float(es.std())
    moved = (abs(float(sig[-1] - sig[-2])), abs(float(sig[-1] - sig[-pl["tile"] - 1])))
    print("%s: sigma over the %d edge rows spreads by %.3e (std), rows P-1/P-2 differ by %.3e, P-1/P-TILE-1 by %.3e; the edge-set bound is %.3e"
          % (what, len(rows), spread, moved[0], moved[1], bound))
    # a moved row r lands where row r' belongs: its error there is at least |sigma r - sigma r'| minus its own (which is within the bound),
    # so the check must fail once the two rows differ by more than twice the bound; "far more" for the set as a whole: a hundred times
    assert spread > 100.0 * bound and min(moved) > 2.0 * bound, "%s: the inputs make the sensitivity check vacuous" % what
    for fault, bad in (("rows P-1 and P-2 swapped", FR.swap_last_two(raw)), ("row P-1 copied over row P-TILE-1", FR.stale_row(raw, pl["tile"]))):
        assert FR.would_fail(bad[:, 15], r32["raw"][:, 15], r64["raw"][:, 15], rows), "%s: %s passes the edge-set check on sigma" % (what, fault)
        assert FR.would_fail(bad[:, :15], r32["raw"][:, :15], r64["raw"][:, :15], rows), "%s: %s passes the edge-set check on rgb/seg" % (what, fault)


# ---------------------------------------------------------------------------------------------------------------------------------
# whole network
# ---------------------------------------------------------------------------------------------------------------------------------
def whole_case(arch, prec, size):
    t0 = time.time()
    pl, rays, z, x6, sl = case(arch, prec, size)
    for level in (0, 1):
        what = "%s %s %s level %d" % (arch, prec, size, level)
        big = whole_network(arch, prec, level, rays, z, guard=True)
        small = cat([whole_network(arch, prec, level, rays[a:b].contiguous(), z[a:b].contiguous()) for a, b in sl])
        compare(big, small, what)
        if prec == "fp32":
            yardstick_case(arch, level, pl, x6, big, "tiles %s %s L%d" % (arch, size, level))
    print("%s %s %s: %.1f s" % (arch, prec, size, time.time() - t0))


@pytest.mark.parametrize("size", FR.SIZES)
@pytest.mark.parametrize("arch", ["audio", "nerface", "nerface_static"])
def test_fp32_field_forward(arch, size):
    """ops.field_forward, fp32, debug planes: raw, dx, w and grid of the large launch equal the small launches' bit for bit, both levels;
    each held to the float64 yardstick over the whole launch and over its edge rows."""
    whole_case(arch, "fp32", size)


@pytest.mark.parametrize("arch,size", [("audio", s) for s in FR.SIZES] + [("nerface", "ragged_third")])
def test_bf16_field_forward(arch, size):
    """field_forward_bf16w_kernel, 256-sample tiles: the AudioFaceModel through ops.field_forward (raw and its debug planes), the
    NeRFaceModel through its mixed-precision chain (split-operand deformation launch, bf16 radiance launch: raw and xw)."""
    whole_case(arch, "bf16", size)


@pytest.mark.parametrize("arch,size", [("audio", s) for s in FR.SIZES] + [("nerface_static", "ragged_third")])
def test_bf16x3_field_forward(arch, size):
    """the split-operand kernels: the AudioFaceModel as the deformation + radiance chain (raw and xw), the NeRFaceModel without
    deformation nets as the whole-network kernel"""
    whole_case(arch, "bf16x3", size)


# ---------------------------------------------------------------------------------------------------------------------------------
# split evaluation
# ---------------------------------------------------------------------------------------------------------------------------------
def split_case(arch, prec, size):
    t0 = time.time()
    pl, rays, z, x6, sl = case(arch, prec, size)
    N, S, P = pl["N"], pl["S"], pl["P"]
    perm = FR.ray_permutation(N, S, dev())
    assert S == 1 or not bool((perm == torch.arange(S, device=dev(), dtype=torch.int32)).all()), "src must not be the identity"
    for level in (0, 1):
        what = "%s %s %s split level %d" % (arch, prec, size, level)
        big = split_modes(arch, prec, level, rays, z, perm, guard=True)
        small = cat([split_modes(arch, prec, level, rays[a:b].contiguous(), z[a:b].contiguous(), perm[a:b].contiguous(),
                                 xw_from=big["xw_all"][a:b].contiguous()) for a, b in sl])
        compare(big, small, what)      # (whole xw buffers: the NaN pattern of the slots a launch does not own included)
        col_all = 0 if (arch, prec) in CHAIN else XW_COL0
        for nm, col in (("xw_all", col_all), ("xw_deform", XW_COL0)):      # a launch writes x', w of its own slots and no other slot
            xw = big[nm]
            assert bool(torch.isfinite(xw[:, col:col + S, :5]).all()), "%s: %s holds x', w that are not finite" % (what, nm)
            assert FR.same_bits(xw[:, :col], nan(N, col, 8)) and FR.same_bits(xw[:, col + S:], nan(N, S + XW_PAD - col - S, 8)), \
                "%s: %s: slots outside columns %d..%d were written" % (what, nm, col, col + S - 1)
        if prec == "fp32":      # (the fp32 kernel writes five floats of a slot's eight; the others write the whole 32-byte slot)
            assert int(torch.isfinite(big["xw_all"]).sum()) == 5 * P and int(torch.isfinite(big["xw_deform"]).sum()) == 5 * P, what
        picked = torch.gather(big["raw_all"], 1, perm.long()[..., None].expand(N, S, 16))
        FR.assert_same_bits(big["raw_radiance"].reshape(P, 16), picked.reshape(P, 16), what + ": raw_radiance[n, s] vs FIELD_ALL raw[n, src[n, s]]")
        if prec == "fp32":
            FR.assert_same_bits(big["xw_deform"], big["xw_all"], what + ": x', w of FIELD_DEFORM vs FIELD_ALL")
            xw = big["xw_all"][:, XW_COL0:XW_COL0 + S]
            yardstick_case(arch, level, pl, x6, dict(raw=big["raw_all"], xp=xw[..., 0:3], w=xw[..., 3:5]), "tiles %s %s split L%d" % (arch, size, level))
    print("%s %s %s split: %.1f s" % (arch, prec, size, time.time() - t0))


@pytest.mark.parametrize("size", ["ragged_third", "one_past"])
@pytest.mark.parametrize("arch", ["audio", "nerface"])
def test_fp32_field_forward_split(arch, size):
    """ops.field_forward_split, fp32: FIELD_ALL, FIELD_DEFORM and FIELD_RADIANCE with xw rows wider than S, a column offset and a
    permuting src; FIELD_ALL also held to the float64 yardstick (raw, x', w)."""
    split_case(arch, "fp32", size)


@pytest.mark.parametrize("prec", ["bf16", "bf16x3"])
def test_lowp_field_forward_split(prec):
    split_case("audio", prec, "ragged_third")


# ---------------------------------------------------------------------------------------------------------------------------------
# saving forward
# ---------------------------------------------------------------------------------------------------------------------------------
def sign_buffer(P, mode, arch):
    bits = pkg("ops").alloc_sign_bits(P, mode, arch, dev())
    assert bits is not None and bits.shape[1] == FR.bits_table(arch)[1][mode]
    return bits.fill_(SENTINEL)


def saves(arch, prec, level, rays, z):
    """-> {form: dict(raw, act, bits)} of whole-network saves of these rays.  NeRFaceModels: "whole" = ops.field_forward_save with sign
    bits; AudioFaceModel: "all" = field_forward_split_save(FIELD_ALL) (fp32 only) and "pair" = a FIELD_DEFORM + a FIELD_RADIANCE launch
    into one whole-network save (whole=), src the identity"""
    ops, m = pkg("ops"), model(arch)
    N, S = z.shape
    P = N * S
    p, pk, fr = getattr(ops, PREC[prec]), pack(arch, prec), m["frame"]
    out = {}
    if arch != "audio":
        bits = sign_buffer(P, ops.FIELD_ALL, arch)
        raw, act = ops.field_forward_save(pk, fr, level, rays, z, arch, bits=bits, precision=p)
        out["whole"] = dict(raw=raw, act=act, bits=bits)
    else:
        if prec == "fp32":
            bits = sign_buffer(P, ops.FIELD_ALL, arch)
            raw, act = ops.field_forward_split_save(pk, fr, level, ops.FIELD_ALL, rays, nan(N, S, 8), z=z, bits=bits)
            out["all"] = dict(raw=raw, act=act, bits=bits)
        bits, act, xw = sign_buffer(P, ops.FIELD_ALL, arch), nan(P, FR.act_words(arch, FR.FIELD_ALL)), nan(N, S, 8)
        ident = torch.arange(S, dtype=torch.int32, device=dev()).repeat(N, 1).contiguous()
        ops.field_forward_split_save(pk, fr, level, ops.FIELD_DEFORM, rays, xw, z=z, precision=p, whole=(act, bits))
        raw, _ = ops.field_forward_split_save(pk, fr, level, ops.FIELD_RADIANCE, rays, xw, src=ident, precision=p, whole=(act, bits))
        out["pair"] = dict(raw=raw, act=act, bits=bits, xw=xw)
    torch.cuda.synchronize()
    return out


def check_planes(arch, big, P, small, p0, p1, what):
    """every activation plane (its defined columns) and every sign-bit plane of the large save, rows [p0, p1), against a small save"""
    Ps = p1 - p0
    for name, col, width, defined, _, _ in FR.act_table(arch)[0]:
        if defined:
            FR.assert_same_bits(FR.plane(big["act"], P, col, width)[p0:p1, :defined], FR.plane(small["act"], Ps, col, width)[:, :defined],
                                "%s: activation plane %s, samples %d..%d" % (what, name, p0, p1))
    for name, (wcol, width) in FR.bits_table(arch)[0].items():
        nw = FR.sign_words(width)
        FR.assert_same_bits(FR.plane(big["bits"], P, wcol, nw)[p0:p1], FR.plane(small["bits"], Ps, wcol, nw), "%s: sign plane %s, samples %d..%d" % (what, name, p0, p1))


def check_signs(arch, sv, P, what):
    """every sign bit = saved post-activation > 0, and every defined activation is finite (written)"""
    signs = FR.bits_table(arch)[0]
    for name, col, width, defined, _, sign in FR.act_table(arch)[0]:
        if not defined:
            continue
        a = FR.plane(sv["act"], P, col, width)[:, :defined]
        assert bool(torch.isfinite(a).all()), "%s: activation plane %s is not finite" % (what, name)
        if sign is not None:
            got = FR.decode_sign_bits(sv["bits"], P, signs[sign][0], width)
            bad = int((got != (a > 0)).sum())
            assert bad == 0, "%s: %d sign bits of %s differ from (saved activation > 0)" % (what, bad, name)


def save_case(arch, prec):
    t0 = time.time()
    ops = pkg("ops")
    pl, rays, z, x6, sl = case(arch, prec, "ragged_third")
    N, S, P = pl["N"], pl["S"], pl["P"]
    for level in (0, 1):
        big = saves(arch, prec, level, rays, z)
        # raw: the saving launch against the launch that saves nothing
        if arch != "audio":
            plain = ops.field_forward(pack(arch, prec), model(arch)["frame"], level, rays, z, precision=getattr(ops, PREC[prec]), arch=arch)
        else:
            xw = nan(N, S, 8)
            plain = ops.field_forward_split(pack(arch, prec), model(arch)["frame"], level, ops.FIELD_ALL, rays, xw, z=z, precision=getattr(ops, PREC[prec]))
        for form, sv in big.items():
            what = "%s %s save[%s] level %d" % (arch, prec, form, level)
            FR.assert_same_bits(sv["raw"].reshape(P, 16), plain.reshape(P, 16), what + ": raw of the saving launch vs the plain launch")
            assert sv["act"].shape == (P, FR.act_words(arch, FR.FIELD_ALL))
            check_signs(arch, sv, P, what)
        if "all" in big and "pair" in big:      # (fp32) the pair leaves what the one FIELD_ALL launch leaves
            check_planes(arch, big["all"], P, big["pair"], 0, P, "%s fp32 level %d: FIELD_ALL save vs FIELD_DEFORM + FIELD_RADIANCE save" % (arch, level))
        for a, b in sl:
            small = saves(arch, prec, level, rays[a:b].contiguous(), z[a:b].contiguous())
            for form, sv in small.items():
                what = "%s %s save[%s] level %d" % (arch, prec, form, level)
                FR.assert_same_bits(big[form]["raw"][a:b].reshape(-1, 16), sv["raw"].reshape(-1, 16), what + ": raw, large launch vs small launch")
                check_planes(arch, big[form], P, sv, a * S, b * S, what)
            del small
        del big
    torch.cuda.empty_cache()
    print("%s %s saving forward: %.1f s" % (arch, prec, time.time() - t0))


@pytest.mark.parametrize("arch", ["nerface", "nerface_static"])
def test_fp32_field_forward_save(arch):
    """ops.field_forward_save with sign bits at the ragged three-tile size: raw equals the plain launch's, every activation and sign
    plane equals the one re-assembled from small saves, every sign bit is (saved activation > 0)"""
    save_case(arch, "fp32")


@pytest.mark.parametrize("prec", ["fp32", "bf16x3"])
def test_audio_field_forward_split_save(prec):
    """ops.field_forward_split_save: FIELD_ALL (fp32), and FIELD_DEFORM + FIELD_RADIANCE into one whole-network save (fp32, bf16x3)"""
    save_case("audio", prec)
