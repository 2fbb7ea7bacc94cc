"""The feature grid's edge contract: positions on and around the grid's faces, their float64 reference, and mutants of it.
Shared by tests/test_grid_reference_host.py (host) and tests/test_gpu_grid_edges.py (GPU).  TEST INFRASTRUCTURE ONLY; importing it
needs no GPU.

The contract (models.py:346-365): the 32 features of a sample are F.grid_sample(spatial_embeddings, x', mode="bilinear",
padding_mode="zeros", align_corners=True) -- ix = (x' + 1) / 2 * 31 per axis, cell floor(ix), a corner outside 0..31 contributes zero and
receives no gradient, and d features / d x' is the derivative inside the cell floor(ix) names (one-sided at a lattice plane).

 * position_sets: named sets of positions, each built as origin + direction x depth from operands of at most 8 significant bits, so
   that the sum is exact in float32 however it is evaluated; every coordinate is exactly +-1 or at least 2^-10 of a cell off a lattice
   plane, so float32 and float64 name the same cell for every sample.
 * edge_state_dict: the architecture's weights with warp_field_mlp.fc_final zeroed: x' = x exactly, tanh' = 1, and d loss / d x' is
   visible in fc_final's own gradient.
 * make_case / host_frame / reference_masks: a backward_reference case dict over one set.
 * BorderField / HalfPixelField, mutants(): wrong lookups, computed from the reference.
 * feature_check / backward_errors / backward_check: the comparisons both test files use.
"""
import numpy as np
import torch
import torch.nn.functional as F

import backward_reference as BR
import field_reference as FR
from oracle import torch_eager as TE

G_RES = 32
LATTICE_MARGIN = 2.0 ** -10
SETS = ("faces", "half_out", "just_out", "far_out", "runs", "pile")
BACKWARD_SETS = tuple(s for s in SETS if s != "far_out")
ZERO_SETS = ("just_out", "far_out")           # every corner of every sample is outside: features and grid gradient are exactly zero
HALF = 1.0 + 2.0 ** -5                        # ix = 31.484 / -0.484: floor 31 / -1, four corners outside per such axis
JUST = (1.125, 1.1875, 1.25)                  # ix = 32.94, 33.91, 34.88 (floor 32, 33, 34); negated: -1.94, -2.91, -3.88 (floor -2, -3, -4)
FAR = (4.0, 2.0 ** 20, 0.875 * 2.0 ** 128)    # 0.875 * 2^128 = 2.98e38, the 3-bit float32 next to 3e38
RUN_CELL, ALT_CELLS, PILE_CELL = (10, 20, 5), ((11, 20, 5), (11, 21, 5)), (15, 7, 22)


def significant_bits(a):
    """per element: the length of the binary significand without its trailing zeros (0 for 0)"""
    m = (np.frexp(np.abs(np.asarray(a, np.float64)))[0] * 2.0 ** 53).astype(np.int64)
    low = m & -m
    return np.where(m == 0, 0, 53 - np.round(np.log2(np.maximum(low, 1))).astype(np.int64))


def _interior(rng, n):
    """n x 3 interior coordinates k / 128, |k| <= 120: (k + 128) * 31 / 256 is a multiple of 1/256 and an integer only at k = +-128"""
    return rng.randint(-120, 121, size=(n, 3)) / 128.0


def _cell_points(rng, cell, n, distinct=False):
    """n positions k / 128 inside cell (xi, yi, zi)"""
    axes = []
    for i in cell:
        lo, hi = 2.0 * i / (G_RES - 1) - 1.0, 2.0 * (i + 1) / (G_RES - 1) - 1.0
        axes.append(np.array([k for k in range(-128, 129) if lo < k / 128.0 < hi]))
    if distinct:
        idx = rng.permutation(len(axes[0]) * len(axes[1]) * len(axes[2]))[:n]
        assert len(idx) == n
        picks = np.stack(np.unravel_index(idx, [len(a) for a in axes]), 1)
    else:
        picks = np.stack([rng.randint(0, len(a), size=n) for a in axes], 1)
    return np.stack([axes[a][picks[:, a]] for a in range(3)], 1) / 128.0


def _on_axes(rng, values, variants=(2, 1, 1)):
    """`values` (signed) put on one, two and three coordinates in every axis and sign combination; the other coordinates interior"""
    rows = []
    for naxes in (1, 2, 3):
        for axes in ((0,), (1,), (2,)) if naxes == 1 else ((0, 1), (0, 2), (1, 2)) if naxes == 2 else ((0, 1, 2),):
            for signs in np.ndindex(*([2] * naxes)):
                for _ in range(variants[naxes - 1]):
                    x = _interior(rng, 1)[0]
                    for a, s in zip(axes, signs):
                        x[a] = values[rng.randint(len(values))] * (1.0 if s else -1.0)
                    rows.append(x)
    return np.array(rows)


def _targets(name, rng):
    if name == "faces":          # ix = 0 / 31 exactly on one, two, three axes
        return _on_axes(rng, (1.0,))
    if name == "half_out":       # floor -1 / 31: four, six, seven corners outside
        return _on_axes(rng, (HALF,))
    if name == "just_out":       # floor <= -2 / >= 32 on at least one axis: no corner inside; the other axes interior, on a face, half out
        rows = []
        for a in range(3):
            for v in JUST:
                for s in (1.0, -1.0):
                    x = _interior(rng, 1)[0]
                    x[a] = s * v
                    rows.append(x)
        for a, b, va, vb in ((0, 1, 1.125, 1.0), (1, 2, -1.125, -1.0), (2, 0, 1.25, -1.0), (0, 2, -1.1875, 1.0), (1, 0, 1.125, HALF), (2, 1, -1.125, -HALF),
                             (0, 1, 1.125, -1.25), (1, 2, -1.1875, -1.125), (2, 0, 1.25, 1.1875), (0, 2, -1.125, 1.125)):
            x = _interior(rng, 1)[0]
            x[a], x[b] = va, vb
            rows.append(x)
        return np.array(rows)
    if name == "far_out":
        rows = []
        for a in range(3):
            for v in FAR:
                for s in (1.0, -1.0):
                    x = _interior(rng, 1)[0]
                    x[a] = s * v
                    rows.append(x)
        return np.array(rows)
    if name == "runs":           # one cell across the 16-sample chunks; a cell change on every sample; a tail that leaves P = 1 (mod 16)
        alt = np.empty((40, 3))
        alt[0::2], alt[1::2] = _cell_points(rng, ALT_CELLS[0], 20), _cell_points(rng, ALT_CELLS[1], 20)
        return np.concatenate([_cell_points(rng, RUN_CELL, 40, distinct=True), alt, _interior(rng, 17)])
    if name == "pile":           # hundreds of half-waves adding into the same eight voxels
        return _cell_points(rng, PILE_CELL, 512)
    raise KeyError(name)


def check_positions(ps):
    """the builder's asserts: few-bit operands, an exact sum however it is evaluated, every coordinate +-1 or off the lattice planes"""
    o, d, z, x = ps["o"], ps["d"], ps["z"], ps["x"]
    for nm, a in (("origin", o), ("direction", d), ("depth", z)):
        assert significant_bits(a).max() <= 8, "%s: %s has an operand of more than 8 significant bits" % (ps["name"], nm)
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
    x64 = o + d * z[:, None]
    o32, d32, z32 = (a.astype(np.float32) for a in (o, d, z))
    prod = d32 * z32[:, None]
    assert prod.dtype == np.float32 and np.array_equal(prod.astype(np.float64), d * z[:, None]), ps["name"] + ": direction x depth rounds in float32"
    x32 = o32 + prod
    assert x32.dtype == np.float32 and np.array_equal(x32.astype(np.float64), x64), ps["name"] + ": float32 and float64 o + d z differ"
    assert np.array_equal(x, x64) and np.isfinite(x64).all()
    ix = (x64 + 1.0) / 2.0 * (G_RES - 1)
    frac = ix - np.floor(ix)
    off = (frac >= LATTICE_MARGIN) & (frac <= 1.0 - LATTICE_MARGIN)
    huge = np.abs(x64) >= 2.0 ** 24         # far_out: every float32 there is a whole number; only "features are exactly 0" is compared
    assert (off | (np.abs(x64) == 1.0) | huge).all(), ps["name"] + ": a coordinate within 2^-10 of a lattice plane"
    assert not huge.any() or ps["name"] == "far_out"
    with np.errstate(over="ignore"):        # (far_out: 2.98e38 * 31 is +inf in float32, as in the kernels)
        ix32 = ((x32 + np.float32(1.0)) / np.float32(2.0)) * np.float32(G_RES - 1)
    cell, cell32 = np.floor(ix), np.floor(ix32).astype(np.float64)
    near = np.abs(x64) < 2.0                # (beyond: both sides only have to agree that no corner is inside)
    assert ix32.dtype == np.float32 and np.array_equal(cell32[near], cell[near]), ps["name"] + ": float32 and float64 name different cells"
    assert (np.minimum(np.abs(cell32[~near]), np.abs(cell[~near])) > G_RES + 1).all()
    if ps["name"] == "faces":
        assert (np.abs(x64) == 1.0).any(1).all() and {1, 2, 3} <= set((np.abs(x64) == 1.0).sum(1))
    if ps["name"] == "half_out":
        out = ((cell == -1) | (cell == G_RES - 1)).sum(1)
        assert {1, 2, 3} <= set(out) and (out >= 1).all() and ((cell >= -1) & (cell <= G_RES - 1)).all()
    if ps["name"] in ZERO_SETS:
        assert ((cell <= -2) | (cell >= G_RES)).any(1).all()
    if ps["name"] == "runs":
        assert ps["P"] % 16 == 1 and (cell[:40] == np.array(RUN_CELL)).all()
        assert (cell[40:80:2] == np.array(ALT_CELLS[0])).all() and (cell[41:80:2] == np.array(ALT_CELLS[1])).all()
    if ps["name"] == "pile":
        assert ps["P"] == 512 and (cell == np.array(PILE_CELL)).all()


_SETS = {}


def position_sets():
    """{name: dict(name, P, o (P, 3), d (P, 3), z (P,), x (P, 3) = o + d z; float64 arrays of float32-exact values)}"""
    if not _SETS:
        for i, name in enumerate(SETS):
            rng = np.random.RandomState(100 + i)
            x = _targets(name, rng)
            P = x.shape[0]
            z = np.array([0.5, 0.75, 1.0])[rng.randint(0, 3, size=P)]
            d = rng.randint(-12, 13, size=(P, 3)) / 16.0
            d[np.abs(x) >= 2.0] = 0.0            # a far coordinate is the origin's: nothing of 8 bits adds to 2^20 exactly
            ps = dict(name=name, P=P, o=x - d * z[:, None], d=d, z=z, x=x)
            check_positions(ps)
            _SETS[name] = ps
    return _SETS


def launch_inputs(ps, device):
    """-> rays (P, 8), z (P, 1), x6 (P, 6): one ray per sample"""
    P = ps["P"]
    rays = np.zeros((P, 8), np.float32)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = ps["o"], ps["d"], 0.25, 2.0
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
    return t(rays), t(ps["z"][:, None]), t(np.concatenate([ps["x"], ps["d"]], 1))


# ---------------------------------------------------------------------------------------------------------------------------------
# weights and cases
# ---------------------------------------------------------------------------------------------------------------------------------
def edge_state_dict(weights_mod, arch):
    """field_reference.state_dict_np with the warp head zeroed (deforming architectures): x' = x + tanh(0) = x exactly on every side"""
    sd = dict(FR.state_dict_np(weights_mod, arch))
    # The reference's initial grid (sigma 0.01) leaves d x' to the encodings alone: the hdr variant's sigma 0.3, as the AudioFaceModel's.
    if arch != "audio":
        sd["spatial_embeddings"] = sd["spatial_embeddings"] * np.float32(30.0)
    # NeRFaceModel: octave k of PE(x') multiplies d x' by 2^k, up to 2^14, and with hashed weights of one size on every octave the
    # grid's share of fc_final's gradient is 1e-4 of its scale, below that walk's bound.  The trunk's weights on octave k are damped by
    # 2^-k (layer 0 and the skip layer 3), as a network that has learnt a smooth field has them.
    if arch == "nerface":
        for lvl in ("coarse", "fine"):
            for layer, col0 in ((0, 0), (3, 256)):
                w = sd["nerf_mlps.%s.layers_xyz.%d.weight" % (lvl, layer)].copy()
                for k in range(15):
                    w[:, col0 + 3 + 6 * k:col0 + 9 + 6 * k] *= np.float32(2.0 ** -k)
                sd["nerf_mlps.%s.layers_xyz.%d.weight" % (lvl, layer)] = w
    for k in ("warp_field_mlp.fc_final.weight", "warp_field_mlp.fc_final.bias"):
        if k in sd:
            sd[k] = np.zeros_like(sd[k])
    return sd


def host_frame(arch):
    """a frame's conditioning words without the HIP fold: [0:76] a fixed driving vector, [80:116] the pose encoding"""
    frame = torch.zeros(128)
    frame[0:76] = torch.from_numpy(np.random.RandomState(7).standard_normal(76).astype(np.float32)) * 0.5
    frame[80:116] = TE.EagerField.pose_encoding(FR.pose_of(arch, torch.device("cpu")))[0]
    return frame


def make_case(weights_mod, arch, name, level, device, frame, flat=None, sd_np=None):
    """the backward_reference case dict over one position set: upstream d raw (and, AudioFaceModel, a seam gradient) drawn on the host"""
    ps = position_sets()[name]
    P = ps["P"]
    rays, z, x6 = launch_inputs(ps, device)
    rng = np.random.RandomState(1000 * SETS.index(name) + 10 * BR_ARCHS.index(arch) + level)
    t = lambda a: torch.from_numpy(a.astype(np.float32)).to(device).contiguous()
    d_raw = t(rng.standard_normal((P, 16)))
    seam = t(rng.standard_normal((P, 8)) * np.array([1, 1, 1, 0, 1, 1, 0, 0.0]))
    sd_np = sd_np if sd_np is not None else edge_state_dict(weights_mod, arch)
    return dict(arch=arch, N=P, S=1, P=P, sd_np=sd_np, flat=flat, frame=frame, rays=rays, z=z, x6=x6, d_raw=d_raw, seam=seam if arch == "audio" else None,
                level=level, off=weights_mod.canonical_offsets(arch), set=name)


BR_ARCHS = ("audio", "nerface", "nerface_static")


class RecordingField(TE.EagerField):
    """EagerField that notes the side of zero every hidden unit takes (the masks another run is then held to)"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.seen = {}

    def act(self, name, x, slope):
        self.seen[name] = (x > 0).detach()
        return super().act(name, x, slope)


def reference_masks(c):
    """the float64 reference's own sides (host tests; the GPU tests read the HIP forward's from its save)"""
    sd = {k: torch.from_numpy(v).to(c["x6"].device, torch.float64) for k, v in c["sd_np"].items()}
    field = RecordingField(sd, num_coarse=c["P"], num_fine=0, arch=c["arch"])
    with torch.no_grad():
        field.forward("coarse" if c["level"] == 0 else "fine", c["x6"].double(), None, None, driving=c["frame"][0:76].double(), pose36=c["frame"][80:116].double())
    return field.seen


# ---------------------------------------------------------------------------------------------------------------------------------
# the lookup and its mutants
# ---------------------------------------------------------------------------------------------------------------------------------
class _GridVariant(TE.EagerField):
    padding_mode, align_corners = "zeros", True

    def grid(self, level, xyz):
        g = self.sd["spatial_embeddings"]
        c = xyz.to(g.dtype).reshape(1, 1, 1, -1, 3)
        s = F.grid_sample(g, c, mode="bilinear", padding_mode=self.padding_mode, align_corners=self.align_corners)
        return s.reshape(g.shape[1], -1).t()


class BorderField(_GridVariant):
    padding_mode = "border"


class HalfPixelField(_GridVariant):
    align_corners = False


FIELDS = {"reference": TE.EagerField, "border": BorderField, "half_pixel": HalfPixelField}


def features(sd_np, arch, x, dtype, variant="reference"):
    """(P, 32) features at x (a torch tensor on the device to compute on) under a lookup variant"""
    g = torch.from_numpy(sd_np["spatial_embeddings"]).to(x.device, dtype)
    field = FIELDS[variant]({"spatial_embeddings": g}, num_coarse=x.shape[0], num_fine=0, arch=arch)
    with torch.no_grad():
        return field.grid("coarse", x.to(dtype))


class InwardField(_GridVariant):
    """the lookup with every coordinate exactly on a face moved 2^-20 into the grid (the encodings keep x'): the coordinate gradient then
    is the neighbouring interior cell's"""
    step = 2.0 ** -20

    def grid(self, level, xyz):
        face = (xyz.detach().abs() == 1.0).to(xyz.dtype)
        return super().grid(level, xyz - face * torch.sign(xyz.detach()) * self.step)


COORD_KEYS = ("seam_x", "warp_field_mlp.fc_final.weight", "warp_field_mlp.fc_final.bias")


def mutants(c, masks, ref):
    """{name: gradient dict} of wrong backwards, all from the float64 reference on the host forward's / HIP forward's sides: zeros padding
    replaced by border; align_corners=False; the grid gradient without sample 0's contribution (a face sample in `faces`, a half-outside
    one in `half_out`); the coordinate gradient of the face samples taken in the neighbouring interior cell"""
    P = c["P"]
    out = {"border": BR._eager(c, masks, 0, P, field_cls=BorderField), "half_pixel": BR._eager(c, masks, 0, P, field_cls=HalfPixelField)}
    one = BR._eager(c, masks, 0, 1)
    out["drop_one"] = dict(ref, spatial_embeddings=ref["spatial_embeddings"] - one["spatial_embeddings"])
    if bool((c["x6"][:, :3].abs() == 1.0).any()):
        inner = BR._eager(c, masks, 0, P, field_cls=InwardField)
        out["inward"] = dict(ref, **{k: inner[k] for k in ("seam",) + COORD_KEYS[1:] if k in inner})
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the comparisons
# ---------------------------------------------------------------------------------------------------------------------------------
def feature_check(got, ref32, ref64, name, what):
    """the 32 features of one set: conftest.yardstick at its default factors against float64 grid_sample, float32 grid_sample's own error
    the measure; where every corner is outside, exactly 0.0.  Raises AssertionError; returns the yardstick record."""
    from conftest import yardstick
    n = lambda a: a.detach().double().cpu().numpy()
    if name in ZERO_SETS:
        assert float(ref64.abs().max()) == 0.0
        assert float(got.abs().max()) == 0.0, "%s: features of samples without a corner inside must be exactly 0.0, max |.| = %.3e" % (what, float(got.abs().max()))
    return yardstick(n(got), n(ref32), n(ref64), what)


def backward_errors(got, ref):
    """backward_reference._errors per tensor, plus "seam_x": the seam's d x' columns on their own scale"""
    errs = BR._errors(got, ref)
    if ref.get("seam") is not None and got.get("seam") is not None:
        g, r = got["seam"].double()[:, 0:3], ref["seam"][:, 0:3]
        errs["seam_x"] = float((g - r).abs().max()) / float(r.abs().max())
    return errs


def group_of(k):
    return "grid" if k == "spatial_embeddings" else "coord" if k in COORD_KEYS else "rest"


def _held32(g, r32, r64):
    """None, or what conftest.yardstick at its default factors says against one tensor (no line left in the session's log)"""
    from conftest import YARDSTICK_LOG, yardstick
    n = lambda t: t.detach().double().cpu().numpy()
    before = len(YARDSTICK_LOG)
    try:
        yardstick(n(g), n(r32), n(r64), "")
        return None
    except AssertionError as e:
        return str(e).split("\n")[0]
    finally:
        del YARDSTICK_LOG[before:]


def backward_check(got, ref, bound, arch, ref32=None):
    """-> {group: [failure text]} for the groups grid (the grid's slice of the parameter gradient), coord (the seam's d x' and fc_final's
    gradient) and rest: every tensor within `bound` of its float64 scale (the ill-conditioned tensor at its own bound), and every grid
    entry that float64 leaves at exactly 0 exactly 0.  ``ref32`` (float32 autograd of the same reference on the same sides): the grid and
    coord tensors, which the grid kernels write or feed without a GEMM in between, are also held by conftest.yardstick at its default
    factors -- as close to float64 as float32 autograd is (max 3 x, rms 2 x, + 32 ulps of scale)."""
    errs = backward_errors(got, ref)
    fails = {"grid": [], "coord": [], "rest": []}
    for k, e in errs.items():
        if e > max(bound, BR.ILL_CONDITIONED.get((arch, k), 0.0)):
            fails[group_of(k)].append("%s %.3e of scale (bound %.1e)" % (k, e, bound))
    r, g = ref["spatial_embeddings"], got["spatial_embeddings"]
    stray = int(((r == 0) & (g != 0)).sum())
    if stray:
        fails["grid"].append("%d grid entries that float64 leaves at exactly 0 are not 0" % stray)
    if ref32 is not None:
        for k in ("spatial_embeddings",) + COORD_KEYS:
            src = "seam" if k == "seam_x" else k
            if got.get(src) is None or ref.get(src) is None:
                continue
            pick = (lambda t: t[:, 0:3]) if k == "seam_x" else (lambda t: t)
            said = _held32(pick(got[src]), pick(ref32[src]), pick(ref[src]))
            if said:
                fails[group_of(k)].append("%s, yardstick%s" % (k, said))
    return fails, errs
