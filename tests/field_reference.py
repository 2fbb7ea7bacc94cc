"""Shared pieces of the field kernels' tile tests (tests/test_gpu_field_tiles.py on the GPU, tests/test_field_reference_host.py on the
host).  TEST INFRASTRUCTURE ONLY; importing it needs no GPU.

The field kernels are persistent: a launch over T tiles starts min(T, CUs) workgroups and workgroup g walks tiles g, g + CUs, ...  The
tests evaluate one LARGE launch, in which workgroups run two and three tiles, and the same rays again in SMALL launches of at most half a
round (every workgroup at most one tile), and require the two to agree bit for bit: the field is pointwise.

 * plan / factor / ragged_remainder: the sample counts on the edges of a round, and their (rays, samples per ray) factoring.
 * build_scene / ray_slices: one frame's rays and depths per architecture, and the ragged ray slices of the small launches.
 * act_table / bits_table / plane / decode_sign_bits / reassemble_planes: the saved-activation and sign-bit planes of a saving forward
   (csrc/sahs_layout.hpp, namespaces act and sbits, restated).
 * edge_rows / eager_field / held / would_fail: the float64 yardstick of the fp32 kernels over a whole launch and over its edge rows.
 * same_bits / first_difference: the bitwise comparators (buffers with NaN sentinels compare through an int32 view).
"""
import numpy as np
import torch

TILE = {"fp32": 128, "bf16": 256, "bf16x3": 128}       # samples per workgroup tile
WAVE = {"fp32": 16, "bf16": 64, "bf16x3": 32}          # samples per wave
SIZES = ("one_past", "two_rounds", "ragged_third")
S_MAX = 192
CHUNK = 32768                                          # samples per eager evaluation


# ---------------------------------------------------------------------------------------------------------------------------------
# sizes
# ---------------------------------------------------------------------------------------------------------------------------------
def ragged_remainder(tile, wave):
    """Samples of a ragged last tile: 77 where that leaves a partly filled wave which is not the first (fp32: four whole waves and 13
    samples in the fifth; bf16x3: two and 13 in the third; bf16: one and 13 in the second), otherwise the next count that does."""
    r = 77
    while not (r < tile and r % wave != 0 and r // wave >= 1):
        r += 1
        assert r < tile, "no ragged remainder for tile %d, wave %d" % (tile, wave)
    return r


def factor(P):
    """P = N x S with S the largest divisor of P in 2..192 (1 only when there is none)."""
    S = next((s for s in range(min(S_MAX, P), 1, -1) if P % s == 0), 1)
    return P // S, S


def plan(cus, precision, size):
    """The launch of `size` on a device with `cus` compute units -> dict: P, (N, S), tiles, tiles of the busiest and the idlest workgroup,
    how many workgroups run the busiest count, the last tile's samples, its first partly filled wave."""
    tile, wave = TILE[precision], WAVE[precision]
    R = cus * tile
    P = {"one_past": R + 1, "two_rounds": 2 * R, "ragged_third": 2 * R + tile + ragged_remainder(tile, wave)}[size]
    N, S = factor(P)
    tiles = -(-P // tile)
    most, least = -(-tiles // cus), tiles // cus
    rem = P - (tiles - 1) * tile
    return dict(P=P, N=N, S=S, tile=tile, wave=wave, cus=cus, tiles=tiles, most=most, least=least,
                busiest=(tiles - least * cus) if most > least else min(cus, tiles),        # workgroups 0 .. busiest-1 run `most` tiles
                last_tile_samples=rem, partial_wave=(rem // wave if rem % wave else None))


def describe(pl):
    who = ("every workgroup runs %d tiles" % pl["most"] if pl["most"] == pl["least"]
           else "workgroups 0..%d run %d tiles, the others %d" % (pl["busiest"] - 1, pl["most"], pl["least"]))
    return ("P=%d (N=%d x S=%d), %d tiles of %d on %d CUs: %s; the last tile holds %d samples"
            % (pl["P"], pl["N"], pl["S"], pl["tiles"], pl["tile"], pl["cus"], who, pl["last_tile_samples"]))


def ray_slices(N, S, cus, tile):
    """Ray ranges [(n0, n1)] of the small launches: each at most half a round of samples (so that every workgroup runs at most one tile),
    of varying length (m, m - 1, m - 2 rays in turn) so that slice boundaries fall inside tiles wherever S is no multiple of the tile."""
    m = (cus * tile // 2) // S
    assert m >= 1, "a ray of %d samples exceeds half a round (%d CUs x %d)" % (S, cus, tile)
    out, n0, i = [], 0, 0
    while n0 < N:
        n1 = min(N, n0 + max(1, m - i % 3))
        out.append((n0, n1))
        n0, i = n1, i + 1
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# scenes (rays and depths per architecture as in tests/test_gpu_backward_tails.py::_setup)
# ---------------------------------------------------------------------------------------------------------------------------------
SCENE = {"audio": dict(near=0.48, far=1.08, cam=0.8), "nerface": dict(near=0.2, far=0.8, cam=0.5), "nerface_static": dict(near=0.2, far=0.8, cam=0.5)}


def state_dict_np(weights_mod, arch):
    """the hdr weights for the AudioFaceModel, the density-boosted ones for the NeRFaceModels"""
    if arch == "audio":
        return weights_mod.hash_state_dict(0, 2.0, 30.0, hdr=True)
    return weights_mod.hash_state_dict(0, 8.0, 30.0, model=arch)


def driving_input(arch, device, seed=5):
    gen = torch.Generator(device=device).manual_seed(seed)
    if arch == "audio":
        return torch.randn(16, 29, device=device, generator=gen)
    return torch.randn(76, device=device, generator=gen) * 0.5


def pose_of(arch, device):
    return torch.from_numpy(np.concatenate([np.eye(3), [[0.0], [0.0], [SCENE[arch]["cam"]]]], 1).astype(np.float32)).to(device)


def build_scene(arch, N, S, device):
    """-> rays (N, 8), z (N, S) sorted along the ray, x6 (N * S, 6) = [point | direction]"""
    sc = SCENE[arch]
    gen = torch.Generator(device=device).manual_seed(1000 * N + S)
    rays = torch.zeros(N, 8, device=device)
    rays[:, 2] = sc["cam"]
    rays[:, 3:6] = torch.randn(N, 3, device=device, generator=gen) * 0.15 + torch.tensor([0, 0, -1.0], device=device)
    rays[:, 6], rays[:, 7] = sc["near"], sc["far"]
    z = torch.sort(torch.rand(N, S, device=device, generator=gen) * (sc["far"] - sc["near"]) + sc["near"], dim=1).values
    x6 = torch.cat([rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None], rays[:, None, 3:6].expand(N, S, 3)], -1).reshape(N * S, 6)
    return rays, z, x6


def ray_permutation(N, S, device, seed=3):
    """(N, S) int32: a random permutation of 0..S-1 per ray (the identity only where S == 1)"""
    gen = torch.Generator(device=device).manual_seed(seed)
    return torch.argsort(torch.rand(N, S, device=device, generator=gen), dim=1).to(torch.int32).contiguous()


# ---------------------------------------------------------------------------------------------------------------------------------
# saved planes (csrc/sahs_layout.hpp restated: one dense [P x width] plane per layer at float column * P)
# ---------------------------------------------------------------------------------------------------------------------------------
ARCH_DIMS = {"audio": dict(kbx=4, kba=2, trunk=8, amb=2, deform=True), "nerface": dict(kbx=6, kba=2, trunk=4, amb=1, deform=True),
             "nerface_static": dict(kbx=4, kba=0, trunk=4, amb=0, deform=False)}
FIELD_ALL, FIELD_DEFORM, FIELD_RADIANCE = 0, 1, 2


def act_table(arch):
    """[(name, column, width, defined columns, part, sign-plane name or None)] in column order, and the row stride.  `defined`: the
    columns the forward writes (dx, w, x' are 3 / AMB_DIM / 3 values in a 16-wide plane whose pad the kernel leaves alone; an
    architecture without deformation nets writes none of the deformation planes)."""
    d = ARCH_DIMS[arch]
    dd = d["deform"]
    rows, c = [], 0

    def add(name, width, defined, part, sign=None):
        nonlocal c
        rows.append((name, c, width, defined, part, sign))
        c += width

    add("pe_x", 16 * d["kbx"], 16 * d["kbx"] if dd else 0, FIELD_DEFORM)
    for i in range(6):
        add("warp.%d" % i, 128, 128 if dd else 0, FIELD_DEFORM, "warp.%d" % i if dd else None)
    add("dx", 16, 3 if dd else 0, FIELD_DEFORM)
    for i in range(6):
        add("hyper.%d" % i, 64, 64 if dd else 0, FIELD_DEFORM, "hyper.%d" % i if dd else None)
    add("w", 16, d["amb"], FIELD_DEFORM)
    add("xw", 16, 3, FIELD_RADIANCE)          # (the deformation part's range ends behind it: both parts hold the warped point)
    add("pe_xw", 16 * d["kbx"], 16 * d["kbx"], FIELD_RADIANCE)
    add("pe_w", 16 * d["kba"], 16 * d["kba"], FIELD_RADIANCE)
    for i in range(d["trunk"]):
        add("trunk.%d" % i, 256, 256, FIELD_RADIANCE, "trunk.%d" % i)
    add("feat", 256, 256, FIELD_RADIANCE)
    add("dir", 32, 32, FIELD_RADIANCE)
    add("grid", 32, 32, FIELD_RADIANCE)
    for i in range(4):
        add("dir.%d" % i, 128, 128, FIELD_RADIANCE, "dir.%d" % i)
    for i in range(4):
        add("seg.%d" % i, 128, 128, FIELD_RADIANCE, "seg.%d" % i)
    return rows, c


def act_words(arch, part):
    """floats per sample of a save of `part`: whole network [0, STRIDE); deformation nets [0, XW + 16); radiance nets [XW, STRIDE)"""
    rows, stride = act_table(arch)
    xw = next(r[1] for r in rows if r[0] == "xw")
    return {FIELD_ALL: stride, FIELD_DEFORM: xw + 16, FIELD_RADIANCE: stride - xw}[part]


def act_col0(arch, part):
    rows, _ = act_table(arch)
    return next(r[1] for r in rows if r[0] == "xw") if part == FIELD_RADIANCE else 0


def sign_words(width):
    """32-bit words per sample of one layer's sign plane: 4 lane quarters x NW, NW = width / 128, at least 1"""
    return 4 * ((width // 16 + 7) // 8)


def bits_table(arch):
    """{sign-plane name: (word column in a WHOLE-network bits buffer, width)} and the words per sample of (whole, deformation, radiance):
    [deformation planes][radiance planes], a plane of word column b at word b * P of its part"""
    d = ARCH_DIMS[arch]
    out, b = {}, 0
    if d["deform"]:
        for i in range(6):
            out["warp.%d" % i] = (b, 128)
            b += sign_words(128)
        for i in range(6):
            out["hyper.%d" % i] = (b, 64)
            b += sign_words(64)
    bd = b
    for name, n, width in (("trunk", d["trunk"], 256), ("dir", 4, 128), ("seg", 4, 128)):
        for i in range(n):
            out["%s.%d" % (name, i)] = (b, width)
            b += sign_words(width)
    return out, (b, bd, b - bd)


def plane(buf, P, column, width):
    """the [P x width] plane at `column` of a flat save of P samples (a view)"""
    flat = buf.reshape(-1)
    return flat[column * P:(column + width) * P].view(P, width)


def decode_sign_bits(bits, P, word_col, width):
    """(P, width) bool from a sign plane: [P][4 q][NW] words; the lane quarter q that holds features 16 t + 4 q + r of 16-row tile t sets
    bit 4 (t % 8) + r of its word t // 8 (the layout comment above namespace sbits)"""
    nw = max(1, width // 128)
    words = plane(bits, P, word_col, 4 * nw).view(P, 4, nw)
    f = torch.arange(width, device=bits.device)
    t, q, r = f // 16, (f % 16) // 4, f % 4
    return ((words[:, q, t // 8] >> (4 * (t % 8) + r)) & 1).bool()


def encode_sign_bits(positive):
    """the inverse (host tests): (P, width) bool -> (P, 4 * NW) int32 sign plane"""
    P, width = positive.shape
    nw = max(1, width // 128)
    words = np.zeros((P, 4, nw), np.uint32)
    for f in range(width):
        t, q, r = f // 16, (f % 16) // 4, f % 4
        words[:, q, t // 8] |= positive[:, f].astype(np.uint32) << np.uint32(4 * (t % 8) + r)
    return words.reshape(P, 4 * nw).view(np.int32)


def stacked_plane(parts, Ps, column, width):
    """plane (column, width) of the large save, re-assembled from the small saves `parts` of Ps[i] samples each"""
    return torch.cat([plane(p, Pi, column, width) for p, Pi in zip(parts, Ps)], 0)


def reassemble_planes(parts, widths):
    """Small saves -> the large one.  parts: flat plane buffers of P_i samples each (every plane [P_i x width], the planes back to back
    in the order of `widths`); returns the flat buffer of sum P_i samples with the same planes: plane k = the parts' planes k stacked."""
    Ps = [p.numel() // sum(widths) for p in parts]
    out, col = [], 0
    for w in widths:
        out.append(stacked_plane(parts, Ps, col, w).reshape(-1))
        col += w
    return torch.cat(out)


# ---------------------------------------------------------------------------------------------------------------------------------
# comparators
# ---------------------------------------------------------------------------------------------------------------------------------
def as_bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def same_bits(a, b):
    """bit for bit, NaN sentinels included"""
    return a.shape == b.shape and bool(torch.equal(as_bits(a), as_bits(b)))


def first_difference(a, b):
    """-> (count of differing elements, flat index of the first, its row when the tensors are 2-D or more) for the failure message"""
    d = (as_bits(a) != as_bits(b)).reshape(-1)
    n = int(d.sum())
    if n == 0:
        return 0, None, None
    i = int(torch.nonzero(d)[0])
    return n, i, i // max(1, int(np.prod(a.shape[1:])))


def assert_same_bits(a, b, what):
    if not same_bits(a, b):
        assert a.shape == b.shape, "%s: shapes %s / %s" % (what, tuple(a.shape), tuple(b.shape))
        n, i, row = first_difference(a, b)
        raise AssertionError("%s: %d of %d elements differ bitwise, the first at flat index %d (row %d)" % (what, n, a.numel(), i, row))


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 yardstick over a launch's edge rows
# ---------------------------------------------------------------------------------------------------------------------------------
def edge_rows(P, cus, tile):
    """the last two tiles, the first tile of every workgroup round (tiles 0, CUs, 2 CUs, ...), the last 16 samples"""
    tiles = -(-P // tile)
    want = {tiles - 1, max(0, tiles - 2)} | set(range(0, tiles, cus))
    rows = set(range(max(0, P - 16), P))
    for t in want:
        rows |= set(range(t * tile, min(P, (t + 1) * tile)))
    return np.array(sorted(rows), np.int64)


def eager_field(sd_np, arch, level, x6, driving, pose36, dtype, chunk=CHUNK):
    """oracle/torch_eager.py::EagerField on x6's device in `dtype`, `chunk` samples at a time, with the frame's own conditioning vectors
    -> dict raw (P, 16), xp (P, 3) the warped point, dx (P, 3) = xp - x, w (P, AMB_DIM), grid (P, 32); dx and w are None without
    deformation nets"""
    from oracle import torch_eager as TE
    dev = x6.device
    sd = {k: torch.from_numpy(v).to(dev, dtype) for k, v in sd_np.items()}
    drv, p36 = driving.to(dtype), pose36.to(dtype)
    lvl = "coarse" if level == 0 else "fine"
    out = dict(raw=[], xp=[], dx=[], w=[], grid=[])
    with torch.no_grad():
        for s in range(0, x6.shape[0], chunk):
            x = x6[s:s + chunk].to(dtype)
            field = TE.EagerField(sd, num_coarse=x.shape[0], num_fine=0, arch=arch)
            taps = {}
            out["raw"].append(field.forward(lvl, x, None, None, driving=drv, pose36=p36, taps=taps))
            warped = taps.get("warped", x[:, :3])
            out["grid"].append(field.grid(lvl, warped))
            out["xp"].append(warped)
            if "warped" in taps:
                out["dx"].append(warped - x[:, :3])
                out["w"].append(taps["amb"])
    return {k: (torch.cat(v) if v else None) for k, v in out.items()}


def held(got, ref32, ref64, what, rows=None):
    """conftest.yardstick with its defaults (rms 2x, max 3x, 32 ulps), over all rows or over `rows`; raises AssertionError, returns the
    record (what, max err, reference's max err, rms err, reference's rms err, scale)"""
    from conftest import yardstick
    pick = (lambda a: a) if rows is None else (lambda a: a[rows])
    n = lambda a: pick(a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a))
    return yardstick(n(got), n(ref32), n(ref64), what)


def would_fail(got, ref32, ref64, rows):
    """whether held() rejects `got` on `rows`; leaves no line in the session's yardstick log"""
    from conftest import YARDSTICK_LOG
    before = len(YARDSTICK_LOG)
    try:
        held(got, ref32, ref64, "sensitivity", rows)
        return False
    except AssertionError:
        return True
    finally:
        del YARDSTICK_LOG[before:]


def yardstick_bound(rec, factor_max=3.0, ulps=32.0):
    """the max-error bound a yardstick record was held to"""
    return factor_max * rec[2] + ulps * 2.0 ** -24 * rec[5]


def swap_last_two(a):
    """rows P-1 and P-2 swapped"""
    b = a.clone()
    b[-1], b[-2] = a[-2], a[-1]
    return b


def stale_row(a, tile):
    """row P-1 copied over row P - tile - 1 (a stale-buffer shape of error)"""
    b = a.clone()
    b[-tile - 1] = a[-1]
    return b
