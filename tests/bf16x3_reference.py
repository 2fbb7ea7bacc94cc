"""The split-operand (bf16x3) field kernels' arithmetic restated in eager torch, as the MEASURE of their per-sample float64 yardstick
(tests/test_gpu_bf16x3_samples.py on the GPU, tests/test_bf16x3_reference_host.py on the host).  TEST INFRASTRUCTURE ONLY; importing it
needs no GPU.

The expected value of every sample is oracle/torch_eager.py::EagerField in float64.  `Bf16x3Field` is the same network with the rounding
points of field_radiance_bf16x3_kernel and field_deform_bf16x3_kernel; its distance from float64 is what a correct kernel's distance is
measured with, exactly as tests/bf16_reference.py::Bf16Field measures the plain-bf16 kernel.  It is NOT an expected value: the kernel sums
its products in fp32 inside the MFMA, in an order of its own.

Rounding points (rounding=True), each with the line that makes it (csrc/ of the package):
 * weights: every layer of the stream (hidden layers and WF, HF, ALPHA, RGB, SEG) is stored as hi = bf16_rne(W), lo = bf16_rne(W - hi)
   (pack.hip:156-157, pack_stream_bf16x3_kernel; W - hi is exact in fp32);
 * the per-frame conditioning columns never reach the matrix pipe: fold_conditioning_kernel (pack.hip:189) multiplies them with the fp32
   weights and adds the sum to the fp32 bias, exactly as in Bf16Field.lin; the bias stays fp32 because it is the C operand of a tile's
   first MFMA (bf16x3_pipe.hpp:296, :312; the 16-row output tile: :387-397);
 * every sample-dependent input of a dense layer is split the same way where the layer reads it, x -> hi = bf16_rne(x),
   lo = bf16_rne(x - hi) (split_pair, bf16x3_pipe.hpp:73-77): the encodings with their raw coordinates (field_bf16x3.hip:85), the grid
   features (:148), the hidden activations and fc_feat's output, which has no activation (pack_tick stages C, D, E,
   bf16x3_pipe.hpp:185-198);
 * product: W_hi x_hi + W_hi x_lo + W_lo x_hi on one accumulator, W_lo x_lo dropped (dense_x, bf16x3_pipe.hpp:312-322; dense_x_out,
   :415-423).  Every term is a sum of exact products; they are summed here in float64 with the fp32 bias and the sum is rounded to fp32;
 * activation in fp32 BEFORE the split, FwdAct::value (bf16x3_pipe.hpp:83): max(v, m) with m = slope * v rounded to fp32 (pack_tick
   stage A, :177); slope 0 is ReLU, slope 1 passes v.  No bit-pattern form and no ops.bf16_exact_leaky here;
 * encodings (sin_rev, field_bf16x3.hip:46-52, from pe_blocks_x, :56-93): u = x / (2 pi) is held as an unevaluated fp32 pair, the
   product by 2^k and the reduction to a revolution are exact, then v_sin_f32.  The argument error is that of u, not 2^k times it: the
   sinusoids are modelled as sin(2^k x) of the fp32 x, evaluated in float64 and rounded to fp32; the raw coordinates pass unchanged (:79);
 * what stays fp32, unsplit: x' = x + tanhf(WF output) (field_bf16x3.hip:418-421) and w = HF output (:439-440) as written to xw and read
   back by the radiance kernel (:234-236); the trilinear lookup, accumulated in fp32 (grid_block_x, :116-141; its RESULT is split, :148);
   the final [rgb | seg | sigma] tile, the fp32 accumulators of the three output layers (:323-326).  The lookup is evaluated here in
   float64 and rounded to fp32 where fc layers_dir.0 reads it; tanh likewise.
rounding=False turns every one of them off and evaluates in float64: that instance must reproduce EagerField (host test).

mutant = (layer name, "no_wlo" | "no_xlo" | "hi_only") is a WRONG kernel, for the host test's proof that the rule sees one: in that layer
alone the term W_lo x_hi, W_hi x_lo, or both (plain bf16 operands) are left out.
"""
import numpy as np
import torch
import torch.nn.functional as F

import bf16_reference as BR
import field_reference as FR
from bf16_reference import bf16_round, r32, hold_to, line, separated, swap_partner, swapped, groups, tensors, conditioning, eager_f64, GROUPS  # noqa: F401

TILE, WAVE = 128, 32             # samples per workgroup tile, per wave (bf16x3_pipe.hpp: X_PTS_PER_WG, X_PTS_PER_WAVE)
SIZES = ((1, 1), (1, 33), (11, 7), (4, 32), (129, 1), (65, 13))      # N x S; the last is the main case
MAIN = (65, 13)
MUTANTS = ("no_wlo", "no_xlo", "hi_only")
assert (TILE, WAVE) == (FR.TILE["bf16x3"], FR.WAVE["bf16x3"])


def split(t):
    """split_pair: fp32 values (any float dtype) -> hi = bf16_rne(x), lo = bf16_rne(x - hi); x - hi is formed in fp32, where it is exact
    for every finite x whose hi is finite.  The two roundings are torch's own fp32 -> bfloat16 conversion, several times faster than
    bf16_reference.bf16_round on the bit patterns (the mutant sweep of the host test splits some 10^9 values); the host test holds both
    halves to bf16_round bit for bit"""
    f = t.to(torch.float32)
    hi = f.to(torch.bfloat16).to(torch.float32)
    lo = (f - hi).to(torch.bfloat16)
    return hi.to(t.dtype), lo.to(t.dtype)


_SPLIT = {}


def _split_weights(sd):
    """{name: (hi, lo)} of every dense layer's weight matrix, made once per state_dict (the mutant sweep builds hundreds of fields on one)"""
    if id(sd) not in _SPLIT or _SPLIT[id(sd)][0] is not sd:
        _SPLIT[id(sd)] = (sd, {k: split(v) for k, v in sd.items() if k.endswith(".weight") and v.dim() == 2})
    return _SPLIT[id(sd)][1]


# ---------------------------------------------------------------------------------------------------------------------------------
# the field
# ---------------------------------------------------------------------------------------------------------------------------------
class Bf16x3Field(BR.Bf16Field):
    """EagerField over float64 tensors with the split-operand kernels' rounding points (module docstring).  sd: float64 tensors of the
    fp32 state_dict.  The conditioning columns (Bf16Field.ncond) are folded into the bias as there."""

    def __init__(self, sd, n, arch, rounding=True, n_driving=76, mutant=None):
        super().__init__(sd, n, arch, rounding=False, n_driving=n_driving)      # (no plain-bf16 weight table)
        self.rounding, self.mutant = rounding, mutant
        assert mutant is None or (mutant[0] + ".weight" in sd and mutant[1] in MUTANTS), mutant
        self.sd_split = _split_weights(sd) if rounding else None
        self.evaluated = []                                                   # names of the dense layers a forward went through, in order

    def lin(self, name, x):
        self.evaluated.append(name)
        W, b = self.sd[name + ".weight"], self.sd[name + ".bias"]
        nc = self.ncond.get(name, 0)
        k = W.shape[1] - nc
        if nc:
            b = b + F.linear(x[:1, k:], W[:, k:])[0]
        if not self.rounding:
            return F.linear(x[:, :k], W[:, :k], b)
        (wh, wl), (xh, xl) = self.sd_split[name + ".weight"], split(x[:, :k])
        kind = self.mutant[1] if self.mutant is not None and self.mutant[0] == name else None
        acc = F.linear(xh, wh[:, :k], r32(b))
        if kind not in ("no_xlo", "hi_only"):
            acc = acc + F.linear(xl, wh[:, :k])
        if kind not in ("no_wlo", "hi_only"):
            acc = acc + F.linear(xh, wl[:, :k])
        return r32(acc)

    def act(self, name, x, slope):
        if not self.rounding:
            return super().act(name, x, slope)
        if slope == 0.0:
            return torch.relu(x)
        return torch.maximum(x, r32(x * float(np.float32(slope))))

    def encode(self, x, L, include_input=True):
        if not self.rounding:
            return super().encode(x, L, include_input)
        x = r32(x)
        out = [x] if include_input else []
        for k in range(L):
            out += [r32(torch.sin(x * 2.0 ** k)), r32(torch.cos(x * 2.0 ** k))]
        return torch.cat(out, dim=-1)


def evaluate(sd, arch, level, x6, driving, pose36, rounding, given=None, mutant=None, layers=None):
    """The field on the rows x6 (P, 6) = [point | direction] -> dict of float64 tensors raw (P, 16), xp (P, 3), and with deformation nets
    dx (P, 3) = x' - x, w (P, AMB_DIM).  rounding=False: float64 throughout (= EagerField).  rounding=True: x' is the fp32 number the
    deformation kernel writes to xw, and dx what a reader of xw finds, x' - x.  given = (x' (P, 3), w (P, AMB_DIM) or None): the radiance
    nets at that seam; dx and w are then not returned.  layers: a list that receives the names of the dense layers evaluated."""
    x = x6.to(torch.float64)
    field = Bf16x3Field(sd, x.shape[0], arch, rounding=rounding, n_driving=driving.shape[-1], mutant=mutant)
    taps = {}
    g = None if given is None else dict(warped=given[0].to(torch.float64), amb=None if given[1] is None else given[1].to(torch.float64))
    with torch.no_grad():
        raw = field.forward("coarse" if level == 0 else "fine", x, None, None, driving=driving.to(torch.float64), pose36=pose36.to(torch.float64),
                            taps=taps, given=g)
    if layers is not None:
        layers += field.evaluated
    out = dict(raw=raw, xp=taps.get("warped", x[:, :3] if g is None else g["warped"]))
    if "warped" in taps and given is None:
        if rounding:
            out["xp"] = r32(out["xp"])
        out["dx"], out["w"] = out["xp"] - x[:, :3], taps["amb"]
    return out


def layer_names(arch, level):
    """-> (deformation layers, radiance layers) of `level`, in evaluation order: every dense layer a forward goes through"""
    a = BR.TE.EagerField.ARCH[arch]
    p = "nerf_mlps.%s." % ("coarse" if level == 0 else "fine")
    deform = []
    if a["deform"]:
        deform = (["warp_field_mlp.layers_xyz.%d" % i for i in range(6)] + ["warp_field_mlp.fc_final"]
                  + ["hyper_sheep_mlp.layers_ambient.%d" % i for i in range(6)] + ["hyper_sheep_mlp.fc_ambient"])
    radiance = ([p + "layers_xyz.%d" % i for i in range(a["layers"])] + [p + "fc_feat", p + "fc_alpha"] + [p + "layers_dir.%d" % i for i in range(4)]
                + [p + "fc_rgb"] + [p + "layers_seg.%d" % i for i in range(4)] + [p + "fc_seg"])
    return deform, radiance


def judged_on(name):
    """the tensors a layer's mutant can move, at the seam the layer belongs to: a warp-field layer dx, a hyper-sheet layer w, a radiance
    layer sigma, rgb, seg (the trunk and fc_feat all three, fc_alpha sigma, the branches their own)"""
    if name.startswith("warp_field_mlp"):
        return ("dx",)
    if name.startswith("hyper_sheep_mlp"):
        return ("w",)
    tail = name.split(".", 2)[2]
    return {"fc_alpha": ("sigma",), "fc_rgb": ("rgb",), "fc_seg": ("seg",)}.get(tail, ("rgb",) if "dir" in tail else ("seg",) if "seg" in tail else ("sigma", "rgb", "seg"))


def points(rays, z):
    """The kernels' sample points: x = o + d z with TWO roundings, the product's and the sum's (field_bf16x3.hip:240, :398:
    rp[i] + rp[3 + i] * z, and build.py compiles with -ffp-contract=off, so no fused multiply-add is formed) -> x6 (N * S, 6) fp32 =
    [point | direction].  A fused form differs in the last bit of most z coordinates, which the NeRFaceModel's 15-octave encoding
    amplifies by 2^14: the GPU test asserts that these are the kernels' points, bit for bit, on the saved encoding planes, whose first
    three columns are the raw coordinates."""
    N, S = z.shape
    assert rays.dtype == torch.float32 and z.dtype == torch.float32
    product = rays[:, None, 3:6] * z[..., None]           # (two statements: one rounded fp32 operation each)
    x = rays[:, None, 0:3] + product
    return torch.cat([x, rays[:, None, 3:6].expand(N, S, 3)], -1).reshape(N * S, 6)


# ---------------------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------------------
def edge_rows(P):
    """the last 32 samples, the first and the last sample of every 32-sample wave of the last tile, the first row of every tile"""
    tiles = -(-P // TILE)
    t0 = (tiles - 1) * TILE
    rows = set(range(max(0, P - WAVE), P)) | set(range(0, P, TILE))
    for w0 in range(t0, P, WAVE):
        rows |= {w0, min(P, w0 + WAVE) - 1}
    return np.array(sorted(rows), np.int64)


def errors(emu, ref64):
    """(max, rms) of |emulation - float64|"""
    e = (emu.double() - ref64.double()).abs()
    return float(e.max()), float((e ** 2).mean().sqrt())


def allowance(emu, ref64, factor_max=3.0, ulps=32.0):
    """the largest |got - float64| conftest.yardstick accepts with its defaults, and its two terms: (3 emu_max + eps, emu_max, eps)"""
    emax = errors(emu, ref64)[0]
    eps = ulps * 2.0 ** -24 * float(ref64.abs().max())
    return factor_max * emax + eps, emax, eps


# ---------------------------------------------------------------------------------------------------------------------------------
# negative controls (values only); (a) is bf16_reference.swapped with bf16_reference.swap_partner's row
# ---------------------------------------------------------------------------------------------------------------------------------
def stale(raw):
    """control (b): row P-1 copied over row P-129 (a whole tile back)"""
    return FR.stale_row(raw, TILE)


def nudged(raw, ref64, emu, row, col=0):
    """control (c): colour logit `col` of sample `row` moved away from float64 by twice the rule's own allowance for the rgb tensor,
    2 x (3 emu_max + eps) -- not bf16_reference.nudged's 6 x emu_max, which is inside the allowance wherever the 32-ulp term leads"""
    raw, ref64, emu = raw.reshape(-1, 16), ref64.reshape(-1, 16), emu.reshape(-1, 16)
    allow = allowance(emu[:, 0:3], ref64[:, 0:3])[0]
    out = raw.clone()
    sign = 1.0 if float(raw[row, col]) >= float(ref64[row, col]) else -1.0
    out[row, col] = raw[row, col] + sign * 2.0 * allow
    return out
