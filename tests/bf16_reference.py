"""The plain-bf16 field kernel's arithmetic restated in eager torch, as the MEASURE of its per-sample float64 yardstick
(tests/test_gpu_bf16_samples.py on the GPU, tests/test_bf16_reference_host.py on the host).  TEST INFRASTRUCTURE ONLY; importing it needs
no GPU.

The expected value of every sample is oracle/torch_eager.py::EagerField in float64.  `Bf16Field` is the same network with the rounding
points of field_forward_bf16w_kernel (csrc/field_bf16w.hip, csrc/bf16_pipe.hpp, csrc/sahs_layout.hpp namespace hb, csrc/pack.hip); its
distance from float64 is what a correct bf16 kernel's distance is measured with, exactly as the reference's fp32 run measures the fp32
kernels in conftest.yardstick.  It is NOT an expected value: the kernel sums its products in fp32 inside the MFMA, in an order of its own.

Rounding points (rounding=True):
 * weights: every layer of the stream (hidden layers and the five output layers WF, HF, ALPHA, RGB, SEG) is rounded to bf16, round to
   nearest even, once (pack.hip: f32_to_bf16_rne);
 * the per-frame conditioning columns (driving vector, pose encoding) never reach the matrix pipe: fold_conditioning_kernel multiplies them
   with the fp32 weights and adds the sum to the fp32 bias, which is the initial value of every accumulator chain;
 * every sample-dependent input of a dense layer is rounded to bf16 where the layer reads it: encodings (raw coordinates included), grid
   features, hidden activations, and fc_feat's output (no activation), which feeds fc_alpha and both branches;
 * products of bf16 values are exact; they are summed here in float64 and the sum is rounded to fp32 (the kernel: fp32 MFMA accumulation);
 * ReLU (deformation nets): bf16(max(v, 0)).  LeakyReLU (radiance nets), default form: v is rounded to bf16, then K = 850 is subtracted
   from a negative BIT PATTERN, saturating at -0.0 (pack_tick: v_pk_mad_i16 ... clamp); exact form (ops.bf16_exact_leaky): max(v, 0.01f v)
   in fp32, then rounded;
 * encodings: sin(2 pi fract(fp32(x * fp32(1 / 2 pi)) * 2^k + phase)), phase 0.25 for the cosine, in fp32 (v_fract_f32, v_sin_f32 take
   revolutions), i.e. the argument carries the fp32 rounding of x / 2 pi amplified by 2^k;
 * x' = x + tanh(WF output) and w = HF output stay fp32, as does the final [rgb | seg | sigma] tile; the trilinear grid lookup is fp32.
rounding=False turns every one of them off and evaluates in float64: that instance must reproduce EagerField (host test).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import field_reference as FR
from oracle import torch_eager as TE

LEAKY_K = 850                    # round(128 log2(1 / 0.01)): pack_tick's constant, in both halves of 0x03520352
TILE, HALF = 256, 32             # samples per workgroup tile, per half of a wave (field_bf16w.hip: W_PTS_PER_WG, 32 * NH with NH = 2)
SIZES = ((1, 1), (1, 33), (11, 7), (4, 64), (257, 1), (65, 13))      # N x S; the last is the main case
MAIN = (65, 13)
GROUPS = (("sigma", slice(15, 16)), ("rgb", slice(0, 3)), ("seg", slice(3, 15)))      # raw's tensors: [rgb 3 | seg 12 | sigma]


# ---------------------------------------------------------------------------------------------------------------------------------
# roundings
# ---------------------------------------------------------------------------------------------------------------------------------
def _patterns(t):
    """fp32 bit patterns as non-negative int64"""
    return t.to(torch.float32).contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def _from_patterns(u, like):
    u = torch.where(u >= 2 ** 31, u - 2 ** 32, u).to(torch.int32)
    return u.view(torch.float32).to(like.dtype)


def r32(t):
    """round to fp32, keep the dtype"""
    return t.to(torch.float32).to(t.dtype)


def bf16_round(t):
    """fp32 -> bf16, round to nearest even, on the bit pattern; NaN stays NaN.  `t` holds fp32 values in any float dtype; so does the result."""
    u = _patterns(t)
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    out = _from_patterns(r, t)
    return torch.where(torch.isnan(t), t, out)


def leaky_pattern(t):
    """pack_tick's default LeakyReLU on bf16 values: a negative value's pattern (sign bit set = a negative int16 whose low 15 bits grow with
    the magnitude) loses K = 850, saturating at int16 min = -0.0; positive patterns and +-0 pass."""
    u = _patterns(t)
    assert bool(((u & 0xFFFF) == 0).all()), "leaky_pattern takes bf16 values"
    mag = (u >> 16) & 0x7FFF
    neg = (u >> 31) & 1
    mag = torch.where(neg == 1, torch.clamp(mag - LEAKY_K, min=0), mag)
    return _from_patterns(((neg << 15) | mag) << 16, t)


def leaky_exact(t):
    """max(v, 0.01f v) in fp32, then bf16"""
    slope = float(np.float32(0.01))
    return bf16_round(torch.maximum(t, r32(t * slope)))


# ---------------------------------------------------------------------------------------------------------------------------------
# the field
# ---------------------------------------------------------------------------------------------------------------------------------
class Bf16Field(TE.EagerField):
    """EagerField over float64 tensors with the bf16 kernel's rounding points (module docstring).  sd: float64 tensors of the fp32
    state_dict.  n_driving: length of the driving vector (the conditioning columns are the trailing ones of every layer that has any)."""

    def __init__(self, sd, n, arch, rounding=True, exact_leaky=False, n_driving=76):
        super().__init__(sd, num_coarse=n, num_fine=0, arch=arch)
        self.rounding, self.exact_leaky = rounding, exact_leaky
        self.sd_bf16 = {k: bf16_round(v) for k, v in sd.items() if k.endswith(".weight") and v.dim() == 2} if rounding else None
        deform, trunk = n_driving + 36, (36 if self.a["trunk_pose"] else n_driving)
        self.ncond = {"warp_field_mlp.layers_xyz.0": deform, "warp_field_mlp.layers_xyz.4": deform,
                      "hyper_sheep_mlp.layers_ambient.0": deform, "hyper_sheep_mlp.layers_ambient.4": deform}
        for lvl in ("coarse", "fine"):
            self.ncond["nerf_mlps.%s.layers_xyz.0" % lvl] = trunk
            self.ncond["nerf_mlps.%s.layers_xyz.3" % lvl] = trunk

    def lin(self, name, x):
        W, b = self.sd[name + ".weight"], self.sd[name + ".bias"]
        nc = self.ncond.get(name, 0)
        k = W.shape[1] - nc
        if nc:      # the fold: fp32 weights x the frame's conditioning vector (every row of x carries the same one), into the bias
            b = b + F.linear(x[:1, k:], W[:, k:])[0]
        if not self.rounding:
            return F.linear(x[:, :k], W[:, :k], b)
        return r32(F.linear(bf16_round(x[:, :k]), self.sd_bf16[name + ".weight"][:, :k], r32(b)))

    def act(self, name, x, slope):
        if not self.rounding:
            return super().act(name, x, slope)
        if slope == 0.0:
            return bf16_round(torch.relu(x))
        assert slope == 0.01
        return leaky_exact(x) if self.exact_leaky else leaky_pattern(bf16_round(x))

    def encode(self, x, L, include_input=True):
        if not self.rounding:
            return super().encode(x, L, include_input)
        x = r32(x)
        rev = r32(x * float(np.float32(0.15915494309189535)))
        out = [x] if include_input else []
        for k in range(L):
            for phase in (0.0, 0.25):
                t = r32(rev * 2.0 ** k + phase)
                out.append(r32(torch.sin(2.0 * math.pi * (t - torch.floor(t)))))
        return torch.cat(out, dim=-1)


def tensors(sd_np, device):
    return {k: torch.from_numpy(v).to(device, torch.float64) for k, v in sd_np.items()}


def evaluate(sd, arch, level, x6, driving, pose36, rounding, exact_leaky=False, given=None):
    """The field on the rows x6 (P, 6) = [point | direction] -> dict of float64 tensors raw (P, 16), xp (P, 3), and with deformation nets
    dx (P, 3) = x' - x, w (P, AMB_DIM).  rounding=False: float64 throughout (= EagerField).  given = (x' (P, 3), w (P, AMB_DIM) or None):
    the radiance nets at that seam; dx and w are then not returned."""
    x = x6.to(torch.float64)
    field = Bf16Field(sd, x.shape[0], arch, rounding=rounding, exact_leaky=exact_leaky, n_driving=driving.shape[-1])
    taps = {}
    g = None if given is None else dict(warped=given[0].to(torch.float64), amb=None if given[1] is None else given[1].to(torch.float64))
    with torch.no_grad():
        raw = field.forward("coarse" if level == 0 else "fine", x, None, None, driving=driving.to(torch.float64), pose36=pose36.to(torch.float64),
                            taps=taps, given=g)
    out = dict(raw=raw, xp=taps.get("warped", x[:, :3] if g is None else g["warped"]))
    if "warped" in taps and given is None:
        out["dx"], out["w"] = taps["warped"] - x[:, :3], taps["amb"]
    return out


def eager_f64(sd, arch, level, x6, driving, pose36, given=None):
    """oracle/torch_eager.py::EagerField itself in float64 (what rounding=False must reproduce) -> raw, and the taps when there are any"""
    x = x6.to(torch.float64)
    field = TE.EagerField(sd, num_coarse=x.shape[0], num_fine=0, arch=arch)
    taps = {}
    kw = {} if given is None else dict(given=dict(warped=given[0].to(torch.float64), amb=None if given[1] is None else given[1].to(torch.float64)))
    with torch.no_grad():
        raw = field.forward("coarse" if level == 0 else "fine", x, None, None, driving=driving.to(torch.float64), pose36=pose36.to(torch.float64),
                            taps=taps, **kw)
    return raw, taps


# ---------------------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------------------
def conditioning(weights_mod, arch, device):
    """-> sd (float64 tensors), driving vector, pose encoding of FR.driving_input / FR.pose_of, computed by EagerField in float64 and
    rounded to fp32 (the host's stand-in for the frame buffer of ops.fold_conditioning; the GPU test reads the frame's own)"""
    sd = tensors(FR.state_dict_np(weights_mod, arch), device)
    field = TE.EagerField(sd, arch=arch)
    inp = FR.driving_input(arch, device).to(torch.float64)
    with torch.no_grad():
        drv = field.audionet(inp) if arch == "audio" else inp
        p36 = field.pose_encoding(FR.pose_of(arch, device).to(torch.float64))[0]
    return sd, r32(drv), r32(p36)


# ---------------------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------------------
def edge_rows(P):
    """the last 64 samples, the first and the last sample of every 32-sample half of the last tile, the first row of every tile"""
    tiles = -(-P // TILE)
    t0 = (tiles - 1) * TILE
    rows = set(range(max(0, P - 64), P)) | set(range(0, P, TILE))
    for h0 in range(t0, P, HALF):
        rows |= {h0, min(P, h0 + HALF) - 1}
    return np.array(sorted(rows), np.int64)


def groups(raw):
    """raw (P, 16) -> [(name, (P, k) tensor)]: sigma, rgb logits, seg logits"""
    raw = raw.reshape(-1, 16)
    return [(name, raw[:, sl]) for name, sl in GROUPS]


def hold_to(got, ref64, emu_max, emu_rms, what, factor=2.0, factor_max=3.0, ulps=32.0):
    """conftest.yardstick's rule with a BORROWED measure (the main case's emulation errors), for the sizes whose own few values give no
    maximum: max |got - f64| <= 3 emu_max + eps, rms <= 2 emu_rms + eps, eps = 32 fp32 ulps of the tensor's largest magnitude."""
    n = lambda a: np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, np.float64)
    got, ref64 = n(got), n(ref64)
    assert np.isfinite(got).all(), what + ": not finite"
    e = np.abs(got.reshape(ref64.shape) - ref64)
    eps = ulps * 2.0 ** -24 * float(np.abs(ref64).max())
    rec = (what, float(e.max()), float(emu_max), float(np.sqrt((e ** 2).mean())), float(emu_rms), float(np.abs(ref64).max()))
    assert rec[1] <= factor_max * emu_max + eps, "%s: max |got - f64| = %.3e, the main case's emulation: %.3e" % (what, rec[1], emu_max)
    assert rec[3] <= factor * emu_rms + eps, "%s: rms |got - f64| = %.3e, the main case's emulation: %.3e" % (what, rec[3], emu_rms)
    return rec


def line(rec):
    """one row of the printed table: how far the kernel's worst sample is from float64, and the emulation's"""
    what, e, r, er, rr, sc = rec
    return "  %-58s max %.3e (emulation %.3e, ratio %5.2f)  rms %.3e (emulation %.3e, ratio %5.2f)  scale %.2e" % (
        what, e, r, e / r if r else float("inf"), er, rr, er / rr if rr else float("inf"), sc)


# ---------------------------------------------------------------------------------------------------------------------------------
# negative controls (values only)
# ---------------------------------------------------------------------------------------------------------------------------------
def separated(ref64, emu, a, b, times=10.0):
    """-> the columns of raw in which the float64 rows a and b differ by more than `times` x the emulation's max error of that column's
    tensor group (sigma | rgb | seg), as [(group name, column)]"""
    ref64, emu = ref64.reshape(-1, 16), emu.reshape(-1, 16)
    out = []
    for name, sl in GROUPS:
        emax = float((emu[:, sl] - ref64[:, sl]).abs().max())
        d = (ref64[a, sl] - ref64[b, sl]).abs()
        out += [(name, sl.start + int(c)) for c in torch.nonzero(d > times * emax).reshape(-1)]
    return out


def swap_partner(ref64, emu, N, S):
    """control (a): the row nearest to P-1 that belongs to another ray and is separated from row P-1 (None when there is none)"""
    P = N * S
    for r in range(P - S - 1, -1, -1):
        if separated(ref64, emu, P - 1, r):
            return r
    return None


def swapped(raw, a, b):
    out = raw.clone()
    out[a], out[b] = raw[b], raw[a]
    return out


def stale(raw):
    """control (b): row P-1 copied over row P-257 (a whole tile back)"""
    return FR.stale_row(raw, TILE)


def nudged(raw, ref64, emu, row, col=0):
    """control (c): 6 x the emulation's max error of the rgb tensor added to colour logit `col` of sample `row`, away from float64"""
    raw, ref64, emu = raw.reshape(-1, 16), ref64.reshape(-1, 16), emu.reshape(-1, 16)
    emax = float((emu[:, 0:3] - ref64[:, 0:3]).abs().max())
    out = raw.clone()
    sign = 1.0 if float(raw[row, col]) >= float(ref64[row, col]) else -1.0
    out[row, col] = raw[row, col] + sign * 6.0 * emax
    return out
