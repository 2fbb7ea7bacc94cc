"""The feature-grid lookup and its backward at the grid's faces (the contract and the position sets: tests/grid_reference.py; the
instruments themselves are tested on the host, tests/test_grid_reference_host.py).

Every lookup -- grid_blocks (csrc/field_f32.hip), the two half-wave lookups (csrc/field_bf16w.hip, csrc/field_bf16x3.hip) -- and the
backward's grid_backward_kernel / grid_transpose_kernel (csrc/field_bwd.hip, from the per-layer and the fused walk) is run on positions
that reach it bit for bit: exactly on one, two and three faces; half a cell outside (four, six, seven corners outside); one to three
cells outside (no corner inside); far outside (4, 2^20, 2.98e38); runs of one cell across the backward's 16-sample chunks, a cell
change on every sample, P = 1 (mod 16); 512 samples piled into one cell.  The warp head's weights are zero, so x' = x exactly.

FORWARD, every architecture x every precision it has: the 32 features (debug planes; the whole-network save where a family has none;
the NeRFaceModel's bf16 chain has neither, there only raw and x' are seen) against float64 grid_sample by conftest.yardstick at its
default factors, float32 grid_sample on the device the measure; exactly 0.0 where no corner is inside.  raw (every set but far_out)
by the same yardstick against the float64 eager field, the float32 eager field the measure, for the kernels that evaluate the networks
in fp32 arithmetic; for bf16 / bf16x3 see RAW_FACTOR.
BACKWARD, fp32 GEMM arithmetic, every walk backward_reference._paths lists and the NeRFaceModels' fused walk, both levels: every gradient against float64 autograd on
the HIP forward's side of every kink, within the walk's bound in backward_reference.FIELD_BOUNDS, the grid slice and d x' (seam,
fc_final's gradient) also by the yardstick with float32 autograd of the same reference the measure; every grid-gradient entry float64
leaves at exactly 0 is exactly 0 (from a zeroed buffer) or keeps its bits (from a prefilled one); level 0 then level 1 into one
buffer gives the sum of the two references.

MEASURED on an MI355X, worst over levels, walks, forms and two runs (no case needed a bound of its own; the kernels were found right):
  features, max |HIP - float64| (float32 grid_sample's own), identical in the fp32, bf16 and bf16x3 families of an architecture; held to
  3 x the reference's + 32 ulps of scale (rms: 2 x):
    set        audio                   NeRFaceModels (both)
    faces      6.97e-08 (5.31e-08)     6.10e-08 (5.70e-08)
    half_out   2.31e-08 (2.31e-08)     2.37e-08 (2.37e-08)
    runs       7.13e-08 (7.13e-08)     8.46e-08 (8.46e-08)
    pile       9.96e-08 (9.96e-08)     1.01e-07 (1.01e-07)
    just_out, far_out: exactly 0.0 everywhere, the 2.98e38 rows whose x' the deforming architectures make NaN included
  raw, max error in units of the float32 eager field's own max error: fp32 kernels 1.3 - 5.5 (within 3 x + 32 ulps of scale); bf16x3
  19 - 33 (allowed 768); bf16 91 - 17,801 (allowed 196,608)
  backward, of the float64 tensor's scale: grid slice / d x' (seam or fc_final) / worst other tensor, and the bound held to
    set        audio (2e-4)                     nerface (3e-3; in brackets fc_ambient.bias, 5e-2)   nerface_static (1e-4)
    faces      6.5e-07 / 8.9e-07 / 2.3e-06      4.4e-07 / 1.5e-06 / 9.0e-04 (3.2e-03)      4.3e-07 / - / 5.1e-06
    half_out   6.8e-07 / 1.1e-06 / 3.0e-06      5.4e-07 / 1.9e-06 / 5.6e-04 (below it)     5.6e-07 / - / 2.0e-06
    just_out   exactly 0 / 1.7e-06 / 2.4e-06    exactly 0 / 1.5e-06 / 5.0e-04 (5.6e-04)    exactly 0 / - / 2.9e-06
    runs       3.6e-07 / 1.2e-06 / 1.0e-05      5.5e-07 / 3.1e-06 / 7.6e-04 (5.2e-03)      7.0e-07 / - / 2.3e-06
    pile       5.0e-07 / 3.8e-06 / 3.8e-06      5.8e-07 / 1.1e-06 / 1.2e-03 (2.1e-03)      6.6e-07 / - / 3.3e-06
    level 0 + level 1 into one buffer, grid slice: at most 6.6e-07 of the summed reference's scale
  Every grid entry float64 leaves at 0 (1,043,712 to 1,048,576 of 1,048,576) came out 0, and kept its bits in a prefilled buffer.
"""
import time

import numpy as np
import pytest
import torch

import backward_reference as BR
import field_reference as FR
import grid_reference as GR
from conftest import pkg, yardstick

pytestmark = pytest.mark.gpu

DEV = BR.DEV
ARCHS = ("audio", "nerface", "nerface_static")
PRECS = ("fp32", "bf16", "bf16x3")
_CACHE = {}


def model(arch):
    if arch not in _CACHE:
        ops, W = pkg("ops"), pkg("weights")
        sd_np = GR.edge_state_dict(W, arch)
        flat = torch.from_numpy(W.flatten_state_dict(sd_np, model=arch)).to(DEV)
        frame = ops.fold_conditioning(flat, FR.driving_input(arch, DEV), FR.pose_of(arch, DEV), arch=arch)
        _CACHE[arch] = dict(sd_np=sd_np, flat=flat, frame=frame, packs={}, refs={})
    return _CACHE[arch]


def pack(arch, prec):
    m, ops = model(arch), pkg("ops")
    if prec not in m["packs"]:
        m["packs"][prec] = ops.pack_weights(m["flat"], ops.PRECISIONS[prec], arch=arch)
    return m["packs"][prec]


def grid_plane(arch, act, P):
    col = next(r[1] for r in FR.act_table(arch)[0] if r[0] == "grid")
    return FR.plane(act, P, col, 32)


def xw_plane(arch, act, P):
    col = next(r[1] for r in FR.act_table(arch)[0] if r[0] == "xw")
    return FR.plane(act, P, col, 16)[:, :3]


# ---------------------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------------------
def forward_taps(arch, prec, level, rays, z):
    """-> dict raw (P, 16), feats (P, 32) or None, xp (P, 3) the kernel's own x' or None, in the form ops.is_mixed selects"""
    ops, m = pkg("ops"), model(arch)
    p, pk, fr = ops.PRECISIONS[prec], pack(arch, prec), m["frame"]
    N, S = z.shape
    P = N * S
    x = rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]
    if not ops.is_mixed(arch, p) and prec != "bf16x3":       # one launch with debug planes
        raw, dx, w, grid = ops.field_forward(pk, fr, level, rays, z, precision=p, debug=True, arch=arch)
        out = dict(raw=raw, feats=grid.reshape(P, 32), xp=(x + dx).reshape(P, 3))
    elif not ops.is_mixed(arch, p):                          # the split-operand whole-network kernel: no debug planes, its save
        bits = ops.alloc_sign_bits(P, ops.FIELD_ALL, arch, DEV)
        raw, act = ops.field_forward_save(pk, fr, level, rays, z, arch, bits=bits, precision=p)
        plain = ops.field_forward(pk, fr, level, rays, z, precision=p, arch=arch)
        assert FR.same_bits(raw, plain), "%s %s: the saving launch's raw differs from the plain launch's" % (arch, prec)
        out = dict(raw=raw, feats=grid_plane(arch, act, P), xp=xw_plane(arch, act, P))
    else:                                                    # the chain: a deformation + a radiance launch
        xw = torch.full((N, S, 8), float("nan"), device=DEV)
        raw = ops.field_forward_split(pk, fr, level, ops.FIELD_ALL, rays, xw, z=z, arch=arch, precision=p)
        out = dict(raw=raw, feats=None, xp=xw[..., 0:3].reshape(P, 3))
        if prec == "bf16x3":                                 # the same two kernels, saving: the features are in the whole-network save
            act = torch.zeros(P, int(ops._fn("act_words_part", arch)[0](ops.FIELD_ALL)), device=DEV)
            bits = ops.alloc_sign_bits(P, ops.FIELD_ALL, arch, DEV)
            xw2 = torch.zeros(N, S, 8, device=DEV)
            ident = torch.arange(S, dtype=torch.int32, device=DEV).repeat(N, 1).contiguous()
            ops.field_forward_split_save(pk, fr, level, ops.FIELD_DEFORM, rays, xw2, z=z, arch=arch, precision=p, whole=(act, bits))
            raw2, _ = ops.field_forward_split_save(pk, fr, level, ops.FIELD_RADIANCE, rays, xw2, src=ident, arch=arch, precision=p, whole=(act, bits))
            assert FR.same_bits(raw2, raw), "%s %s: the saving chain's raw differs from the plain chain's" % (arch, prec)
            out["feats"] = grid_plane(arch, act, P)
    torch.cuda.synchronize()
    out["raw"] = out["raw"].reshape(P, 16)
    return out


# raw of the lower-precision kernels: the yardstick measures an error in units of the float32 eager field's own, which carries the
# network's amplification (the octaves of the encodings) times float32's unit round-off.  A kernel that carries its operands in a shorter
# format is allowed that format's unit in its place: split bf16 operands (hi + lo: 16 significant bits) 2^8 times the factors, plain
# bf16 (8 bits) 2^16 times.  For bf16 this holds raw against misplaced rows and non-finite values only (observed: 60 times the
# float32 field's error, not 2^16 times); those kernels' lookups are held by their fp32 feature planes above, at the default factors.
RAW_FACTOR = {"fp32": 1.0, "bf16": 2.0 ** 16, "bf16x3": 2.0 ** 8}


def eager(arch, name, level):
    m = model(arch)
    key = ("fwd", name, level)
    if key not in m["refs"]:
        x6 = GR.launch_inputs(GR.position_sets()[name], DEV)[2]
        m["refs"][key] = {dt: FR.eager_field(m["sd_np"], arch, level, x6, m["frame"][0:76], m["frame"][80:116], dt) for dt in (torch.float32, torch.float64)}
    return m["refs"][key]


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("arch", ARCHS)
def test_forward_at_the_faces(arch, prec):
    t0 = time.time()
    failures = []
    for name in GR.SETS:
        ps = GR.position_sets()[name]
        rays, z, x6 = GR.launch_inputs(ps, DEV)
        x = x6[:, :3]
        f64, f32 = GR.features(model(arch)["sd_np"], arch, x, torch.float64), GR.features(model(arch)["sd_np"], arch, x, torch.float32)
        for level in (0, 1):
            what = "grid edges %s %s %s L%d" % (arch, prec, name, level)
            got = forward_taps(arch, prec, level, rays, z)
            if got["xp"] is not None and name != "far_out":      # the kernel's own x' is the set's x, bit for bit
                assert FR.same_bits(got["xp"], x), what + ": x' differs from x (the warp head is zero and o + d z is exact)"
            try:
                if got["feats"] is not None:
                    rec = GR.feature_check(got["feats"], f32, f64, name, what + " features")
                    print("%s features: max %.2e (float32 grid_sample %.2e) rms %.2e (%.2e) scale %.2e" % ((what,) + rec[1:]))
                if name != "far_out":
                    ref = eager(arch, name, level)
                    r32, r64 = ref[torch.float32]["raw"], ref[torch.float64]["raw"]
                    n = lambda a: a.detach().double().cpu().numpy()
                    for part, cols in (("rgb/seg", slice(0, 15)), ("sigma", slice(15, 16))):
                        rec = yardstick(n(got["raw"][:, cols]), n(r32[:, cols]), n(r64[:, cols]), what + " " + part, factor=2.0 * RAW_FACTOR[prec], factor_max=3.0 * RAW_FACTOR[prec])
                        print("%s %s: max %.2e (float32 eager %.2e) rms %.2e (%.2e) scale %.2e" % ((what, part) + rec[1:]))
            except AssertionError as e:
                failures.append(str(e))
    print("%s %s: %.1f s" % (arch, prec, time.time() - t0))
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------------------
def backward_case(arch, name, level):
    """-> (case, act, bits, float64 reference, float32 reference); the save and the references are made once per session.  The
    NeRFaceModels save with sign bits too (ops.field_forward_save), so that their fused walk can run on the same activations."""
    m, ops = model(arch), pkg("ops")
    key = ("bwd", name, level)
    if key not in m["refs"]:
        c = GR.make_case(pkg("weights"), arch, name, level, DEV, m["frame"], flat=m["flat"], sd_np=m["sd_np"])
        if arch == "audio":
            act, bits = BR._forward(c, "f32")
        else:
            bits = ops.alloc_sign_bits(c["P"], ops.FIELD_ALL, arch, DEV)
            _, act = ops.field_forward_save(pack(arch, "fp32"), c["frame"], level, c["rays"], c["z"], arch, bits=bits)
            torch.cuda.synchronize()
        assert FR.same_bits(xw_plane(arch, act, c["P"]), c["x6"][:, :3]), "%s %s L%d: the saved x' differs from x" % (arch, name, level)
        masks = BR._masks(act, arch, c["P"])
        # (NeRFaceModel: a zero seam input makes the reference return d raw-loss / d (x', w) for the radiance part's seam output)
        ce = c if arch != "nerface" else dict(c, seam=torch.zeros(c["P"], 8, device=DEV))
        m["refs"][key] = (c, act, bits, BR._eager(ce, masks, 0, c["P"]), BR._eager(ce, masks, 0, c["P"], dtype=torch.float32))
    return m["refs"][key]


def walks(arch):
    """(walk, form): backward_reference._paths in fp32 arithmetic, and the NeRFaceModels' fused walk (tests/test_gpu_nerface_fused.py: held
    to the per-layer walk's bound), whole and -- where there are deformation nets -- as radiance part + deformation part"""
    out = [(w, f) for w, p, f in BR._paths(arch, "f32") if p == "fp32"]
    if arch != "audio":
        out += [("fused", "part3")] + ([("fused", "part2+1")] if arch == "nerface" else [])
    return out


def bound_of(arch, walk):
    return BR.FIELD_BOUNDS[(arch, "f32", walk if arch == "audio" else "layer", "fp32")]


def hip_walk(c, act, bits, walk, form, grad_flat=None):
    """one HIP backward walk in fp32 GEMM arithmetic -> {tensor: gradient}"""
    arch = c["arch"]
    if arch == "audio" or walk == "layer":
        return BR._hip(c, act, bits, walk, "fp32", form, False, grad_flat=grad_flat)
    ops = pkg("ops")
    flat, frame, lv = c["flat"], c["frame"], c["level"]
    gf, gc = torch.zeros_like(flat) if grad_flat is None else grad_flat, torch.zeros(128, device=DEV)
    seam = None
    found = ops.backward_gemm_precision(), ops.fused_backward()
    try:
        ops.backward_gemm_precision("fp32")
        ops.fused_backward(True)
        if form == "part3":
            ops.field_backward_split(flat, frame, lv, 3, act, gf, gc, d_raw=c["d_raw"], arch=arch, bits=bits)
        else:
            seam = ops.field_backward_split(flat, frame, lv, ops.FIELD_RADIANCE, act, gf, gc, d_raw=c["d_raw"], arch=arch, full_act=True, bits=bits)
            ops.field_backward_split(flat, frame, lv, ops.FIELD_DEFORM, act, gf, gc, xw_grad_in=seam, arch=arch, full_act=True, bits=bits)
        torch.cuda.synchronize()
    finally:
        ops.backward_gemm_precision(found[0])
        ops.fused_backward(found[1])
    got = {k: gf[o:o + int(np.prod(shape))].view(shape) for k, (o, shape) in c["off"].items() if BR._compared(k, lv)}
    got["driving"], got["pose36"] = gc[0:76], gc[80:116]
    if seam is not None:
        got["seam"] = seam
    return got


def prefill(n):
    """a fixed nonzero pattern: no entry is zero, neighbours differ"""
    return (0.375 + 0.001 * (torch.arange(n, device=DEV) % 257).float()) * (1.0 - 2.0 * (torch.arange(n, device=DEV) % 2).float())


@pytest.mark.parametrize("name", GR.BACKWARD_SETS)
@pytest.mark.parametrize("arch", ARCHS)
def test_backward_at_the_faces(arch, name):
    t0 = time.time()
    ops = pkg("ops")
    found = ops.backward_gemm_precision(), ops.fused_backward()
    failures = []
    try:
        goff, gshape = pkg("weights").canonical_offsets(arch)["spatial_embeddings"]
        gn = int(np.prod(gshape))
        for level in (0, 1):
            c, act, bits, ref, ref32 = backward_case(arch, name, level)
            rg = ref["spatial_embeddings"].reshape(-1)
            for walk, form in walks(arch):
                bound = bound_of(arch, walk)
                what = "grid edges %s %s L%d %s/%s" % (arch, name, level, walk, form)
                got = hip_walk(c, act, bits, walk, form)
                fails, errs = GR.backward_check(got, ref, bound, arch, ref32=ref32)
                top = sorted(errs.items(), key=lambda kv: -kv[1])[:3]
                coord = max([errs[k] for k in errs if GR.group_of(k) == "coord"], default=float("nan"))
                print("%s: grid %.2e coord %.2e worst %s (bound %.1e); %d of %d grid entries are exactly 0 in float64"
                      % (what, errs["spatial_embeddings"], coord, ", ".join("%s %.2e" % kv for kv in top), bound, int((rg == 0).sum()), gn))
                failures += ["%s: %s" % (what, f) for g in fails.values() for f in g]
                # the same walk into a prefilled buffer: what float64 leaves at 0 keeps its bits
                gf = prefill(c["flat"].numel())
                before = gf[goff:goff + gn].clone()
                hip_walk(c, act, bits, walk, form, grad_flat=gf)
                keep = rg == 0
                if not FR.same_bits(gf[goff:goff + gn][keep], before[keep]):
                    failures.append("%s: grid entries without a gradient changed in a prefilled buffer" % what)
                if name not in GR.ZERO_SETS and FR.same_bits(gf[goff:goff + gn], before):
                    failures.append("%s: the prefilled grid gradient did not change at all" % what)
        # level 0, then level 1, into one buffer
        (c0, a0, b0, r0, _), (c1, a1, b1, r1, _) = backward_case(arch, name, 0), backward_case(arch, name, 1)
        rsum = (r0["spatial_embeddings"] + r1["spatial_embeddings"]).reshape(-1)
        for walk, form in walks(arch):
            bound = bound_of(arch, walk)
            what = "grid edges %s %s L0+L1 %s/%s" % (arch, name, walk, form)
            gf = torch.zeros_like(c0["flat"])
            hip_walk(c0, a0, b0, walk, form, grad_flat=gf)
            hip_walk(c1, a1, b1, walk, form, grad_flat=gf)
            g = gf[goff:goff + gn].double()
            sc = float(rsum.abs().max())
            err = float((g - rsum).abs().max()) / sc if sc > 0 else 0.0
            print("%s: grid %.2e of the summed reference's scale (bound %.1e)" % (what, err, bound))
            if err > bound:
                failures.append("%s: grid gradient of both levels %.3e of scale (bound %.1e)" % (what, err, bound))
            if bool(((rsum == 0) & (g != 0)).any()):
                failures.append("%s: grid entries both references leave at 0 are not 0" % what)
    finally:
        ops.backward_gemm_precision(found[0])
        ops.fused_backward(found[1])
    assert (ops.backward_gemm_precision(), ops.fused_backward()) == found
    print("%s %s: %.1f s" % (arch, name, time.time() - t0))
    assert not failures, "\n".join(failures)
