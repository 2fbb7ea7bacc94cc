"""Shared pieces of the field backward's float64 tests (tests/test_gpu_backward_tails.py, tests/test_gpu_nerface_fused.py,
tests/test_gpu_grid_edges.py on the GPU; tests/test_grid_reference_host.py on the host).  TEST INFRASTRUCTURE ONLY; importing it needs
no GPU.

A case is a dict `c`: arch, N, S, P, sd_np, flat, frame, rays, z, x6, d_raw, seam (AudioFaceModel) or None, level, off.  `_forward` runs
the saving HIP forward, `_masks` reads the side of every kink from its save, `_eager` is float64 autograd of oracle/torch_eager.py's
EagerField on those sides, `_hip` one HIP backward walk, `_errors` the per-tensor comparison the bounds in FIELD_BOUNDS are held on."""
import numpy as np
import torch

from conftest import pkg

DEV = torch.device("cuda:0")

CHUNK = 32768          # samples per float64 evaluation
EDGE_GAIN = 31.0       # upstream rows of edge samples are scaled by 1 + 30

# worst |HIP - float64| / scale over the compared tensors, per (arch, saving forward, walk, GEMM arithmetic): ~3-4x the worst observed
# over all sizes and forms (audio fp32-MFMA forward 5.3e-5 in every walk; its split-operand forward 1.65e-4; 15-octave NeRFace 8.6e-4;
# static 2.6e-5 in f32 products, 2.5e-4 with split-bf16 operands -- a cancelling bias sum at P = 1,023)
FIELD_BOUNDS = {
    ("audio", "f32", "fused", "fp32"): 2e-4, ("audio", "f32", "fused", "bf16x3"): 2e-4,
    ("audio", "f32", "layer", "fp32"): 2e-4, ("audio", "f32", "layer", "bf16x3"): 2e-4,
    ("audio", "x3", "fused", "fp32"): 6e-4, ("audio", "x3", "fused", "bf16x3"): 6e-4,
    ("nerface", "f32", "layer", "fp32"): 3e-3, ("nerface", "f32", "layer", "bf16x3"): 3e-3,
    ("nerface_static", "f32", "layer", "fp32"): 1e-4, ("nerface_static", "f32", "layer", "bf16x3"): 1e-3,
}

# Held to a bound of its own, outside the path's: the NeRFaceModel's single fc_ambient bias.  Its gradient reaches the loss only through
# the 15-octave encoding of w, which multiplies the ~1e-7 round-off of the forward's w by up to 2^14, and it is a sum that cancels.
# Observed 1.6e-2 of scale at P = 17 in both GEMM arithmetics (plain fp32 autograd with its own branches: up to 31 %,
# tests/test_gpu_nerface.py::test_field_backward_seam_vs_autograd).  This bound cannot see one lost sample in this tensor; the other
# tensors of the deformation part can (the sensitivity floor of every case).
ILL_CONDITIONED = {("nerface", "hyper_sheep_mlp.fc_ambient.bias"): 5e-2}


def _paths(arch, fwd):
    """(walk, GEMM arithmetic, form) of the backward runs over one saving forward"""
    if arch != "audio":
        return [("layer", p, "whole") for p in ("fp32", "bf16x3")]
    walks = ("fused", "layer") if fwd == "f32" else ("fused",)
    return [(w, p, f) for w in walks for p in ("fp32", "bf16x3") for f in ("part3", "part2+1")]


def _edge_rows(P):
    """the samples the tails are made of: the last 16, the first and last of every 1,024 block, 128 k for a few k"""
    rows = set(range(max(0, P - 16), P))
    for b in range(0, P, 1024):
        rows |= {b, min(P, b + 1024) - 1}
    rows |= {128 * k for k in (1, 2, 3, 8, 255, 256) if 128 * k < P}
    return sorted(rows)


def _masks(act, arch, P):
    """Which side of zero every hidden unit is on, as the HIP forward saw it: the saved post-activations of a whole-network save
    (sahs::act layout, csrc/sahs_layout.hpp: one dense [P x width] array per layer, array of column c at c * P)."""
    kbx, kba, trl = {"audio": (4, 2, 8), "nerface": (6, 2, 4), "nerface_static": (4, 0, 4)}[arch]
    WH = 16 * kbx
    HH = WH + 6 * 128 + 16
    Tt = HH + 6 * 64 + 32 + 16 * kbx + 16 * kba
    C = Tt + trl * 256 + 256 + 64
    Ss = C + 512
    assert act.shape == (P, Ss + 512)
    flat_act = act.reshape(-1)
    arr = lambda c, w: flat_act[c * P:(c + w) * P].view(P, w)
    masks = {}
    for i in range(6):
        masks["warp.%d" % i] = arr(WH + 128 * i, 128) > 0
        masks["hyper.%d" % i] = arr(HH + 64 * i, 64) > 0
    for i in range(trl):
        masks["trunk.%d" % i] = arr(Tt + 256 * i, 256) > 0
    for i in range(4):
        masks["dir.%d" % i] = arr(C + 128 * i, 128) > 0
        masks["seg.%d" % i] = arr(Ss + 128 * i, 128) > 0
    return masks


def _forward(c, fwd):
    """the saving forward -> (act, bits); AudioFaceModel: the split evaluation's whole-network save (fp32 MFMAs, or the split-operand
    kernels as a deformation + a radiance launch into one whole-network save); NeRFaceModels: field_forward_save"""
    ops = pkg("ops")
    N, S, arch = c["N"], c["S"], c["arch"]
    if arch != "audio":
        packed = ops.pack_weights(c["flat"], arch=arch)
        _, act = ops.field_forward_save(packed, c["frame"], c["level"], c["rays"], c["z"], arch)
        return act, None
    xw = torch.zeros(N, S, 8, device=DEV)
    bits = ops.alloc_sign_bits(N * S, ops.FIELD_ALL, "audio", DEV)
    if fwd == "f32":
        _, act = ops.field_forward_split_save(ops.pack_weights(c["flat"]), c["frame"], c["level"], ops.FIELD_ALL, c["rays"], xw, z=c["z"], bits=bits)
    else:
        pk = ops.pack_weights(c["flat"], ops.SAHS_BF16X3)
        act = torch.zeros(N * S, int(ops._fn("act_words_part", "audio")[0](ops.FIELD_ALL)), device=DEV)
        ident = torch.arange(S, dtype=torch.int32, device=DEV).repeat(N, 1).contiguous()
        ops.field_forward_split_save(pk, c["frame"], c["level"], ops.FIELD_DEFORM, c["rays"], xw, z=c["z"], precision=ops.SAHS_BF16X3, whole=(act, bits))
        ops.field_forward_split_save(pk, c["frame"], c["level"], ops.FIELD_RADIANCE, c["rays"], xw, src=ident, precision=ops.SAHS_BF16X3, whole=(act, bits))
    torch.cuda.synchronize()
    return act, bits


def _compared(k, level):
    """the parameter tensors the field backward of `level` writes (the other level's net gets nothing; AudioNet is the conditioning
    backward's)"""
    lvl = "coarse" if level == 0 else "fine"
    return not (("nerf_mlps." in k and lvl not in k) or k.startswith("audNet_head"))


def _eager(c, masks, lo, hi, dtype=torch.float64, field_cls=None):
    """Autograd of EagerField (float64: the yardstick) on samples [lo, hi), on the HIP forward's side of every kink, with the frame's own
    conditioning vectors as leaves: {tensor: gradient} for the parameters, "driving", "pose36" and (AudioFaceModel) "seam" = d raw-loss /
    d (x', w).  Evaluated on the device of the case's points; ``field_cls``: a subclass of EagerField to differentiate instead."""
    from oracle import torch_eager as TE
    arch, frame = c["arch"], c["frame"]
    dev = c["x6"].device
    sd = {k: torch.from_numpy(v).to(dev, dtype).requires_grad_(True) for k, v in c["sd_np"].items()}
    drv = frame[0:76].to(dtype).clone().requires_grad_(True)
    p36 = frame[80:116].to(dtype).clone().requires_grad_(True)
    lvl = "coarse" if c["level"] == 0 else "fine"
    seams = []
    for s in range(lo, hi, CHUNK):
        e = min(hi, s + CHUNK)
        field = (field_cls or TE.EagerField)(sd, num_coarse=e - s, num_fine=0, arch=arch, masks={k: m[s:e] for k, m in masks.items()})
        taps = {}
        raw = field.forward(lvl, c["x6"][s:e].to(dtype), None, None, driving=drv, pose36=p36, taps=taps)
        loss = (raw * c["d_raw"][s:e].to(dtype)).sum()
        if c["seam"] is not None:
            na = taps["amb"].shape[1]
            sm = c["seam"][s:e].to(dtype)
            loss = loss + (taps["warped"] * sm[:, 0:3]).sum() + (taps["amb"] * sm[:, 4:4 + na]).sum()
            taps["warped"].retain_grad()
            taps["amb"].retain_grad()
        loss.backward()
        if c["seam"] is not None:
            g = torch.zeros(e - s, 8, dtype=dtype, device=dev)
            g[:, 0:3] = taps["warped"].grad - sm[:, 0:3]
            g[:, 4:4 + na] = taps["amb"].grad - sm[:, 4:4 + na]
            seams.append(g)
        del raw, loss, taps, field
    out = {k: v.grad for k, v in sd.items() if _compared(k, c["level"])}
    out["driving"], out["pose36"] = drv.grad, p36.grad
    if seams:
        out["seam"] = torch.cat(seams)
    return out


def _hip(c, act, bits, walk, prec, form, zero_last, grad_flat=None):
    """one HIP backward walk -> {tensor: gradient (views of grad_flat / grad_cond)}.  ``grad_flat``: the parameter-gradient buffer to add
    into (default: a zeroed one)"""
    ops = pkg("ops")
    d_raw, seam = c["d_raw"], c["seam"]
    if zero_last:       # the negative control: the last sample's upstream rows dropped
        d_raw = d_raw.clone()
        d_raw[-1] = 0.0
        seam = None if seam is None else seam.clone()
        if seam is not None:
            seam[-1] = 0.0
    flat, frame, lv, arch = c["flat"], c["frame"], c["level"], c["arch"]
    gf, gc = torch.zeros_like(flat) if grad_flat is None else grad_flat, torch.zeros(128, device=DEV)
    g_out = None
    found = ops.backward_gemm_precision(), ops.fused_backward()
    try:
        ops.backward_gemm_precision(prec)
        ops.fused_backward(walk == "fused")
        if form == "whole":
            ops.field_backward(flat, frame, lv, act, d_raw, gf, gc, arch)
        elif form == "part3":
            ops.field_backward_split(flat, frame, lv, 3, act, gf, gc, d_raw=d_raw, xw_grad_in=seam, bits=bits)
        else:           # radiance part, then the deformation part from its seam gradient: RenderRaysFn's chain
            g_out = ops.field_backward_split(flat, frame, lv, ops.FIELD_RADIANCE, act, gf, gc, d_raw=d_raw, full_act=True, bits=bits)
            ops.field_backward_split(flat, frame, lv, ops.FIELD_DEFORM, act, gf, gc, xw_grad_in=g_out + seam, full_act=True, bits=bits)
        torch.cuda.synchronize()
    finally:
        ops.backward_gemm_precision(found[0])
        ops.fused_backward(found[1])
    got = {k: gf[o:o + int(np.prod(shape))].view(shape) for k, (o, shape) in c["off"].items() if _compared(k, lv)}
    got["driving"], got["pose36"] = gc[0:76], gc[80:116]
    if g_out is not None:
        got["seam"] = g_out
    return got


def _part(k):
    if k.startswith(("warp_field_mlp", "hyper_sheep_mlp")):
        return "deformation"
    if k.startswith("nerf_mlps") or k == "spatial_embeddings":
        return "radiance"
    return k        # driving / pose36 / seam


def _errors(got, ref):
    """per tensor: max |HIP - float64| / max |float64|; a tensor float64 leaves at zero must be exactly zero"""
    errs = {}
    for k, r in ref.items():
        if k not in got:
            continue
        if got[k] is None and r is None:
            continue
        g = got[k].double()
        if k == "seam":
            g, r = g[:, [0, 1, 2, 4, 5]], r[:, [0, 1, 2, 4, 5]]
        if r is None:
            errs[k] = 0.0 if float(g.abs().max()) == 0.0 else float("inf")
            continue
        sc = float(r.abs().max())
        errs[k] = float((g - r).abs().max()) / sc if sc > 0 else (0.0 if float(g.abs().max()) == 0.0 else float("inf"))
    return errs
