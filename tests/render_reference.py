"""References and seeded inputs for the render stages around the field kernel (csrc/render_ops.hip), shared by the host suite
(tests/test_render_reference_host.py) and the GPU suite (tests/test_gpu_render_tails.py).  TEST INFRASTRUCTURE ONLY.

 * composite64: volume_render_radiance_field (volume_rendering_utils.py:7-78) plus the caller's prior overwrite (train_utils.py:135-136)
   restated in numpy float64, with the fp32 constants the reference uses (1e10, 1e-6, 1e-10 as float32 values widened), and a ``fault=``
   switch that returns a deliberately WRONG result: the faults a lane-per-sample compositor can have at its block and size edges.
 * composite_case: the density regimes the compositor is fed (normal, opaque mid-ray, empty, saturated colour logits, thin medium).
 * torch_sample_pdf / torch_merge: ATen itself on the host = the reference's arithmetic for sample_pdf_2 and for sort(cat(z, samples)).
 * resample_case / branch_rows: the weight families of the resampling sweep and, per row, the branch of resample_kernel it takes
   (row-sum form, cumsum path, scan blocks), computed on the host the way the kernel decides it.
"""
import numpy as np
import torch

F32_FAR = float(np.float32(1e10))       # the last sample's distance, volume_rendering_utils.py:16
F32_SIGMA_EPS = float(np.float32(1e-6))  # sigma[:, -1] += 1e-6, :57
F32_T_EPS = float(np.float32(1e-10))     # cumprod(1 - alpha + 1e-10), :59

REGIMES = ("normal", "opaque", "empty", "saturated", "thin")
COMPOSITE_S = (1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)
OPTIONS = {"prior": dict(bg=True, noise=False, white=False), "prior_noise": dict(bg=True, noise=True, white=False),
           "white": dict(bg=False, noise=False, white=True), "plain": dict(bg=False, noise=False, white=False)}
# carry: the transmittance carried into a block of 64 samples reset to 1 (applies from S = 65); far / prior: the two halves of "the last
# sample is special" -- its 1e10 distance missing (its own distance is 0: it absorbs nothing), the prior not written over its colour (only
# with a prior); drop_last: sample S-1 left out; extra_factor: a lane past S leaking the clamped last sample's factor into the running
# product, which every sample after the first then inherits (lane 0's product is final from the start; nothing to inherit at S = 1).
FAULTS = ("carry", "far", "prior", "drop_last", "extra_factor")
OUTPUTS = ("rgb", "disp", "acc", "weights", "depth")


def fault_applies(fault, S, opt):
    return {"carry": S >= 65, "far": True, "prior": OPTIONS[opt]["bg"], "drop_last": True, "extra_factor": S >= 2}[fault]


def composite64(raw, z, rd, noise=None, bg=None, white_background=False, fault=None):
    """-> (rgb (N,15), disp, acc, weights (N,S), depth) in float64.  fault: None or one of FAULTS."""
    assert fault is None or fault in FAULTS, fault
    raw, z, rd = (np.asarray(a, np.float64) for a in (raw, z, rd))
    N, S, _ = raw.shape
    nrm = np.sqrt((rd * rd).sum(-1))
    dist = np.concatenate([z[:, 1:] - z[:, :-1], np.full((N, 1), 0.0 if fault == "far" else F32_FAR)], axis=1) * nrm[:, None]
    with np.errstate(over="ignore", under="ignore"):
        if bg is not None:
            seg = raw[..., 3:15] - raw[..., 3:15].max(-1, keepdims=True)
            seg = np.exp(seg)
            col = np.concatenate([1.0 / (1.0 + np.exp(-raw[..., :3])), seg / seg.sum(-1, keepdims=True)], axis=-1)
            if fault != "prior":
                col[:, -1, :] = np.asarray(bg, np.float64)
        else:
            col = 1.0 / (1.0 + np.exp(-raw[..., :15]))
        sigma = np.maximum(raw[..., 15] + (0.0 if noise is None else np.asarray(noise, np.float64)), 0.0)
        sigma[:, -1] += F32_SIGMA_EPS
        alpha = 1.0 - np.exp(-sigma * dist)
        f = 1.0 - alpha + F32_T_EPS
        T = np.ones((N, S))
        for s in range(1, S):
            T[:, s] = 1.0 if (fault == "carry" and s % 64 == 0) else T[:, s - 1] * f[:, s - 1]
        if fault == "extra_factor":
            T[:, 1:] *= f[:, -1:]
        w = alpha * T
        if fault == "drop_last":
            w[:, -1] = 0.0
        rgb = (w[..., None] * col).sum(1)
        depth, acc = (w * z).sum(1), w.sum(1)
        with np.errstate(invalid="ignore", divide="ignore"):
            dd = depth / acc
            disp = np.where(np.isnan(dd), dd, 1.0 / np.maximum(F32_T_EPS, dd))
        if white_background:
            rgb = rgb + (1.0 - acc[:, None])
    return rgb, disp, acc, w, depth


def composite_case(regime, S, opt, N=67, seed=0):
    """Seeded inputs of one compositor case -> dict(raw, z, rays (N,8), rd, noise | None, bg | None, white)."""
    o = OPTIONS[opt]
    rng = np.random.default_rng([seed, REGIMES.index(regime), S, list(OPTIONS).index(opt)])
    raw = (rng.standard_normal((N, S, 16)) * 1.5).astype(np.float32)
    sg = raw[..., 15] * 8 + 2                         # moderate density: transmittance ~e^-3 by sample 64
    if regime == "opaque":                            # goes opaque mid-ray: factors of 1e-10, transmittance denormal, then zero
        sg = np.where(rng.uniform(size=(N, S)) < 0.5, 10.0 ** rng.uniform(2, 5, (N, S)), sg)
    elif regime == "empty":                           # all density <= 0: the weight sits on the last sample
        sg = -np.abs(sg)
    elif regime == "saturated":                       # colour logits x 60: sigmoid and softmax saturate, expf over- and underflows
        raw[..., :15] *= 60.0
    elif regime == "thin":                            # thin medium: the tail samples carry the weight
        sg = np.abs(sg) * 1e-4
    raw[..., 15] = sg.astype(np.float32)
    z = np.sort(rng.uniform(0.48, 1.08, (N, S)).astype(np.float32), axis=1)
    rays = np.zeros((N, 8), np.float32)
    rays[:, 3:6] = rng.normal(0, 0.2, (N, 3)) + np.array([0, 0, -1.0])
    rays[:, 6], rays[:, 7] = 0.48, 1.08
    noise = rng.standard_normal((N, S)).astype(np.float32) if o["noise"] else None
    bg = rng.uniform(0, 1, (N, 15)).astype(np.float32) if o["bg"] else None
    return dict(raw=raw, z=z, rays=rays, rd=rays[:, 3:6].copy(), noise=noise, bg=bg, white=o["white"])


def composite_refs(case, oracle, fault=None):
    """(fp32 C oracle's five outputs, float64 restatement's five outputs [with ``fault``]) of a composite_case."""
    r32 = oracle.composite(case["raw"], case["z"], case["rd"], noise=case["noise"], bg=case["bg"], white_background=case["white"])
    r64 = composite64(case["raw"], case["z"], case["rd"], noise=case["noise"], bg=case["bg"], white_background=case["white"], fault=fault)
    return r32, r64


def torch_volume_render(case, torch_eager):
    """The torch-eager fp32 restatement on a composite_case (the prior written over the last sample's colours first)."""
    raw = torch.from_numpy(case["raw"].copy())
    if case["bg"] is not None:
        raw[:, -1, :15] = torch.from_numpy(case["bg"])
    outs = torch_eager.volume_render(raw, torch.from_numpy(case["z"]), torch.from_numpy(case["rd"]),
                                     None if case["noise"] is None else torch.from_numpy(case["noise"]), case["white"], case["bg"] is not None)
    return tuple(o.numpy() for o in outs)


# ---- importance resampling ---------------------------------------------------------------------------------------------------
RESAMPLE_S = (3, 4, 5, 9, 10, 11, 12, 13, 14, 17, 33, 34, 41, 42, 64, 65, 66, 67, 130, 194, 255, 256)   # 12..14: np % 8 = 2, 3, 4 in the vector form
RESAMPLE_NF = (1, 2, 5, 63, 64, 65, 128, 255, 256)
FAMILIES = ("u6", "zero", "onehot", "wide", "span")
ROWS_PER_FAMILY = 8
U_LAST = float(np.float32(1.0) - np.float32(2.0 ** -24))      # the largest draw of a 24-bit uniform


def family_weights(family, N, S, rng):
    if family == "u6":
        w = rng.uniform(0, 1, (N, S)) ** 6
    elif family == "zero":
        w = np.zeros((N, S))
    elif family == "onehot":
        w = np.zeros((N, S))
        w[np.arange(N), rng.integers(0, S, N)] = 1.0
        w[0, 1 + rng.integers(0, S - 2)] = 1.0                        # (at least one ray with the one inside the pdf's columns 1..S-2)
    elif family == "wide":                                              # 16 decades wide, with exact zeros
        w = 10.0 ** rng.uniform(-16, 0, (N, S)) * (rng.uniform(size=(N, S)) > 0.2)
    elif family == "span":       # one weight of 10 * 2^U(0.5, 2.5) among a sparse sprinkle below the 1e-5 the reference adds: the quotients' exponents
        w = np.where(rng.uniform(size=(N, S)) < 0.25, 10.0 ** rng.uniform(-9, -5.5, (N, S)), 0.0)     # span 20, 21 or 22 binades
        w[np.arange(N), 1 + rng.integers(0, S - 2, N)] = 10.0 * 2.0 ** rng.uniform(0.5, 2.5, N)
    else:
        raise KeyError(family)
    return w.astype(np.float32)


def resample_case(S, nf, rand_u, seed=0, rows=ROWS_PER_FAMILY):
    """One launch of the sweep: ``rows`` rays of every family side by side (so a 4-ray workgroup holds rays of different branches).
    -> z (N,S) sorted, weights (N,S), u (N,nf) | None (det=True), family (N,) index into FAMILIES."""
    rng = np.random.default_rng([seed, S, nf, int(rand_u)])
    fam = np.repeat(np.arange(len(FAMILIES)), rows)
    N = fam.size
    z = np.sort(rng.uniform(0.48, 1.08, (N, S)).astype(np.float32), axis=1)
    w = np.concatenate([family_weights(f, rows, S, rng) for f in FAMILIES], axis=0)
    u = None
    if rand_u:
        u = (rng.integers(0, 2 ** 24, (N, nf)).astype(np.float64) * 2.0 ** -24).astype(np.float32)   # 24-bit uniforms, as ray_uniforms draws them
        u[::2, 0] = 0.0                       # exact 0 and the largest draw, on alternating rays (nf may be 1)
        u[1::2, -1] = U_LAST
    return z, w, u, fam


def torch_sample_pdf(bins, weights, num_samples, u=None):
    """nerf_helpers.py:454-497 by ATen on the host -> (samples, inds, number of draws with denom < 1e-5), numpy."""
    bins, weights = torch.from_numpy(np.ascontiguousarray(bins)), torch.from_numpy(np.ascontiguousarray(weights))
    weights = weights + 1e-5
    pdf = weights / torch.sum(weights, dim=-1, keepdim=True)
    cdf = torch.cat([torch.zeros_like(pdf[..., :1]), torch.cumsum(pdf, dim=-1)], dim=-1)
    if u is None:
        u = torch.linspace(0.0, 1.0, steps=num_samples, dtype=weights.dtype).expand(list(cdf.shape[:-1]) + [num_samples])
    else:
        u = torch.from_numpy(np.ascontiguousarray(u))
    u = u.contiguous()
    inds = torch.searchsorted(cdf.contiguous(), u, right=True)
    below, above = torch.clamp(inds - 1, min=0), torch.clamp(inds, max=cdf.shape[-1] - 1)
    cb, ca = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
    bb, ba = torch.gather(bins, 1, below), torch.gather(bins, 1, above)
    den = ca - cb
    small = den < 1e-5
    den = torch.where(small, torch.ones_like(den), den)
    return (bb + (u - cb) / den * (ba - bb)).numpy(), inds.numpy(), small.sum(dim=-1).numpy()


def torch_merge(z, z_new):
    """train_utils.py:166 on the host: torch.sort(cat(z, z_new)) -- stable, NaN after every number -> (sorted values, source index)."""
    cat = torch.cat([torch.from_numpy(np.ascontiguousarray(z)), torch.from_numpy(np.ascontiguousarray(z_new))], dim=-1)
    v, i = torch.sort(cat, dim=-1, stable=True)
    return v.numpy(), i.numpy()


def bits(a):
    """fp32 array as its bit patterns: equality that tells NaNs (and their payloads) apart."""
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def branch_rows(weights, oracle):
    """Per row of (N,S) coarse weights, the branch resample_kernel takes, decided on the host as the kernel decides it:
    np (pdf entries = S-2), form ("scalar": np < 8 | "vector"), rem (np % 8), groups (groups of four 8-lane vectors), span (float32
    quotient exponents' max - min over the non-zero quotients, 255 if any is not finite; the divisor is ATen's row sum), path
    ("scan": span <= 20 | "sequential") and blocks (64-lane blocks of the cumsum)."""
    w = np.asarray(weights, np.float32)
    N, S = w.shape
    n = S - 2
    rows = []
    for r in range(N):
        wp = w[r, 1:-1] + np.float32(1e-5)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            q = (wp / oracle.aten_sum(wp)).astype(np.float32)
        e = (q.view(np.uint32) >> 23) & 255
        if not np.all(np.isfinite(q)):
            span = 255
        else:
            nz = e[q != 0.0]
            span = int(nz.max()) - int(nz.min()) if nz.size else -255
        rows.append(dict(np=n, form="scalar" if n < 8 else "vector", rem=n % 8, groups=(n // 8) // 4, span=span,
                         path="scan" if span <= 20 else "sequential", blocks=(n + 63) // 64))
    return rows


class Coverage:
    """What a sweep of resample inputs entered, accumulated over its launches; ``missing()`` names every branch of the list in
    tests/test_gpu_render_tails.py's docstring that no row took."""

    def __init__(self):
        self.scalar = 0
        self.vector_rem, self.vector_groups = set(), set()
        self.span20 = self.span21 = 0
        self.scan_blocks, self.seq_blocks = set(), set()
        self.small_denom = {f: 0 for f in FAMILIES}

    def add(self, rows, fam, small):
        for row, f, k in zip(rows, fam, small):
            if row["form"] == "scalar":
                self.scalar += 1
            else:
                self.vector_rem.add(row["rem"])
                self.vector_groups.add(min(row["groups"], 2))
            self.span20 += row["span"] == 20
            self.span21 += row["span"] >= 21
            (self.scan_blocks if row["path"] == "scan" else self.seq_blocks).add(row["blocks"])
            self.small_denom[FAMILIES[f]] += int(k)

    def missing(self):
        m = []
        if not self.scalar:
            m.append("row sum, np < 8 form")
        m += ["row sum, np >= 8 form with np %% 8 == %d" % k for k in range(8) if k not in self.vector_rem]
        m += ["row sum, np >= 8 form with %s groups of four" % ("0", "1", ">= 2")[k] for k in range(3) if k not in self.vector_groups]
        if not self.span20:
            m.append("quotient exponent span == 20 (the lane scan's last exact case)")
        if not self.span21:
            m.append("quotient exponent span >= 21 (the sequential cumsum)")
        m += ["lane scan over %d blocks of 64" % k for k in (1, 2, 3, 4) if k not in self.scan_blocks]
        m += ["sequential cumsum over %d blocks of 64" % k for k in (1, 2, 3, 4) if k not in self.seq_blocks]
        m += ["a draw with denom < 1e-5 in family %s" % f for f, k in self.small_denom.items() if not k]
        return m


# ---- merge rows ---------------------------------------------------------------------------------------------------------------
MERGE_KINDS = ("sorted", "unsorted", "flat", "repeated_u")


def merge_case(S, nf, N=22, seed=0):
    """Rays of the four kinds interleaved (ray r is kind r % 4: every 4-ray workgroup holds sorted and unsorted rows).
    sorted: stratified-like depths; unsorted: a random column permutation of them; flat: near == far, all depths equal (the new samples
    then equal them too); repeated_u: every draw appears at least twice, so samples tie."""
    rng = np.random.default_rng([seed, S, nf])
    kind = np.arange(N) % 4
    z = np.sort(rng.uniform(0.48, 1.08, (N, S)).astype(np.float32), axis=1)
    for r in np.nonzero(kind == 1)[0]:
        z[r] = z[r, rng.permutation(S)]
    z[kind == 2] = rng.uniform(0.48, 1.08, (int((kind == 2).sum()), 1)).astype(np.float32)
    w = (rng.uniform(0, 1, (N, S)) ** 6).astype(np.float32)
    u = rng.uniform(0, 1, (N, nf)).astype(np.float32)
    for r in np.nonzero(kind == 3)[0]:
        u[r] = u[r, rng.integers(0, max(1, nf // 3), nf)]
    return z, w, u, kind
