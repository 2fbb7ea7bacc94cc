"""The dense-against-sparse recipe of the fp32 inference render, shared by tests/test_gpu_sparse_branches.py, tests/test_gpu_sparse_pipeline.py
and tests/test_gpu_sparse_fused.py.  TEST INFRASTRUCTURE ONLY.

 * setup / scene: packed weights with a chosen density bias and seeded rays, draws, background prior and noise.
 * render: one ops.render_rays_rows call with the sparse branches on or off -> rows, depths, weights, raw, live count, head word.
 * compare: the sparse render against the dense one (ops.sparse_branches(False)), the reference everywhere: rows, depths and weights
   bit for bit, the raw rows of the live samples, every sigma, raw finite, the live count exact, the head's second word 1.
"""
import torch

from conftest import pkg

NC = 64
TILE = 128
_CACHE = {}
# density_bias of the NeRFaceModels' cases: 2.0 minus the median sigma of the dense fine pass of scene(arch, 129, 64) with density_bias 2.0,
# measured once on MI355X: 19.1422 and -14.4984
CENTRED_BIAS = {"nerface": -17.1422, "nerface_static": 16.4984}


def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def cus():
    return torch.cuda.get_device_properties(dev()).multi_processor_count


def tiles(samples):
    return (samples + TILE - 1) // TILE


def default_bias(arch):
    """density_bias of a case.  AudioFaceModel: 2.0 -- hash_state_dict(0, 2.0, 30.0, hdr=True) centres that model's density logit, so 35-65 %
    of its samples are dead.  The NeRFaceModels' synthetic weights are not centred (weights.py does it for the audio model only): with 2.0
    every sigma is positive and only the last sample of a ray is dead (1.6 % measured), so a dense-against-sparse comparison would compare
    the dense path with itself.  sigma is affine in fc_alpha.bias, so for them the bias is moved by the median sigma of a dense render
    (CENTRED_BIAS): the same weights otherwise (seed 0, gain 30, hdr), and the same 20-80 % assertion on the dead fraction as for the audio
    model."""
    return 2.0 if arch == "audio" else CENTRED_BIAS[arch]


def setup(arch, density_bias):
    """packed fp32 weights and the folded frame of hash_state_dict(0, density_bias, 30.0, hdr=True), once per (arch, bias)"""
    key = (arch, float(density_bias))
    if key not in _CACHE:
        ops, W = pkg("ops"), pkg("weights")
        d = dev()
        flat = torch.from_numpy(W.flatten_state_dict(W.hash_state_dict(0, density_bias, 30.0, model=arch, hdr=True), model=arch)).to(d)
        g = torch.Generator(device=d).manual_seed(5)
        drv = torch.randn(16, 29, device=d, generator=g) if arch == "audio" else torch.randn(76, device=d, generator=g) * 0.5
        cam = 0.8 if arch == "audio" else 0.5
        pose = torch.tensor([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, cam]], device=d)
        _CACHE[key] = (ops.pack_weights(flat, ops.SAHS_F32, arch=arch), ops.fold_conditioning(flat, drv, pose, arch=arch))
    return _CACHE[key]


def scene(arch, N, nf, noise_std=0.0, with_bg=True, nc=NC):
    d = dev()
    cam = 0.8 if arch == "audio" else 0.5
    g = torch.Generator(device=d).manual_seed(1000 * N + nf)
    near, far = (0.483771, 1.083771) if arch == "audio" else (0.2, 0.8)
    rays = torch.zeros(N, 8, device=d)
    rays[:, 2] = cam
    rays[:, 3:6] = torch.randn(N, 3, device=d, generator=g) * 0.15 + torch.tensor([0, 0, -1.0], device=d)
    rays[:, 6], rays[:, 7] = near, far
    kw = dict(t_rand=torch.rand(N, nc, device=d, generator=g))
    if nf > 0:
        kw["u"] = torch.rand(N, nf, device=d, generator=g)
    if with_bg:
        kw["bg"] = torch.cat([torch.rand(N, 3, device=d, generator=g), torch.ones(N, 1, device=d), torch.zeros(N, 11, device=d)], 1)
    if noise_std > 0.0:
        kw["noise_c"] = torch.randn(N, nc, device=d, generator=g) * noise_std
        if nf > 0:
            kw["noise_f"] = torch.randn(N, nc + nf, device=d, generator=g) * noise_std
    return rays, kw


def render(arch, rays, nf, kw, sparse, share=True, density_bias=None, nc=NC, ws=None):
    """-> rows, depths, weights, raw of the last pass, live count of the last pass and the head's second word (sparse only)"""
    ops = pkg("ops")
    packed, frame = setup(arch, default_bias(arch) if density_bias is None else density_bias)
    rows = torch.full((rays.shape[0], 36), float("nan"), device=rays.device)
    ws = {} if ws is None else ws
    was = ops.sparse_branches()
    ops.sparse_branches(sparse)
    try:
        ops.render_rays_rows(packed, frame, rays, nc, nf, rows, workspace=ws, arch=arch, share_deformation=share, **kw)
    finally:
        ops.sparse_branches(was)
    assert ("sparse" in ws) == sparse
    if nf == 0:      # (no fine pass: columns 17..33, rgb_f / disp_f / acc_f, are not written and keep their NaN)
        rows = torch.cat([rows[:, :17], rows[:, 34:]], 1)
    assert bool(torch.isfinite(rows).all()), "a rendered row holds a value that was not written"
    z = ws["z_f"] if nf > 0 else ws["z_c"]
    S = nc + nf
    # (without a fine pass the raw and weights workspaces are the coarse pass's: the first nc columns' worth of the flat buffers)
    raw = ws["raw"].reshape(-1)[:rays.shape[0] * S * 16].reshape(rays.shape[0], S, 16)
    wts = ws["weights"].reshape(-1)[:rays.shape[0] * S].reshape(rays.shape[0], S)
    return (rows, z.clone(), wts.clone(), raw.clone(), (ops.sparse_last_count(ws) if sparse else None),
            (ops.sparse_last_path(ws) if sparse else None))


def live_mask(raw, noise, with_bg):
    """the samples whose colour and seg logits the composite can use (render_ops.hip: sg = max(sigma + noise, 0); the last sample always has
    a weight, but a background prior replaces its channels)"""
    sg = raw[..., 15] + (noise if noise is not None else 0.0)
    live = sg > 0.0
    live[:, -1] = not with_bg
    return live


def compare(dense, sparse, noise, with_bg, what):
    """rows, depths, weights; raw of the live samples; sigma of all samples; raw finite; the count; the head word -> live mask"""
    for a, b, nm in zip(dense[:3], sparse[:3], ("rows", "depths", "weights")):
        assert torch.equal(a, b), "%s: %s differs (max %.3e)" % (what, nm, float((a - b).abs().max()))
    rd, rs = dense[3], sparse[3]
    live = live_mask(rd, noise, with_bg)
    assert torch.equal(rd[live], rs[live]), what + ": raw rows of live samples differ"
    assert torch.equal(rd[..., 15], rs[..., 15]), what + ": sigma differs"
    assert bool(torch.isfinite(rs).all()), what + ": raw is not finite"
    assert sparse[4] == int(live.sum()), what + ": %d records, %d live samples" % (sparse[4], int(live.sum()))
    assert sparse[5] == 1, what + ": the head's second word is %d" % sparse[5]
    return live
