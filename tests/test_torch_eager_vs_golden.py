"""Pin the torch-eager restatement (oracle/torch_eager.py: gradient oracle + "reference PyTorch path" baseline)
to the real reference's golden vectors: forward seams, end-to-end renders and parameter gradients."""
import numpy as np
import pytest
import torch

from conftest import golden_rand, golden_weights_kw, load_golden, yardstick
from oracle import torch_eager as TE


def sd_torch(weights_mod, seed, bias, gain, requires_grad=False, hdr=False):
    sd = {k: torch.from_numpy(v.copy()) for k, v in weights_mod.hash_state_dict(seed, bias, gain, hdr=hdr).items()}
    if requires_grad:
        for v in sd.values():
            v.requires_grad_(True)
    return sd


def close(a, b, rtol, atol, what=""):
    a = a.detach().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    err = np.abs(a.astype(np.float64) - np.asarray(b, np.float64))
    tol = atol + rtol * np.abs(np.asarray(b, np.float64))
    assert a.shape == np.asarray(b).shape, (what, a.shape, np.asarray(b).shape)
    assert np.all(err <= tol), "%s: max err %.3e" % (what, err.max())


@pytest.mark.parametrize("variant,kw", [("default", (0, 0.0, 1.0)), ("boosted", (0, 8.0, 30.0)), ("hdr", (0, 2.0, 30.0, False, True))])
def test_field(weights_mod, variant, kw):
    g = load_golden("field")
    f = TE.EagerField(sd_torch(weights_mod, *kw))
    x = torch.from_numpy(g["x"])
    with torch.no_grad():
        for lvl in ("coarse", "fine"):
            out = f.forward(lvl, x, torch.from_numpy(g["audio"]), torch.from_numpy(g["pose"]))
            close(out, g[variant + "_raw_" + lvl], 1e-4, 1e-5 * (1 if variant == "default" else 30), "raw " + lvl)
            yardstick(out, g[variant + "_raw_" + lvl], g[variant + "_raw_" + lvl + "_f64"], "eager field[%s] raw %s" % (variant, lvl))


def _rand_chunks(g, nchunks):
    log = golden_rand(g)
    per = len(log) // nchunks
    keys = {4: ["t_rand", "noise_c", "u", "noise_f"], 2: ["t_rand", "u"], 0: []}[per]
    std = float(g["noise_std"]) if "noise_std" in g else 0.1
    return [{k: torch.from_numpy(arr) * (std if k.startswith("noise") else 1.0) for k, (_, arr) in zip(keys, log[c * per:(c + 1) * per])}
            for c in range(nchunks)]


@pytest.mark.parametrize("name,nchunks", [("e2e_boosted_val", 1), ("e2e_boosted_val_2chunks", 2), ("e2e_boosted_det", 1),
                                          ("e2e_boosted_train_noise", 1), ("e2e_hdr_val", 1), ("e2e_hdr_train_noise", 1)])
def test_end_to_end(weights_mod, name, nchunks):
    g = load_golden(name)
    kw = golden_weights_kw(g)
    f = TE.EagerField(sd_torch(weights_mod, kw["seed"], kw["density_bias"], kw["density_gain"], hdr=kw["hdr"]))
    with torch.no_grad():
        outs = TE.run_one_iter(f, torch.from_numpy(g["ro"]), torch.from_numpy(g["rd"]), float(g["near"]), float(g["far"]),
                               torch.from_numpy(g["audio"]), torch.from_numpy(g["pose"]), chunksize=int(g["chunksize"]),
                               bg=torch.from_numpy(g["bg"]), rand=_rand_chunks(g, nchunks), perturb=bool(g["perturb"]),
                               noise_std=float(g["noise_std"]))
    for nm, o in zip(["rgb_c", "disp_c", "acc_c", "rgb_f", "disp_f", "acc_f", "w_bg", "depth_f"], outs):
        if "hdr" not in name:      # SURVEY 8d's fp32 tolerance; the hdr network is held to the float64 yardstick instead
            close(o, g["out_" + nm].reshape(o.shape), 1e-4, 2e-5, name + ":" + nm)
        yardstick(o, g["out_" + nm], g["f64_" + nm], "eager %s:%s" % (name, nm), outlier_rays=0.0 if nm.endswith("_c") else 0.02, scale_floor=1.0,
                  ray_shape=(int(g["H"]) * int(g["W"]),))


def test_gradients(weights_mod):
    """config[4] semantics: train mode, noise 0.1, loss = <rgb_c,A> + <rgb_f,B> + 0.1*sum(depth_f)."""
    g = load_golden("train_grads")
    sd = sd_torch(weights_mod, 0, 8.0, 30.0, requires_grad=True)
    f = TE.EagerField(sd)
    audio = torch.from_numpy(g["audio"]).requires_grad_(True)
    mask = torch.zeros(32, 12)
    mask[:, 0] = 1.0
    log = golden_rand(g)
    rand = [dict(t_rand=torch.from_numpy(log[0][1]), noise_c=torch.from_numpy(log[1][1]) * 0.1, u=torch.from_numpy(log[2][1]),
                 noise_f=torch.from_numpy(log[3][1]) * 0.1)]
    outs = TE.run_one_iter(f, torch.from_numpy(g["ro"]), torch.from_numpy(g["rd"]), float(g["near"]), float(g["far"]), audio,
                           torch.from_numpy(g["pose"]), bg=torch.from_numpy(g["bg"]), rand=rand, perturb=True, noise_std=0.1, mask=mask)
    loss = (outs[0] * torch.from_numpy(g["A"])).sum() + (outs[3] * torch.from_numpy(g["B"])).sum() + outs[7].sum() * 0.1
    assert abs(loss.item() - float(g["loss"])) < 1e-3 * abs(float(g["loss"])) + 1e-4
    loss.backward()
    names = [str(n) for n in g["grad_names"]]
    norms = g["grad_norms"]
    for k, ref_norm in zip(names, norms):
        gr = sd[k].grad
        n = 0.0 if gr is None else float(gr.double().norm())
        assert abs(n - ref_norm) <= 2e-3 * ref_norm + 1e-7, (k, n, ref_norm)
        if "grad_" + k in g.keys():
            close(gr, g["grad_" + k], 5e-3, 2e-3 * float(np.abs(g["grad_" + k]).max()) + 1e-9, "grad " + k)
    close(audio.grad, g["grad_audio"], 5e-3, 2e-3 * float(np.abs(g["grad_audio"]).max()), "grad audio")


@pytest.mark.parametrize("arch", ["nerface", "nerface_static"])
def test_nerface_forward_and_gradients(weights_mod, arch):
    """The NeRFaceModel architectures of the eager restatement (the gradient oracle of their HIP backward): forward seam and the
    reference's own parameter / expression gradients (tests/golden/make_golden_nerface.py, train mode, noise 0.1)."""
    sd = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in weights_mod.hash_state_dict(0, 8.0, 30.0, model=arch).items()}
    f = TE.EagerField(sd, arch=arch)
    fld = load_golden(arch + "_field")
    with torch.no_grad():
        out = f.forward("fine", torch.from_numpy(fld["x"]), torch.from_numpy(fld["expression"]), torch.from_numpy(fld["pose"]))
    tol = 2e-3 if arch == "nerface" else 1e-4      # 15 octaves: see test_oracle_nerface_vs_golden.py
    close(out[:, :15], fld["boosted_raw_fine"][:, :15], tol, tol, "raw fine")
    g = load_golden(arch + "_train_grads")
    expr = torch.from_numpy(g["expression"]).requires_grad_(True)
    mask = torch.zeros(32, 12)
    mask[:, 0] = 1.0
    log = golden_rand(g)
    rand = [dict(t_rand=torch.from_numpy(log[0][1]), noise_c=torch.from_numpy(log[1][1]) * 0.1, u=torch.from_numpy(log[2][1]),
                 noise_f=torch.from_numpy(log[3][1]) * 0.1)]
    outs = TE.run_one_iter(f, torch.from_numpy(g["ro"]), torch.from_numpy(g["rd"]), float(g["near"]), float(g["far"]), expr,
                           torch.from_numpy(g["pose"]), bg=torch.from_numpy(g["bg"]), rand=rand, perturb=True, noise_std=0.1, mask=mask)
    loss = (outs[0] * torch.from_numpy(g["A"])).sum() + (outs[3] * torch.from_numpy(g["B"])).sum() + outs[7].sum() * 0.1
    # the 15-octave model's fine pass is ill-conditioned in the resampled depths (a 1e-5 depth change turns the top octave by
    # 0.16 rad), and so are its gradients: norms to 3 %, entries to 5 % of the tensor's scale; the 10-octave one as the audio model
    rn, ra = (3e-2, 5e-2) if arch == "nerface" else (2e-3, 2e-3)
    assert abs(loss.item() - float(g["loss"])) < rn * abs(float(g["loss"])) + 1e-3
    loss.backward()
    for k, ref_norm in zip([str(n) for n in g["grad_names"]], g["grad_norms"]):
        gr = sd[k].grad
        n = 0.0 if gr is None else float(gr.double().norm())
        assert abs(n - ref_norm) <= rn * ref_norm + 1e-7, (k, n, ref_norm)
        if "grad_" + k in g.keys():
            close(gr, g["grad_" + k], 5e-3, ra * float(np.abs(g["grad_" + k]).max()) + 1e-9, "grad " + k)
    close(expr.grad, g["grad_expression"], 5e-3, ra * float(np.abs(g["grad_expression"]).max()), "grad expression")


@pytest.mark.parametrize("arch", ["audio", "nerface", "nerface_static"])
def test_field_conditioning_hooks(weights_mod, arch):
    """EagerField.forward with the conditioning given precomputed (driving=, pose36=) and the seam tapped (taps=), the form the float64
    gradient tests of the HIP backward use (tests/test_gpu_backward_tails.py), equals the default call bit for bit, forward and float64
    gradients, at a tiny P; and the tapped seam carries the gradient that reaches the deformation nets."""
    sd_np = weights_mod.hash_state_dict(0, 8.0, 30.0, model=arch) if arch != "audio" else weights_mod.hash_state_dict(0, 8.0, 30.0)
    gen = torch.Generator().manual_seed(3)
    P = 5
    x = torch.cat([torch.rand(P, 3, generator=gen, dtype=torch.float64) * 0.4 - 0.2, torch.randn(P, 3, generator=gen, dtype=torch.float64)], 1)
    cond = torch.randn(16, 29, generator=gen, dtype=torch.float64) if arch == "audio" else torch.randn(76, generator=gen, dtype=torch.float64) * 0.5
    pose = torch.from_numpy(np.concatenate([np.eye(3), [[0.0], [0.0], [0.5]]], 1))
    d_raw = torch.randn(P, 16, generator=gen, dtype=torch.float64)

    def run(hooked):
        sd = {k: torch.from_numpy(v.copy()).double().requires_grad_(True) for k, v in sd_np.items()}
        c = cond.clone().requires_grad_(True)
        f = TE.EagerField(sd, num_coarse=P, num_fine=0, arch=arch)
        taps = {}
        if hooked:
            drv = f.audionet(c) if arch == "audio" else c
            raw = f.forward("fine", x, None, None, driving=drv, pose36=f.pose_encoding(pose), taps=taps)
        else:
            raw = f.forward("fine", x, c, pose)
        (raw * d_raw).sum().backward()
        return raw.detach(), {k: v.grad for k, v in sd.items()}, c.grad, taps

    raw0, g0, c0, _ = run(False)
    raw1, g1, c1, taps = run(True)
    assert torch.equal(raw0, raw1)
    assert g0.keys() == g1.keys()
    for k in g0:
        assert (g0[k] is None) == (g1[k] is None), k
        if g0[k] is not None:
            assert torch.equal(g0[k], g1[k]), k
    assert torch.equal(c0, c1)
    assert ("warped" in taps) == (arch != "nerface_static")
    if "warped" in taps:
        assert taps["warped"].shape == (P, 3) and taps["amb"].shape == (P, 2 if arch == "audio" else 1)
        # the seam: d raw-loss / d (x', w) through the radiance net, pulled back through the deformation nets, is the deformation nets'
        # whole gradient (they reach the output through x' and w only)
        sd ={k: torch.from_numpy(v.copy()).double().requires_grad_(True) for k, v in sd_np.items()}
        f = TE.EagerField(sd, num_coarse=P, num_fine=0, arch=arch)
        taps = {}
        drv = f.audionet(cond) if arch == "audio" else cond
        raw = f.forward("fine", x, None, None, driving=drv, pose36=f.pose_encoding(pose), taps=taps)
        gw, ga = torch.autograd.grad((raw * d_raw).sum(), [taps["warped"], taps["amb"]], retain_graph=True)
        k = "warp_field_mlp.fc_final.bias"
        via_seam = torch.autograd.grad((taps["warped"] * gw).sum(), [sd[k]])[0]
        assert torch.allclose(via_seam, g0[k], rtol=1e-12, atol=1e-15), k
