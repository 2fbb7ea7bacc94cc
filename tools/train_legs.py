"""bench.py's two training legs alone (configs[4]: fp32 backward products, and the default split-bf16 backward), optionally with the
fused backward walk switched off (--per-layer) for a same-box A/B.  --arch nerface / nerface_static: the same two legs for the
NeRFaceModels (bench.py has none): a 2,048-ray step of config/expression_hotpath.yml -- 64 + 64 samples, noise 0.1, the fused Stage-I
loss, no optimiser -- with the deformation nets (person_2/3.yml) or without (person_1.yml).  --only x3fwd --arch nerface|nerface_static:
the step with its saving forward on the split-operand kernels (ops.training_forward_precision "bf16x3") alternated with the fp32-forward
step, --repeats times each, in one process.  --optimizer (any --arch; with --only x3fwd on the split-operand saving forward): the FULL
optimisation step -- forward, loss, backward, optimiser step and the re-pack the next forward needs, weights changing every step -- with
torch.optim.Adam on an unflattened model and with training.FlatAdam on a flattened one, alternated with the fixed-weights step of the
legs above (--repeats alternations, every path warmed up, each leg ended by a device synchronise).  Prints one JSON line."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402


def nerface_leg(pkg, dev, arch, rays=2048, steps=5, warmup=2, backward="bf16x3", forward="fp32"):
    """One NeRFaceModel training step as training.train_step takes it (forward + backward through the HIP autograd op, the objective
    and its gradient inside the HIP launches), timed over `steps` after `warmup`: 2,048 rays x (64 coarse + 128 fine) samples."""
    W, Tr = pkg.weights, pkg.training
    cfg = pkg.default_config("expression" if arch == "nerface" else "expression_static")
    model = pkg.NeRFaceModel(cfg).to(dev).load_flat(W.flatten_state_dict(W.hash_state_dict(0, 8.0, 30.0, model=arch), model=arch)).train()
    g = torch.Generator(device=dev).manual_seed(3)
    H = Wd = 128
    mask = torch.zeros(H, Wd, 12, device=dev)
    mask.scatter_(2, torch.randint(0, 12, (H, Wd, 1), device=dev, generator=g), 1.0)
    sel = Tr.sample_training_rays(Tr.semantic_ray_probs(torch.ones(12, device=dev) / 12, mask), rays, g)
    expr = torch.randn(76, device=dev, generator=g) * 0.5
    pose = torch.from_numpy(np.concatenate([np.eye(3), [[0.0], [0.0], [0.5]]], 1).astype(np.float32)).to(dev)
    intr = np.array([1200.0 * H / 512, 1200.0 * H / 512, 0.5, 0.5], np.float32)
    ro, rd = pkg.get_ray_bundle(H, Wd, intr, pose)
    ro, rd = ro.reshape(-1, 3)[sel], rd.reshape(-1, 3)[sel]
    m = mask.reshape(-1, 12)[sel]
    target = torch.rand(rays, 3, device=dev, generator=g)
    bg = torch.cat([torch.rand(rays, 3, device=dev, generator=g), torch.ones(rays, 1, device=dev), torch.zeros(rays, 11, device=dev)], 1)
    cw = Tr.sample_prob_weights(dev)

    def step():
        outs = pkg.run_one_iter_of_nerf(H, Wd, intr, model, ro, rd, cfg, mode="train", driving=expr, pose=pose, background_prior=bg, inHead=m,
                                        _loss=(target, m, cw))
        model.zero_grad(set_to_none=True)
        outs[8].backward()
        return outs[8]

    before, fwd_before = pkg.ops.backward_gemm_precision(), pkg.ops.training_forward_precision()
    pkg.ops.backward_gemm_precision(backward)
    pkg.ops.training_forward_precision(forward)
    try:
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            loss = step()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
    finally:
        pkg.ops.backward_gemm_precision(before)
        pkg.ops.training_forward_precision(fwd_before)
    assert bool(torch.isfinite(loss))
    nc, nf = int(cfg.nerf.train.num_coarse), int(cfg.nerf.train.num_fine)
    return {"arch": arch, "rays": rays, "samples": [rays * nc, rays * (nc + nf)], "ms_per_step": round(dt * 1e3, 3), "steps": steps,
            "backward": backward, "forward": forward, "fused_backward": pkg.ops.fused_backward()}


def _scene(pkg, dev, arch, rays):
    """The 2,048-ray batch of bench.train_leg (audio) / nerface_leg: fixed rays, targets and conditioning."""
    W, Tr = pkg.weights, pkg.training
    if arch == "audio":
        cfg, fw = pkg.default_config(), W.flatten_state_dict(W.hash_state_dict(**bench.HDR))
        make = lambda: pkg.AudioFaceModel(cfg).to(dev).load_flat(fw).train()
    else:
        cfg = pkg.default_config("expression" if arch == "nerface" else "expression_static")
        fw = W.flatten_state_dict(W.hash_state_dict(0, 8.0, 30.0, model=arch), model=arch)
        make = lambda: pkg.NeRFaceModel(cfg).to(dev).load_flat(fw).train()
    g = torch.Generator(device=dev).manual_seed(3)
    H = Wd = 128
    mask = torch.zeros(H, Wd, 12, device=dev)
    mask.scatter_(2, torch.randint(0, 12, (H, Wd, 1), device=dev, generator=g), 1.0)
    sel = Tr.sample_training_rays(Tr.semantic_ray_probs(torch.ones(12, device=dev) / 12, mask), rays, g)
    drv = torch.randn(16, 29, device=dev, generator=g) if arch == "audio" else torch.randn(76, device=dev, generator=g) * 0.5
    pose = torch.from_numpy(np.concatenate([np.eye(3), [[0.0], [0.0], [0.8 if arch == "audio" else 0.5]]], 1).astype(np.float32)).to(dev)
    intr = np.array([1200.0 * H / 512, 1200.0 * H / 512, 0.5, 0.5], np.float32)
    ro, rd = pkg.get_ray_bundle(H, Wd, intr, pose)
    ro, rd = ro.reshape(-1, 3)[sel], rd.reshape(-1, 3)[sel]
    m = mask.reshape(-1, 12)[sel]
    target = torch.rand(rays, 3, device=dev, generator=g)
    bg = torch.cat([torch.rand(rays, 3, device=dev, generator=g), torch.ones(rays, 1, device=dev), torch.zeros(rays, 11, device=dev)], 1)
    cw = Tr.sample_prob_weights(dev)

    def forward(model):
        return pkg.run_one_iter_of_nerf(H, Wd, intr, model, ro, rd, cfg, mode="train", driving=drv, pose=pose, background_prior=bg, inHead=m,
                                        _loss=(target, m, cw))[8]

    return cfg, make, forward


def optimizer_legs(pkg, dev, arch, rays=2048, steps=50, warmup=5, repeats=3, forward="fp32", trace_steps=0):
    """Three steps on the same batch, alternated `repeats` times in one process:
      none   forward + loss + backward, weights fixed (the step of the legs above: the packed-stream cache always hits), on the `torch`
             model as the previous alternation left it
      torch  ... + torch.optim.Adam.step() on an unflattened model: torch.cat of the parameters and its backward, Adam's per-tensor
             kernels, the _version compare, the cat and the re-pack of the next forward
      flat   ... + training.FlatAdam.step() on a flattened model: one add into the flat gradient buffer, one optimiser launch, the re-pack
    trace_steps > 0: no timing, that many steps of `torch` then of `flat` (for a kernel trace)."""
    Tr = pkg.training
    cfg, make, fwd = _scene(pkg, dev, arch, rays)
    lr = float(cfg.optimizer.lr)
    # (`none` runs on the torch path's model, at whatever weights that path has reached: the step's GPU time moves with the weights, so a
    # fixed-weights figure is only comparable next to the weights it was taken at)
    models = {"torch": make(), "flat": make().flatten_parameters_()}
    models["none"] = models["torch"]
    opts = {"torch": torch.optim.Adam(models["torch"].parameters(), lr=lr), "flat": Tr.FlatAdam(models["flat"], lr=lr)}

    def step(path):
        model = models[path]
        loss = fwd(model)
        if path == "none":
            model.zero_grad(set_to_none=True)
            loss.backward()
        else:
            opts[path].zero_grad(set_to_none=True)
            loss.backward()
            opts[path].step()
        return loss

    before_fwd = pkg.ops.training_forward_precision()
    pkg.ops.training_forward_precision(forward)
    runs = {k: [] for k in models}
    try:
        if trace_steps:
            for path in ("torch", "flat"):
                for _ in range(trace_steps):
                    loss = step(path)
                torch.cuda.synchronize()
            return {"arch": arch, "forward": forward, "traced_steps_per_path": trace_steps}
        for _ in range(repeats):
            for path in ("none", "torch", "flat"):
                for _ in range(warmup):
                    step(path)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    loss = step(path)
                torch.cuda.synchronize()
                runs[path].append(round((time.perf_counter() - t0) / steps * 1e3, 3))
                assert bool(torch.isfinite(loss)), path
    finally:
        pkg.ops.training_forward_precision(before_fwd)
    med = {k: float(np.median(v)) for k, v in runs.items()}
    spread = {k: round(max(v) - min(v), 3) for k, v in runs.items()}
    return {"arch": arch, "rays": rays, "forward": forward, "steps": steps, "warmup": warmup, "repeats": repeats, "ms_runs": runs,
            "ms_median": med, "ms_spread": spread, "optimizer_cost_torch_ms": round(med["torch"] - med["none"], 3),
            "optimizer_cost_flat_ms": round(med["flat"] - med["none"], 3), "gain_ms": round(med["torch"] - med["flat"], 3),
            "flat_faster_than_torch_by_more_than_its_spread": bool(med["torch"] - med["flat"] > spread["torch"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--per-layer", action="store_true", help="keep the per-layer backward walk (ops.fused_backward(False))")
    ap.add_argument("--only", default=None, choices=["fp32", "bf16x3", "x3fwd"])
    ap.add_argument("--arch", default="audio", choices=["audio", "nerface", "nerface_static"])
    ap.add_argument("--repeats", type=int, default=3, help="--only x3fwd with a NeRFace --arch: alternations of the two steps")
    ap.add_argument("--optimizer", action="store_true", help="the full optimisation step: torch.optim.Adam vs training.FlatAdam vs no optimiser")
    ap.add_argument("--trace-steps", type=int, default=0, help="--optimizer: run that many untimed steps per path instead (for a kernel trace)")
    a = ap.parse_args()
    pkg = importlib.import_module("sahs-deformable-nerf_amd")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(0)
    pkg.ops.fused_backward(not a.per_layer)
    out = {"fused_backward": pkg.ops.fused_backward()}
    if a.optimizer:
        fwd = "bf16x3" if a.only == "x3fwd" else "fp32"
        out["optimizer_step_%s_T2048_%s" % (a.arch, "x3fwd" if fwd == "bf16x3" else "fp32fwd")] = optimizer_legs(
            pkg, dev, a.arch, steps=max(a.steps, 50) if not a.trace_steps else a.steps, warmup=a.warmup, repeats=max(a.repeats, 3), forward=fwd,
            trace_steps=a.trace_steps)
        print(json.dumps(out))
        return
    if a.arch != "audio":
        if a.only == "x3fwd":      # the fp32-forward and the x3-forward step, alternated (same process, same model, default backward)
            legs = {"fp32fwd": [], "x3fwd": []}
            for _ in range(a.repeats):
                for name, fwd in (("fp32fwd", "fp32"), ("x3fwd", "bf16x3")):
                    legs[name].append(nerface_leg(pkg, dev, a.arch, steps=a.steps, warmup=a.warmup, forward=fwd))
            for name, runs in legs.items():
                ms = [r["ms_per_step"] for r in runs]
                out["train_%s_T2048_%s" % (a.arch, name)] = dict(runs[0], ms_per_step=min(ms), ms_runs=ms)
            print(json.dumps(out))
            return
        for mode in ("fp32", "bf16x3"):
            if a.only in (None, mode):
                out["train_%s_T2048%s" % (a.arch, "" if mode == "fp32" else "_bf16x3")] = nerface_leg(pkg, dev, a.arch, steps=a.steps, warmup=a.warmup,
                                                                                                       backward=mode)
        print(json.dumps(out))
        return
    for mode in ("fp32", "bf16x3"):
        if a.only in (None, mode):
            out["train_T2048" + ("" if mode == "fp32" else "_bf16x3")] = bench.train_leg(pkg, dev, steps=a.steps, warmup=a.warmup, backward=mode)
    if a.only in (None, "x3fwd"):      # the saving forward on the split-operand kernels too (ops.training_forward_precision)
        out["train_T2048_x3fwd"] = bench.train_leg(pkg, dev, steps=a.steps, warmup=a.warmup, backward="bf16x3", forward="bf16x3")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
