"""The fused image objective on one GPU: forward + backward against the same objective composed in torch, and one refiner step with
and without it (profiles/image_loss.json).

  python tools/time_image_loss.py [--size 512] [--rounds 3] [--reps 100] [--steps 10] [--out profiles/image_loss.json]

Op level, size x size x 3 at B = 1 and B = 8, weights (1, 1, 1), clamp on, (B, 3, H, W) tensors as the refiner emits them.  Two variants
alternated round by round in one process, HIP events around ``reps`` calls of forward + backward on preallocated inputs:
  * fused: ops.image_loss (two launches forward, the gradient image formed there; backward one scaling);
    also sahs_image_loss alone through the C ABI on preallocated buffers -- the two kernels without autograd around them -- with
    and without a gradient pointer (kernels_ms, kernels_no_gradient_ms);
  * torch: tests/image_loss_reference.py's torch_composition -- clamp, mse_loss, l1_loss and SSIM as five avg_pool2d moment planes with
    raw-moment variances -- and its autograd backward.  Its allocations go through torch's caching allocator (warm after the first
    call); both variants' launches are counted with torch.profiler in a call outside the timed windows.
Step level: ``spade.refine_step`` of ``Generator`` in train() mode with torch.optim.Adam on a size x size frame, three copies of one
initialisation alternated round by round: loss=None (clamp and mse_loss in torch), RefineLoss(l2=1) (the same objective, fused) and
RefineLoss(1, 1, 1); ms per step by a host clock around ``steps`` steps that end in a device synchronise.
The file records each comparison against the rounds' own min-max spread -- fused_faster_beyond_spread: max of the fused rounds < min of
torch's; not_slower_beyond_spread: not (min of the fused rounds > max of the other's) -- whichever way it comes out; nothing is tuned
to make it hold.  It also records both variants' gradient errors against the float64 reference at 128 x 128 for a generic pair and the
flat bright pair.  There is no CPU path: without a GPU this fails.
"""
import argparse
import copy
import ctypes
import importlib
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import image_loss_reference as R      # noqa: E402  (the float64 references and the torch composition the GPU tests use)
import metrics_reference as M      # noqa: E402

pkg = importlib.import_module("sahs-deformable-nerf_amd")
ops, spade, _lib = pkg.ops, pkg.spade, pkg._lib
WEIGHTS = (1.0, 1.0, 1.0)


def events_ms(fn, reps):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def count_launches(fn):
    """Device kernels of one call, by torch.profiler -> int, or a string saying why it could not be counted."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
        return n if n > 0 else "not counted: the profiler recorded no device events"
    except Exception as exc:      # noqa: BLE001  (a profiler that cannot start must not lose the timings)
        return "not counted: %s" % exc


def abi_call(pred, target, with_grad):
    """pred, target: (B, 3, H, W) -> a closure of one sahs_image_loss call (the two kernels alone) on preallocated buffers."""
    L, P, st = _lib.lib(), ops._p, ops._stream()
    p, t = pred.detach().permute(0, 2, 3, 1), target.permute(0, 2, 3, 1)
    B, H, W, C = p.shape
    grad = torch.empty_like(p) if with_grad else None
    out = torch.empty(4 + 3 * B, dtype=torch.float64, device=p.device)
    need = int(L.sahs_image_loss_workspace_bytes(B, H, W, C))
    work = torch.empty(need // 8, dtype=torch.float64, device=p.device)
    sp, stt = (ctypes.c_long * 4)(*p.stride()), (ctypes.c_long * 4)(*t.stride())
    sg = (ctypes.c_long * 4)(*grad.stride()) if with_grad else None
    return lambda: _lib.check(L.sahs_image_loss(P(p), P(t), B, H, W, C, sp, stt, WEIGHTS[0], WEIGHTS[1], WEIGHTS[2], 1, 1.0, P(grad), sg, P(out),
                                                P(work), need, st), "sahs_image_loss")


def forward_backward(loss_fn, pred, target):
    """-> a closure of one forward + backward; pred is a leaf whose .grad is dropped each call (so the backward writes, not accumulates)."""
    def call():
        pred.grad = None
        loss_fn(pred, target).backward()
    return call


def steps_ms(G, opt, inputs, steps, loss):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        value = spade.refine_step(G, opt, *inputs, loss=loss)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, float(value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "image_loss.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_image_loss.py needs a GPU: nothing here can be measured on a CPU")
    dev = torch.device("cuda:0")
    S = args.size
    rng = np.random.default_rng(3)

    def pair(B, size):
        items = [M.ramp_noise_pair(size, size, 3, 0.01 * (i + 1), 20 + i, np.float32) for i in range(B)]
        a, b = (np.stack(x) for x in zip(*items))
        pred = (a + 0.15 * rng.standard_normal(a.shape)).astype(np.float32)
        return (torch.from_numpy(x).to(dev).permute(0, 3, 1, 2).contiguous() for x in (pred, b))

    shapes = {}
    for B in (1, 8):
        pred, target = pair(B, S)
        pred.requires_grad_(True)
        fused = forward_backward(lambda p, t: ops.image_loss(p, t, *WEIGHTS), pred, target)
        composed = forward_backward(lambda p, t: R.torch_composition(p, t, WEIGHTS), pred, target)
        fused()
        g_fused = pred.grad.clone()
        composed()
        scale = float(g_fused.abs().max())
        rec = {"fused_ms": [], "torch_ms": [], "fused_launches": count_launches(fused), "torch_launches": count_launches(composed),
               "max_abs_gradient_difference_over_max_gradient": float((pred.grad - g_fused).abs().max()) / scale,
               "image_bytes": {"read_once": 2 * pred.numel() * 4, "gradient_written": pred.numel() * 4}}
        kernels, kernels_no_grad = abi_call(pred, target, True), abi_call(pred, target, False)
        rec.update(kernels_ms=[], kernels_no_gradient_ms=[])
        for _ in range(args.rounds):
            rec["fused_ms"].append(events_ms(fused, args.reps))
            rec["torch_ms"].append(events_ms(composed, max(args.reps // 4, 1)))
            rec["kernels_ms"].append(events_ms(kernels, args.reps))
            rec["kernels_no_gradient_ms"].append(events_ms(kernels_no_grad, args.reps))
        rec.update(fused_ms_best=min(rec["fused_ms"]), torch_ms_best=min(rec["torch_ms"]), speedup_best=min(rec["torch_ms"]) / min(rec["fused_ms"]),
                   fused_faster_beyond_spread=max(rec["fused_ms"]) < min(rec["torch_ms"]))
        shapes["B%d" % B] = rec

    # one refiner step: three copies of one initialisation, alternated
    torch.manual_seed(1)
    first = spade.Generator().to(dev).train()
    variants = {"loss_none": None, "refine_loss_l2": spade.RefineLoss(l2=1.0), "refine_loss_l2_l1_ssim": spade.RefineLoss(1.0, 1.0, 1.0)}
    nets = {k: copy.deepcopy(first) for k in variants}
    opts = {k: torch.optim.Adam(nets[k].parameters(), lr=2e-4, betas=(0.5, 0.999)) for k in variants}
    gen = torch.Generator(device=dev).manual_seed(1)
    inputs = tuple(torch.rand(1, 3, S, S, device=dev, generator=gen) for _ in range(3))
    step = {k: {"ms_per_step": [], "loss_after_window": []} for k in variants}
    for k in variants:
        steps_ms(nets[k], opts[k], inputs, 3, variants[k])      # warm-up: MIOpen picks its algorithms, the allocator its blocks
    for _ in range(args.rounds):
        for k in variants:
            ms, value = steps_ms(nets[k], opts[k], inputs, args.steps, variants[k])
            step[k]["ms_per_step"].append(ms)
            step[k]["loss_after_window"].append(value)
    for k in variants:
        step[k]["ms_best"] = min(step[k]["ms_per_step"])
    for k in ("refine_loss_l2", "refine_loss_l2_l1_ssim"):
        step[k]["not_slower_than_loss_none_beyond_spread"] = not min(step[k]["ms_per_step"]) > max(step["loss_none"]["ms_per_step"])

    # gradient errors against float64 (128 x 128 x 3: the reference forms every window)
    errors = {}
    for name, (a, b) in (("noise0.03", M.ramp_noise_pair(128, 128, 3, 0.03, 1, np.float32)), ("flat_bright", M.flat_bright_pair(128, 128, 3, np.float32))):
        p = (a + 0.15 * rng.standard_normal(a.shape)).astype(np.float32)
        g64 = R.combine(*R.closed_terms(p, b), WEIGHTS)[1]
        got = {}
        for key, fn in (("fused", lambda x, t: ops.image_loss(x, t, *WEIGHTS)), ("torch", lambda x, t: R.torch_composition(x, t, WEIGHTS))):
            leaf = torch.from_numpy(p).to(dev).permute(2, 0, 1)[None].contiguous().requires_grad_(True)
            fn(leaf, torch.from_numpy(b).to(dev).permute(2, 0, 1)[None].contiguous()).backward()
            got[key + "_gradient_E"] = R.grad_error(leaf.grad[0].permute(1, 2, 0).double().cpu().numpy(), g64, WEIGHTS)
        errors[name] = got

    result = {"command": "python tools/time_image_loss.py --size %d --rounds %d --reps %d --steps %d" % (S, args.rounds, args.reps, args.steps),
              "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
              "workload": "loss = MSE + L1 + (1 - SSIM) of clamp(pred, 0, 1) against a target, %dx%dx3 fp32 (B, 3, H, W), forward + backward; fused = "
                          "ops.image_loss, torch = clamp, mse_loss, l1_loss and five avg_pool2d moment planes (tests/image_loss_reference.py: "
                          "torch_composition); refine_step: Generator.train() with Adam on one %dx%d frame" % (S, S, S, S),
              "timing": "op: HIP events on the launch stream around %d fused and %d torch forward + backward calls per round, alternated, %d rounds "
                        "(the tensors of one call fit the 256 MB last-level cache: the rates are not HBM rates); step: a host clock around %d steps "
                        "ending in a device synchronise, the three variants alternated, %d rounds"
                        % (args.reps, max(args.reps // 4, 1), args.rounds, args.steps, args.rounds),
              "rule": "fused_faster_beyond_spread: max(fused rounds) < min(torch rounds); not_slower_than_loss_none_beyond_spread: not "
                      "min(variant rounds) > max(loss=None rounds)",
              "op_forward_backward": shapes, "refine_step": step, "gradient_errors_vs_float64_128x128": errors}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
