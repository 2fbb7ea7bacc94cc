"""Stage-II refiner training on one GPU: what the fused SPADE backward buys (profiles/spade_train_step.json).

  python tools/time_spade_train.py [--size 512] [--steps 10] [--warmup 3] [--rounds 3] [--out profiles/spade_train_step.json]

Three measurements in one process, the fused path (ops.spade_modulate: SpadeModulateFn) and the "swapped" path (the reference's six
element-wise torch ops in its place) alternated round by round:
  * one ``spade.refine_step`` of ``Generator`` in train() mode with torch.optim.Adam on a size x size frame: ms per step, a host clock
    around ``steps`` steps that end in a device synchronise;
  * ``torch.cuda.max_memory_allocated`` over such a step, above what was allocated before it (parameters, optimiser state, inputs);
  * the op's backward alone on (1, 64, size / 2, size / 2) -- the largest SPADE layer of the network -- through the C ABI with preallocated
    buffers, HIP events around 200 launch pairs, against its algorithmic 44 B per element (16 read by the sums pass, 16 read + 12
    written by the apply pass); beside it the swapped backward of the same tensors (autograd of the six ops), for scale.
There is no CPU path: without a GPU this fails.
"""
import argparse
import copy
import importlib
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
pkg = importlib.import_module("sahs-deformable-nerf_amd")
ops, spade, _lib = pkg.ops, pkg.spade, pkg._lib
FUSED = ops.spade_modulate


def six_ops(x, gamma, beta, eps=1e-5, slope=1.0):
    """nerf/_init_spade.py:130-139 + the block's LeakyReLU, as the reference runs them."""
    return F.leaky_relu(F.instance_norm(x, eps=eps) * (1 + gamma) + beta, slope)


def steps_ms(G, opt, inputs, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = spade.refine_step(G, opt, *inputs)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, float(loss)


def step_peak_bytes(G, opt, inputs):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    spade.refine_step(G, opt, *inputs)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "spade_train_step.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_spade_train.py needs a GPU: nothing here can be measured on a CPU")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    torch.manual_seed(1)
    nets = {"fused": spade.Generator().to(dev).train()}
    nets["swapped"] = copy.deepcopy(nets["fused"])
    opts = {k: torch.optim.Adam(G.parameters(), lr=2e-4, betas=(0.5, 0.999)) for k, G in nets.items()}
    inputs = tuple(torch.rand(1, 3, args.size, args.size, device=dev, generator=gen) for _ in range(3))
    modes = {"fused": FUSED, "swapped": six_ops}
    step = {k: {"ms_per_step": [], "peak_bytes_above_resident": []} for k in modes}
    for k in modes:      # warm-up: MIOpen picks its algorithms, Adam allocates its state
        ops.spade_modulate = modes[k]
        step[k]["first_loss"] = steps_ms(nets[k], opts[k], inputs, args.warmup)[1]
    for _ in range(args.rounds):
        for k in modes:
            ops.spade_modulate = modes[k]
            step[k]["ms_per_step"].append(steps_ms(nets[k], opts[k], inputs, args.steps)[0])
            step[k]["peak_bytes_above_resident"].append(step_peak_bytes(nets[k], opts[k], inputs))
    ops.spade_modulate = FUSED
    for k in modes:
        step[k]["ms_per_step_best"] = min(step[k]["ms_per_step"])
    # the op's backward alone
    C, H = 64, args.size // 2
    x, gamma, beta, g = (torch.randn(1, C, H, H, device=dev, generator=gen) for _ in range(4))
    L, P, st = _lib.lib(), ops._p, ops._stream()
    out, stats = torch.empty_like(x), torch.empty(int(L.sahs_spade_modulate_workspace_words(C)), device=dev)
    _lib.check(L.sahs_spade_modulate(C, H * H, P(x), P(gamma), P(beta), 1e-5, 0.2, P(out), P(stats), st), "sahs_spade_modulate")
    dx, dgamma, dbeta = (torch.empty_like(x) for _ in range(3))
    work = torch.empty(int(L.sahs_spade_modulate_backward_workspace_words(C)), device=dev)
    fused_bwd = lambda: _lib.check(L.sahs_spade_modulate_backward(C, H * H, P(x), P(gamma), P(out), P(stats), P(g), 1e-5, 0.2, P(dx), P(dgamma),
                                                                  P(dbeta), P(work), st), "sahs_spade_modulate_backward")
    leaves = [t.clone().requires_grad_(True) for t in (x, gamma, beta)]
    y = six_ops(*leaves, slope=0.2)
    swapped_bwd = lambda: torch.autograd.grad(y, leaves, g, retain_graph=True)
    op = {"fused_ms": [], "swapped_ms": []}
    for _ in range(args.rounds):
        op["fused_ms"].append(events_ms(fused_bwd, 200))
        op["swapped_ms"].append(events_ms(swapped_bwd, 50))
    ref = torch.autograd.grad(y, leaves, g, retain_graph=True)
    nbytes = 44 * x.numel()
    best = min(op["fused_ms"])
    op.update(shape=[1, C, H, H], bytes_per_element=44, fused_ms_best=best, swapped_ms_best=min(op["swapped_ms"]),
              fused_GB_per_s=nbytes / best / 1e6, hbm_peak_GB_per_s=8000.0, fused_fraction_of_hbm_peak=nbytes / best / 1e6 / 8000.0,
              max_abs_diff_vs_swapped=[float((a - b).abs().max()) for a, b in zip((dx, dgamma, dbeta), ref)],
              timing="HIP events on the launch stream: 200 sahs_spade_modulate_backward calls (two launches each) on preallocated buffers; "
                     "swapped = 50 torch.autograd.grad calls through the six ops' graph (allocations and launch pacing included)",
              note="the seven tensors of the fused backward (112 MB at 512) fit the 256 MB last-level cache: the rate is not an HBM rate")
    result = {"command": "python tools/time_spade_train.py --size %d --steps %d --warmup %d --rounds %d" % (args.size, args.steps, args.warmup, args.rounds), "device": torch.cuda.get_device_name(0),
              "torch": torch.__version__, "workload": "Generator.train(), refine_step (forward, clamp, MSE, backward, Adam) on a %dx%d frame, fp32; "
              "convolutions on MIOpen in both modes" % (args.size, args.size), "steps_per_window": args.steps, "rounds": args.rounds,
              "step": step, "step_speedup_fused_vs_swapped": step["swapped"]["ms_per_step_best"] / step["fused"]["ms_per_step_best"],
              "step_peak_bytes_ratio_fused_vs_swapped": max(step["fused"]["peak_bytes_above_resident"]) / max(step["swapped"]["peak_bytes_above_resident"]),
              "op_backward": op}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
