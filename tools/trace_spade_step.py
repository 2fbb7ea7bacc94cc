"""A few Stage-II training steps to run under a kernel trace (profiles/spade_bf16_step_kernel_stats_before.csv):

  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/trace_spade_step.py [--precision bf16|fp32] [--steps 8]
  python tools/summarize_profiles.py --steady DIR/*/*_kernel_trace.csv adam_step_kernel 3 OUT.csv "header"

``refine_step`` of ``Generator`` in train() mode on a 512 x 512 frame, with torch.optim.Adam; prints the wall time of every step.  After
every step the program launches one marker kernel (this library's adam_step on four floats -- the step itself uses torch's optimiser, so
the name is the marker's alone) and synchronises: the summary counts only the steps behind the first few markers, when the library has
chosen its algorithms (its first-call search runs reference convolutions that take a hundred times the step).
--host-profile N: after the steps, N more under torch.profiler, and the table of the operators by their own host time: the kernel trace
says how long the GPU works in a step, this says where the host spends the step while it does not.
--power-iteration fp32: an experiment, defined here and not shipped -- spectral norm's power iteration (two matrix-vector products and a
dot product per normalised convolution and step) runs with autocast switched off, i.e. in fp32 as in the fp32 step.
--spectral-norm fused: the steps run on ``spade.fuse_spectral_norm_(G)`` -- every normalised weight from the fused op.
--rounds R: after the steps, R windows of ten steps, each ending in a synchronise: ms per step, a host clock.
There is no CPU path."""
import argparse
import importlib
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pkg = importlib.import_module("sahs-deformable-nerf_amd")

ap = argparse.ArgumentParser()
ap.add_argument("--precision", choices=("bf16", "fp32"), default="bf16")
ap.add_argument("--power-iteration", choices=("autocast", "fp32"), default="autocast")
ap.add_argument("--spectral-norm", choices=("hooks", "fused"), default="hooks")
ap.add_argument("--steps", type=int, default=8)
ap.add_argument("--size", type=int, default=512)
ap.add_argument("--host-profile", type=int, default=0)
ap.add_argument("--rounds", type=int, default=0)
args = ap.parse_args()
if args.power_iteration == "fp32":
    sn = importlib.import_module("torch.nn.utils.spectral_norm").SpectralNorm
    compute_weight = sn.compute_weight

    def outside_autocast(self, module, do_power_iteration):
        with torch.autocast("cuda", enabled=False):
            return compute_weight(self, module, do_power_iteration)

    sn.compute_weight = outside_autocast
dev = torch.device("cuda:0")
torch.manual_seed(1)
gen = torch.Generator(device=dev).manual_seed(1)
G = pkg.spade.Generator().to(dev).train()
if args.spectral_norm == "fused":
    pkg.spade.fuse_spectral_norm_(G)
opt = torch.optim.Adam(G.parameters(), lr=2e-4, betas=(0.5, 0.999))
inputs = tuple(torch.rand(1, 3, args.size, args.size, device=dev, generator=gen) for _ in range(3))
mark = [torch.zeros(4, device=dev) for _ in range(4)]
dt = torch.bfloat16 if args.precision == "bf16" else None
wall = []
for _ in range(args.steps):
    t0 = time.perf_counter()
    loss = pkg.spade.refine_step(G, opt, *inputs, autocast_dtype=dt)
    pkg.ops.adam_step(*mark, lr=1e-3)
    torch.cuda.synchronize()
    wall.append((time.perf_counter() - t0) * 1e3)
print("wall ms per step: " + " ".join("%.1f" % t for t in wall))
windows = []
for _ in range(args.rounds):
    t0 = time.perf_counter()
    for _ in range(10):
        loss = pkg.spade.refine_step(G, opt, *inputs, autocast_dtype=dt)
    torch.cuda.synchronize()
    windows.append((time.perf_counter() - t0) * 100)
if windows:
    print("ms per step over windows of ten: " + " ".join("%.2f" % t for t in windows))
if args.host_profile:
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]) as prof:
        for _ in range(args.host_profile):
            pkg.spade.refine_step(G, opt, *inputs, autocast_dtype=dt)
        torch.cuda.synchronize()
    print("%d steps under torch.profiler, operators by their own host time:" % args.host_profile)
    print(prof.key_averages().table(sort_by="self_cpu_time_total", row_limit=14, max_name_column_width=60))
print("%s, power iteration %s, spectral norm %s, %d steps, last loss %.6f" % (args.precision, args.power_iteration, args.spectral_norm, args.steps, float(loss)))
