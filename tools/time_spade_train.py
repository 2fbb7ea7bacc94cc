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

  python tools/time_spade_train.py --autocast bf16 [--size 512] [...] [--out profiles/spade_bf16_step.json]

The refiner under ``torch.autocast("cuda", dtype=torch.bfloat16)`` (profiles/spade_bf16_step.json).  Three variants, alternated round by
round in one process: fp32 with the fused op; autocast with the fused bf16 op (``refine_step(..., autocast_dtype=torch.bfloat16)``);
autocast with the op swapped for the six torch ops.  For each: the training step and its peak memory as above, ``Generator`` inference
(eval() under no_grad) in ms per image, and the op alone on (1, 64, size / 2, size / 2), forward and backward, by HIP events -- fp32 and
bf16 through the C ABI (20 / 44 and 10 / 22 B per element), and the six ops on bf16 tensors for scale.  The file records whether autocast
with the fused op is not slower than autocast with the swapped op, and the bf16 op not slower than the fp32 op, each beyond the run's
own min-max spread; nothing is tuned to make them hold.

  python tools/time_spade_train.py --spectral-norm [--size 512] [...] [--out profiles/spade_sn_step.json]

What the fused spectral norm buys (``spade.fuse_spectral_norm_``; profiles/spade_sn_step.json).  Four variants of the ``Generator`` step,
alternated round by round in one process: (a) fp32 with torch's hooks, (b) fp32 fused, (c) autocast bf16 with torch's hooks and
``SpectralNorm.compute_weight`` run outside autocast -- an experiment defined here, the baseline for what the KERNEL buys, since a
one-line autocast guard gives that much -- and (d) autocast bf16 fused; one round of today's autocast step with plain hooks, for the
record.  And the op alone: the 18 matrices of ``Generator`` in one forward and one backward call through the C ABI on preallocated
buffers, by HIP events, against ``SpectralNorm.compute_weight`` in fp32 plus its autograd backward over the same 18 weights.  The file
records whether (d) is faster than (a), (d) and (b) not slower than (c) and (a), and the op faster than torch's chain, each beyond the
run's own min-max spread; nothing is tuned to make them hold.
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


def steps_ms(G, opt, inputs, steps, **kw):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = spade.refine_step(G, opt, *inputs, **kw)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, float(loss)


def step_peak_bytes(G, opt, inputs, **kw):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    spade.refine_step(G, opt, *inputs, **kw)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def inference_ms(G, inputs, steps, autocast):
    """eval() under no_grad: ms per image, a host clock around ``steps`` forwards that end in a device synchronise."""
    G.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        for _ in range(2):
            G(*inputs)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            G(*inputs)
        torch.cuda.synchronize()
    G.train()
    return (time.perf_counter() - t0) / steps * 1e3


def not_slower(a, b):
    """a, b: the rounds' timings of two variants of one run.  a counts as slower only beyond the run's own min-max spread: when even its
    fastest round is slower than b's slowest."""
    return not min(a) > max(b)


def main_autocast(args):
    """--autocast bf16: fp32 fused, autocast with the fused bf16 op, autocast with the op swapped for the six-op formula (module
    docstring), alternated round by round in one process -> profiles/spade_bf16_step.json."""
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    torch.manual_seed(1)
    #           (the op, refine_step's autocast_dtype)
    variants = {"fp32_fused": (FUSED, None), "autocast_fused": (FUSED, torch.bfloat16), "autocast_swapped": (six_ops, torch.bfloat16)}
    first = spade.Generator().to(dev).train()
    nets = {k: (first if i == 0 else copy.deepcopy(first)) for i, k in enumerate(variants)}
    opts = {k: torch.optim.Adam(G.parameters(), lr=2e-4, betas=(0.5, 0.999)) for k, G in nets.items()}
    inputs = tuple(torch.rand(1, 3, args.size, args.size, device=dev, generator=gen) for _ in range(3))
    res = {k: {"train_ms_per_step": [], "train_peak_bytes_above_resident": [], "inference_ms_per_image": []} for k in variants}
    for k, (op, dt) in variants.items():      # warm-up: MIOpen picks its algorithms (per dtype), Adam allocates its state
        ops.spade_modulate = op
        t0 = time.perf_counter()
        res[k]["first_loss"] = steps_ms(nets[k], opts[k], inputs, args.warmup, autocast_dtype=dt)[1]
        res[k]["warmup_wall_s"] = time.perf_counter() - t0
        inference_ms(nets[k], inputs[:2], 1, dt is not None)
    for _ in range(args.rounds):
        for k, (op, dt) in variants.items():
            ops.spade_modulate = op
            res[k]["train_ms_per_step"].append(steps_ms(nets[k], opts[k], inputs, args.steps, autocast_dtype=dt)[0])
            res[k]["train_peak_bytes_above_resident"].append(step_peak_bytes(nets[k], opts[k], inputs, autocast_dtype=dt))
            res[k]["inference_ms_per_image"].append(inference_ms(nets[k], inputs[:2], args.steps, dt is not None))
    ops.spade_modulate = FUSED
    for k in variants:
        res[k]["train_ms_per_step_best"] = min(res[k]["train_ms_per_step"])
        res[k]["inference_ms_per_image_best"] = min(res[k]["inference_ms_per_image"])
    # the op alone, forward and backward, through the C ABI on preallocated buffers
    C, H = 64, args.size // 2
    L, P, st = _lib.lib(), ops._p, ops._stream()
    src = [torch.randn(1, C, H, H, device=dev, generator=gen) for _ in range(4)]
    op = {}
    calls = {}
    for tag, dtype, suffix in (("fp32", torch.float32, ""), ("bf16", torch.bfloat16, "_bf16")):
        x, gamma, beta, g = (t.to(dtype) for t in src)
        out, dx, dgamma, dbeta = (torch.empty_like(x) for _ in range(4))
        stats = torch.empty(int(L.sahs_spade_modulate_workspace_words(C)), device=dev)
        work = torch.empty(int(L.sahs_spade_modulate_backward_workspace_words(C)), device=dev)
        fwd_f, bwd_f = getattr(L, "sahs_spade_modulate" + suffix), getattr(L, "sahs_spade_modulate_backward" + suffix)
        keep = (x, gamma, beta, g, out, dx, dgamma, dbeta, stats, work)
        fwd = lambda f=fwd_f, t=keep: _lib.check(f(C, H * H, P(t[0]), P(t[1]), P(t[2]), 1e-5, 0.2, P(t[4]), P(t[8]), st), "forward")
        bwd = lambda f=bwd_f, t=keep: _lib.check(f(C, H * H, P(t[0]), P(t[1]), P(t[4]), P(t[8]), P(t[3]), 1e-5, 0.2, P(t[5]), P(t[6]), P(t[7]),
                                                   P(t[9]), st), "backward")
        fwd()
        calls[tag] = (fwd, bwd)
        op[tag] = {"forward_ms": [], "backward_ms": []}
    xb, gb, bb, gg = (t.bfloat16() for t in src)
    leaves = [t.clone().requires_grad_(True) for t in (xb, gb, bb)]
    with torch.autocast("cuda", dtype=torch.bfloat16):
        y = six_ops(*leaves, slope=0.2)

    def swapped_fwd():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            six_ops(xb, gb, bb, slope=0.2)

    calls["swapped_bf16"] = (swapped_fwd, lambda: torch.autograd.grad(y, leaves, gg.to(y.dtype), retain_graph=True))
    op["swapped_bf16"] = {"forward_ms": [], "backward_ms": []}
    for _ in range(args.rounds):
        for tag, (fwd, bwd) in calls.items():
            reps = 50 if tag == "swapped_bf16" else 200
            op[tag]["forward_ms"].append(events_ms(fwd, reps))
            op[tag]["backward_ms"].append(events_ms(bwd, reps))
    n = C * H * H
    for tag, per in (("fp32", (20, 44)), ("bf16", (10, 22))):
        op[tag].update(bytes_per_element_forward=per[0], bytes_per_element_backward=per[1],
                       forward_GB_per_s=per[0] * n / min(op[tag]["forward_ms"]) / 1e6, backward_GB_per_s=per[1] * n / min(op[tag]["backward_ms"]) / 1e6)
    op.update(shape=[1, C, H, H], timing="HIP events on the launch stream: 200 C-ABI calls (two launches each) on preallocated buffers per round; "
              "swapped_bf16 = 50 calls of the six torch ops on bf16 tensors under autocast (forward under no_grad; backward = "
              "torch.autograd.grad through their graph), allocations and launch pacing included",
              note="the tensors of one call fit the 256 MB last-level cache: the rates are not HBM rates")
    checks = {"autocast_fused_step_not_slower_than_autocast_swapped": not_slower(res["autocast_fused"]["train_ms_per_step"], res["autocast_swapped"]["train_ms_per_step"]),
              "autocast_fused_inference_not_slower_than_autocast_swapped": not_slower(res["autocast_fused"]["inference_ms_per_image"], res["autocast_swapped"]["inference_ms_per_image"]),
              "bf16_op_forward_not_slower_than_fp32": not_slower(op["bf16"]["forward_ms"], op["fp32"]["forward_ms"]),
              "bf16_op_backward_not_slower_than_fp32": not_slower(op["bf16"]["backward_ms"], op["fp32"]["backward_ms"]),
              "rule": "a is slower than b only if min(a's rounds) > max(b's rounds): beyond the run's own min-max spread"}
    result = {"command": "python tools/time_spade_train.py --autocast bf16 --size %d --steps %d --warmup %d --rounds %d" % (args.size, args.steps, args.warmup, args.rounds),
              "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
              "workload": "Generator: refine_step in train() mode (forward, clamp, MSE, backward, Adam) and eval() inference under no_grad on a %dx%d "
                          "frame; convolutions on MIOpen in every variant; parameters and Adam state fp32 in every variant" % (args.size, args.size),
              "steps_per_window": args.steps, "rounds": args.rounds, "variants": res, "op": op, "checks": checks}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


def faster(a, b):
    """a is faster than b beyond the run's own min-max spread: even its slowest round beats b's fastest."""
    return max(a) < min(b)


class hooks_outside_autocast:
    """Variant (c): while entered, torch's SpectralNorm.compute_weight runs with autocast switched off (its matrix-vector products in fp32)."""

    def __enter__(self):
        from torch.nn.utils.spectral_norm import SpectralNorm
        self.cls, self.own = SpectralNorm, SpectralNorm.compute_weight
        own = self.own

        def guarded(hook, module, do_power_iteration):
            with torch.autocast("cuda", enabled=False):
                return own(hook, module, do_power_iteration)

        SpectralNorm.compute_weight = guarded

    def __exit__(self, *exc):
        self.cls.compute_weight = self.own


def main_spectral_norm(args):
    """--spectral-norm: variants (a) .. (d) of the step and the op alone (module docstring) -> profiles/spade_sn_step.json."""
    import contextlib
    from torch.nn.utils.spectral_norm import SpectralNorm
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    torch.manual_seed(1)
    #           (fused, refine_step's autocast_dtype, the context the steps run in)
    variants = {"a_fp32_hooks": (False, None, contextlib.nullcontext), "b_fp32_fused": (True, None, contextlib.nullcontext),
                "c_autocast_hooks_outside_autocast": (False, torch.bfloat16, hooks_outside_autocast),
                "d_autocast_fused": (True, torch.bfloat16, contextlib.nullcontext)}
    first = spade.Generator().to(dev).train()
    nets = {k: copy.deepcopy(first) for k in variants}
    nets["autocast_plain_hooks"] = first
    for k, (fused, _, _) in variants.items():
        if fused:
            spade.fuse_spectral_norm_(nets[k])
    opts = {k: torch.optim.Adam(G.parameters(), lr=2e-4, betas=(0.5, 0.999)) for k, G in nets.items()}
    inputs = tuple(torch.rand(1, 3, args.size, args.size, device=dev, generator=gen) for _ in range(3))
    res = {k: {"train_ms_per_step": []} for k in variants}
    for k, (_, dt, ctx) in variants.items():      # warm-up: MIOpen picks its algorithms (per dtype), Adam allocates its state
        with ctx():
            res[k]["first_loss"] = steps_ms(nets[k], opts[k], inputs, args.warmup, autocast_dtype=dt)[1]
    for _ in range(args.rounds):
        for k, (_, dt, ctx) in variants.items():
            with ctx():
                res[k]["train_ms_per_step"].append(steps_ms(nets[k], opts[k], inputs, args.steps, autocast_dtype=dt)[0])
    for k in variants:
        res[k]["train_ms_per_step_best"] = min(res[k]["train_ms_per_step"])
    k = "autocast_plain_hooks"      # today's autocast step (the power iteration in bf16): one round, for the record
    steps_ms(nets[k], opts[k], inputs, args.warmup, autocast_dtype=torch.bfloat16)
    res[k] = {"train_ms_per_step": [steps_ms(nets[k], opts[k], inputs, args.steps, autocast_dtype=torch.bfloat16)[0]]}
    # the op alone: Generator's 18 normalised weights, one forward and one backward call through the C ABI on preallocated buffers
    import ctypes
    convs = [m for m in first.modules() if any(isinstance(h, SpectralNorm) for h in m._forward_pre_hooks.values())]
    Ws = [m.weight_orig.detach().clone() for m in convs]
    dims = [(W.shape[0], W.numel() // W.shape[0]) for W in Ws]
    us, vs = [m.weight_u.clone() for m in convs], [m.weight_v.clone() for m in convs]
    Gs = [torch.randn(W.shape, device=dev, generator=gen) for W in Ws]
    saved, dWs = [torch.empty(h + w + 1, device=dev) for h, w in dims], [torch.empty_like(W) for W in Ws]
    table = lambda ts: (ctypes.c_void_p * len(ts))(*(t.data_ptr() for t in ts))
    hs, ws = (ctypes.c_int * len(dims))(*(h for h, _ in dims)), (ctypes.c_int * len(dims))(*(w for _, w in dims))
    L, st, n = _lib.lib(), ops._stream(), len(Ws)
    op, calls = {}, {}
    for tag, dtype in (("fused_fp32", torch.float32), ("fused_bf16", torch.bfloat16)):
        outs, grads = [torch.empty(W.shape, dtype=dtype, device=dev) for W in Ws], [g.to(dtype) for g in Gs]
        t = (table(Ws), table(us), table(vs), table(outs), table(saved), table(grads), table(dWs), outs, grads)
        fwd = lambda t=t, b=int(dtype == torch.bfloat16): _lib.check(L.sahs_spectral_norm_forward(n, t[0], t[1], t[2], t[3], t[4], hs, ws, b, 1, 1e-12, st), "forward")
        bwd = lambda t=t, b=int(dtype == torch.bfloat16): _lib.check(L.sahs_spectral_norm_backward(n, t[0], t[4], t[5], t[6], hs, ws, b, st), "backward")
        fwd()
        calls[tag] = (fwd, bwd)
    holders = []
    for W, u, v in zip(Ws, us, vs):
        holder = torch.nn.Module()
        holder.weight_orig = torch.nn.Parameter(W.clone())
        holder.register_buffer("weight_u", u.clone())
        holder.register_buffer("weight_v", v.clone())
        holders.append(holder)
    sn = SpectralNorm("weight", 1, 0, 1e-12)
    torch_fwd = lambda: [sn.compute_weight(m, True) for m in holders]
    graph = torch_fwd()
    calls["torch_fp32"] = (torch_fwd, lambda: torch.autograd.grad(graph, [m.weight_orig for m in holders], Gs, retain_graph=True))
    for tag in calls:
        op[tag] = {"forward_ms": [], "backward_ms": []}
    for _ in range(args.rounds):
        for tag, (fwd, bwd) in calls.items():
            reps = 50 if tag == "torch_fp32" else 200
            op[tag]["forward_ms"].append(events_ms(fwd, reps))
            op[tag]["backward_ms"].append(events_ms(bwd, reps))
    op.update(shapes=[list(d) for d in dims], weights=sum(h * w for h, w in dims),
              timing="HIP events on the launch stream: 200 C-ABI calls per round (forward: two launches; backward: one) over the 18 weights on "
                     "preallocated buffers, power_iteration = 1; torch_fp32 = 50 calls of SpectralNorm.compute_weight over 18 holder modules "
                     "(forward, building the graph as a training step does) and of torch.autograd.grad through it (backward), allocations "
                     "and launch pacing included")
    a, b, c, d = (res[k]["train_ms_per_step"] for k in variants)
    checks = {"d_faster_than_a": faster(d, a), "d_not_slower_than_c": not_slower(d, c), "b_not_slower_than_a": not_slower(b, a),
              "op_forward_faster_than_torch": faster(op["fused_fp32"]["forward_ms"], op["torch_fp32"]["forward_ms"]),
              "op_backward_faster_than_torch": faster(op["fused_fp32"]["backward_ms"], op["torch_fp32"]["backward_ms"]),
              "rule": "a is slower than b only if min(a's rounds) > max(b's rounds), faster only if max(a's rounds) < min(b's rounds): "
                      "beyond the run's own min-max spread"}
    reported = {"d_vs_autocast_plain_hooks_speedup": res["autocast_plain_hooks"]["train_ms_per_step"][0] / min(d),
                "c_minus_d_ms_best": min(c) - min(d), "c_minus_d_ms_range": [min(c) - max(d), max(c) - min(d)],
                "a_minus_b_ms_best": min(a) - min(b)}
    result = {"command": "python tools/time_spade_train.py --spectral-norm --size %d --steps %d --warmup %d --rounds %d" % (args.size, args.steps, args.warmup, args.rounds),
              "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
              "workload": "Generator: refine_step in train() mode (forward, clamp, MSE, backward, Adam) on a %dx%d frame; convolutions on MIOpen and "
                          "the fused SPADE modulation in every variant; parameters and Adam state fp32 in every variant" % (args.size, args.size),
              "steps_per_window": args.steps, "rounds": args.rounds, "variants": res, "op": op, "checks": checks, "reported": reported}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


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
    ap.add_argument("--autocast", choices=("bf16",), default=None)
    ap.add_argument("--spectral-norm", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.out is None:
        name = "spade_sn_step.json" if args.spectral_norm else "spade_bf16_step.json" if args.autocast else "spade_train_step.json"
        args.out = os.path.join(REPO, "profiles", name)
    if not torch.cuda.is_available():
        raise SystemExit("time_spade_train.py needs a GPU: nothing here can be measured on a CPU")
    if args.spectral_norm:
        return main_spectral_norm(args)
    if args.autocast:
        return main_autocast(args)
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
