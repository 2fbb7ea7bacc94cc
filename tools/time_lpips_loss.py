"""LPIPS as a training term on one GPU: the fused ends against the same objective composed in torch (profiles/lpips_loss.json).

  python tools/time_lpips_loss.py [--size 512] [--rounds 3] [--reps 50] [--steps 10] [--out profiles/lpips_loss.json]

Variants are alternated round by round in one process; op timings are HIP events around ``reps`` calls of forward + backward on
preallocated inputs; launches are counted with torch.profiler in a call outside the timed windows; peak memory is torch's allocator
peak over one forward + backward, above what was allocated before it.
  (a) head: ops.lpips_head (two launches forward, one backward; saved: the features and 24 bytes per pixel) against
      tests/lpips_reference.py's torch_head with autograd, on synthetic features of a 512 x 512 image's map sizes -- 127^2, 63^2, 31^2,
      31^2, 31^2 pixels with C = 64, 192, 384, 256, 256 -- at B = 1 and B = 8; the gradient flows to the first operand only in both.
  (b) loss: metrics.LPIPS.loss (LPIPS.from_seed(0)) against the same steps composed in torch (clamp, scaling layer, the same
      convolutions, torch_head), size x size, B = 1 and B = 8.
  (c) step: ``spade.refine_step`` of ``Generator`` in train() mode with Adam on one size x size frame, three copies of one
      initialisation: RefineLoss(l2=1); RefineLoss(l2=1, lpips=1, lpips_model=...); and l2 plus the torch-composed LPIPS.  ms per step
      by a host clock around ``steps`` steps that end in a device synchronise.
Each comparison is recorded against the rounds' own min-max spread -- fused_faster_beyond_spread: max of the fused rounds < min of
torch's; fused_slower_beyond_spread: min of the fused rounds > max of torch's -- whichever way it comes out; nothing is tuned to make
either hold.  There is no CPU path: without a GPU this fails.
"""
import argparse
import copy
import importlib
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import lpips_grad_reference as G      # noqa: E402  (the torch composition the GPU tests use)
import lpips_reference as R      # noqa: E402

pkg = importlib.import_module("sahs-deformable-nerf_amd")
ops, spade, metrics = pkg.ops, pkg.spade, pkg.metrics
LAYERS = ((64, 127), (192, 63), (384, 31), (256, 31), (256, 31))      # (C, side) of a 512 x 512 image's five maps


def events_ms(fn, reps):
    for _ in range(3):
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


def peak_bytes(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - before)


def compare(fused, composed, rounds, reps):
    rec = {"fused_ms": [], "torch_ms": [], "fused_launches": count_launches(fused), "torch_launches": count_launches(composed),
           "fused_peak_bytes": peak_bytes(fused), "torch_peak_bytes": peak_bytes(composed)}
    for _ in range(rounds):
        rec["fused_ms"].append(events_ms(fused, reps))
        rec["torch_ms"].append(events_ms(composed, reps))
    rec.update(fused_ms_best=min(rec["fused_ms"]), torch_ms_best=min(rec["torch_ms"]), speedup_best=min(rec["torch_ms"]) / min(rec["fused_ms"]),
               fused_faster_beyond_spread=max(rec["fused_ms"]) < min(rec["torch_ms"]),
               fused_slower_beyond_spread=min(rec["fused_ms"]) > max(rec["torch_ms"]))
    return rec


def torch_head_loss(fa, fb, lins):
    """lpips_reference.torch_head on two operands -> the batch's mean LPIPS."""
    return R.torch_head([torch.cat([a, b]) for a, b in zip(fa, fb)], lins)[:, 0].mean()


def torch_lpips_loss(model, pred, target):
    convs, lins = model.device_weights(pred.device)
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        return G.chain(pred, target, convs, lins, model.normalize, True, G.naive_head, metrics.alexnet_features)[0]
    finally:
        torch.backends.cudnn.deterministic = before


def steps_ms(net, opt, inputs, steps, loss):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        value = spade.refine_step(net, opt, *inputs, loss=loss)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3, float(value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lpips_loss.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_lpips_loss.py needs a GPU: nothing here can be measured on a CPU")
    dev = torch.device("cuda:0")
    S = args.size
    model = metrics.LPIPS.from_seed(0)
    _, lins = model.device_weights(dev)
    gen = torch.Generator(device=dev).manual_seed(1)

    head, whole = {}, {}
    for B in (1, 8):
        # (a) features like ReLU outputs lifted by 1e-3: no all-zero pixel, at which torch_head's gradient would be NaN
        fa = [torch.randn(B, C, s, s, device=dev, generator=gen).clamp_(min=0).add_(1e-3).requires_grad_(True) for C, s in LAYERS]
        fb = [(f.detach() * 1.01 + 0.05 * torch.rand(f.shape, device=dev, generator=gen)) for f in fa]

        def head_call(fn, fa=fa, fb=fb):
            def call():
                for f in fa:
                    f.grad = None
                fn(fa, fb).backward()
            return call

        rec = compare(head_call(lambda a, b: ops.lpips_head(a, b, lins)[0].mean()), head_call(lambda a, b: torch_head_loss(a, b, lins)),
                      args.rounds, args.reps)
        rec["feature_bytes_per_operand"] = sum(f.numel() * 4 for f in fa)
        rec["statistics_bytes"] = 24 * B * sum(s * s for _, s in LAYERS)
        head["B%d" % B] = rec

        # (b) the whole term
        pred = torch.rand(B, 3, S, S, device=dev, generator=gen).mul_(1.2).sub_(0.1).requires_grad_(True)
        target = torch.rand(B, 3, S, S, device=dev, generator=gen)

        def loss_call(fn, pred=pred, target=target):
            def call():
                pred.grad = None
                fn(pred, target).backward()
            return call

        whole["B%d" % B] = compare(loss_call(model.loss), loss_call(lambda p, t: torch_lpips_loss(model, p, t)), args.rounds,
                                   max(args.reps // 2, 1))

    # (c) one refiner step: three copies of one initialisation, alternated
    torch.manual_seed(1)
    first = spade.Generator().to(dev).train()
    variants = {"refine_loss_l2": spade.RefineLoss(l2=1.0), "refine_loss_l2_lpips": spade.RefineLoss(l2=1.0, lpips=1.0, lpips_model=model),
                "l2_plus_torch_lpips": lambda fake, t: spade.RefineLoss(l2=1.0)(fake, t) + torch_lpips_loss(model, fake.float(), t)}
    nets = {k: copy.deepcopy(first) for k in variants}
    opts = {k: torch.optim.Adam(nets[k].parameters(), lr=2e-4, betas=(0.5, 0.999)) for k in variants}
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
    f, t = step["refine_loss_l2_lpips"]["ms_per_step"], step["l2_plus_torch_lpips"]["ms_per_step"]
    step["fused_faster_than_torch_lpips_beyond_spread"] = max(f) < min(t)
    step["fused_slower_than_torch_lpips_beyond_spread"] = min(f) > max(t)
    step["lpips_term_ms_best"] = min(f) - step["refine_loss_l2"]["ms_best"]

    result = {"command": "python tools/time_lpips_loss.py --size %d --rounds %d --reps %d --steps %d" % (S, args.rounds, args.reps, args.steps),
              "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
              "workload": "head: synthetic fp32 features of a 512x512 image's five AlexNet maps, forward + backward to the first operand; loss: "
                          "LPIPS.from_seed(0).loss on %dx%d (B, 3, H, W) fp32 against clamp, scaling layer, the same convolutions and torch_head in "
                          "torch; refine_step: Generator.train() with Adam on one %dx%d frame" % (S, S, S, S),
              "timing": "op: HIP events on the launch stream around %d (head) and %d (loss) forward + backward calls per round, alternated, %d "
                        "rounds; step: a host clock around %d steps ending in a device synchronise, the variants alternated, %d rounds"
                        % (args.reps, max(args.reps // 2, 1), args.rounds, args.steps, args.rounds),
              "rule": "fused_faster_beyond_spread: max(fused rounds) < min(torch rounds); fused_slower_beyond_spread: min(fused rounds) > "
                      "max(torch rounds)",
              "head_forward_backward": head, "loss_forward_backward": whole, "refine_step": step}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        json.dump(result, fo, indent=1)
        fo.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
