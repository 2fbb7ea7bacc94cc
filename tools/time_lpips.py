"""LPIPS on one GPU: the fused scaling layer and head against the same steps written in torch (profiles/lpips.json).

  python tools/time_lpips.py [--size 512] [--rounds 3] [--reps 100] [--out profiles/lpips.json]

Shapes: size x size x 3 pairs at B = 1 and B = 8, uint8 and fp32, synthetic weights (metrics.LPIPS.from_seed: the time does not depend
on the weights' values).  Per shape, two variants alternated round by round in one process, HIP events around ``reps`` calls on
preallocated inputs after a warm-up that absorbs the convolution library's search:
  (a) ends alone   fused: ops.lpips_prepare (one launch) + ops.lpips_distance on the five feature tensors (two launches);
                   torch: tests/lpips_reference.py's torch_scaling + torch_head on the SAME five feature tensors.
                   The convolutions are outside both.
  (b) whole call   fused: metrics.LPIPS.layers; torch: torch_scaling, the same convolutions, torch_head.
  (c) what the convolutions' deterministic mode costs (metrics.LPIPS.features sets it): the fused whole call against the same steps
      with the library left to pick any kernel.
Launches per call are counted with torch.profiler outside the timed windows.  The file records the minimum and maximum over the rounds
and whether the fused variant is faster beyond the rounds' own spread (max of its rounds < min of torch's); nothing is tuned to make
that hold, and where the convolutions dominate the whole call it says so by the numbers.  There is no CPU path: without a GPU this fails.
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
import lpips_reference as R      # noqa: E402  (the torch formulation the GPU tests measure E_torch with)
from time_metrics import count_launches, events_ms      # noqa: E402

pkg = importlib.import_module("sahs-deformable-nerf_amd")
ops, metrics = pkg.ops, pkg.metrics


def rounds_of(fused, other, rounds, reps, name="torch"):
    """The two callables alternated round by round -> their times per round, min, max, and whether ``fused`` wins beyond the spread."""
    f, o = [], []
    for _ in range(rounds):
        f.append(events_ms(fused, reps))
        o.append(events_ms(other, reps))
    return {"fused_ms": f, name + "_ms": o, "fused_ms_min": min(f), "fused_ms_max": max(f), name + "_ms_min": min(o), name + "_ms_max": max(o),
            "speedup_of_minima": min(o) / min(f), "fused_faster_beyond_spread": max(f) < min(o)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "lpips.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_lpips.py needs a GPU: nothing here can be measured on a CPU")
    dev = torch.device("cuda:0")
    S = args.size
    model = metrics.LPIPS.from_seed(0)
    convs, lins = model.device_weights(dev)
    shapes = {}
    for dtype in (np.uint8, np.float32):
        for B in (1, 8):
            pairs = [R.noisy_pair(S, S, dtype, 20 + i) for i in range(B)]
            a, b = (torch.from_numpy(np.stack(x)).to(dev) for x in zip(*pairs))
            with torch.no_grad():
                feats = metrics.alexnet_features(ops.lpips_prepare(a, b), convs)

                def ends_fused():
                    ops.lpips_prepare(a, b)
                    return ops.lpips_distance(feats, lins)

                def ends_torch():
                    R.torch_scaling(a, b, False)
                    return R.torch_head(feats, lins)

                def whole_fused():
                    return model.layers(a, b)

                def whole_torch():
                    return R.torch_head(model.features(R.torch_scaling(a, b, False)), lins)

                def whole_fused_default_convolutions():      # the same steps with the library left to pick any kernel
                    return ops.lpips_distance(metrics.alexnet_features(ops.lpips_prepare(a, b), convs), lins)

                for fn in (whole_fused, whole_torch, whole_fused_default_convolutions):      # the convolution search, outside every timed window
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                agree = float((whole_fused() - whole_torch().double()).abs().max())
                rec = {"lpips_of_the_pairs": [float(v) for v in whole_fused()[:, 0]], "max_abs_difference_fused_vs_torch": agree,
                       "feature_bytes_read_by_the_head": sum(f.numel() * 4 for f in feats),
                       "launches": {"ends_fused": count_launches(ends_fused), "ends_torch": count_launches(ends_torch),
                                    "whole_fused": count_launches(whole_fused), "whole_torch": count_launches(whole_torch)},
                       "ends_alone": rounds_of(ends_fused, ends_torch, args.rounds, args.reps),
                       "whole_call": rounds_of(whole_fused, whole_torch, args.rounds, max(args.reps // 2, 1)),
                       "deterministic_mode": rounds_of(whole_fused, whole_fused_default_convolutions, args.rounds, max(args.reps // 2, 1),
                                                       "default_convolutions")}
                rec["launches"]["whole_fused_default_convolutions"] = count_launches(whole_fused_default_convolutions)
            shapes["%s_B%d" % (np.dtype(dtype).name, B)] = rec
    result = {"command": "python tools/time_lpips.py --size %d --rounds %d --reps %d" % (S, args.rounds, args.reps),
              "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
              "workload": "LPIPS (alex, v0.1) of %dx%dx3 image pairs on synthetic weights; ends_alone = scaling layer + head on fixed feature "
                          "tensors (fused: 3 launches; torch: tests/lpips_reference.py torch_scaling + torch_head), whole_call = with the five "
                          "convolutions, which both variants run through torch.nn.functional in fp32 in the library's deterministic mode; "
                          "deterministic_mode = the fused whole call against itself with the mode off" % (S, S),
              "timing": "HIP events on the launch stream around %d calls per round (whole call: %d), the two variants alternated, %d rounds, "
                        "after a warm-up that absorbs the convolution search; includes the Python and allocator cost of each call"
                        % (args.reps, max(args.reps // 2, 1), args.rounds),
              "rule": "fused_faster_beyond_spread: max(fused rounds) < min(torch rounds)", "shapes": shapes}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
