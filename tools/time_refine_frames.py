"""Stage-II inference on one GPU: the generator per frame against its frozen form (profiles/refine_frames.json).

  python tools/time_refine_frames.py [--size 512] [--rounds 5] [--frames 16] [--out profiles/refine_frames.json]
  python tools/time_refine_frames.py --trace generator:fp32:1 [--frames 20]      # one frozen leg alone, for a kernel trace of its own

One process, seeded weights (torch.manual_seed(0)), size x size frames.  For both generators, in fp32 and in bf16, five legs alternated
round by round:
  * unfrozen:   G.eval() under no_grad, frame by frame (bf16: under torch.autocast) -- the path this repository had before the frozen one;
  * frozen_B1, frozen_B8:                   spade.freeze_identity(G, I_src, dtype=...) on 1 and on 8 frames per call;
  * frozen_B1_nofold, frozen_B8_nofold:     the same snapshot with fold_upsample=False (F.interpolate written out before the "up" layers).
Each figure is milliseconds PER FRAME from HIP events around ``frames`` frames of synchronised work (warmed up first: the library picks
its convolution algorithms on first sight of a shape).  Per leg: the rounds, min / median / max.
Also recorded: device launches per frame (torch.profiler, in a call outside the timed windows), cached_bytes of the snapshot, the
largest difference between the frozen and the unfrozen output on one frame, and the modulation alone -- the 18 layers' frozen ops
(statistics + modulate launches) on the snapshot's own maps at B = 1 and B = 8, folded and not, with the bytes they must move computed
from the shapes and the GB/s that makes; the per-frame op on the same maps beside it.  A frame's planes and maps are larger than the
256 MB last-level cache only in sum: the rates are whole-op rates, named for what they are.
There is no CPU path: without a GPU this fails.
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
pkg = importlib.import_module("sahs-deformable-nerf_amd")
ops, S = pkg.ops, pkg.spade
GENERATORS = {"generator": "Generator", "generator_audio": "Generator_audio"}
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def events_ms(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def count_launches(fn):
    """Device kernels of one call, by torch.profiler -> int, or a string saying why it could not be counted."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower())
        return n if n > 0 else "not counted: the profiler recorded no device events"
    except Exception as exc:      # noqa: BLE001  (a profiler that cannot start must not lose the timings)
        return "not counted: %s" % exc


def summary(ms):
    return {"rounds_ms_per_frame": ms, "median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def build(name, dtype, size, dev):
    """-> (legs: name -> (closure of one call, frames per call), the snapshot)."""
    torch.manual_seed(0)
    G = getattr(S, GENERATORS[name])().eval().to(dev)
    gen = torch.Generator().manual_seed(1)
    i_src = torch.rand(1, 3, size, size, generator=gen).to(dev)
    frames = torch.rand(8, 3, size, size, generator=gen).to(dev)
    windows = torch.randn(8, 16, 29, generator=gen).to(dev) if name == "generator_audio" else None
    frozen = S.freeze_identity(G, i_src, dtype=DTYPES[dtype], fold_upsample=True)
    nofold = S.FrozenRefiner(frozen.size, frozen.dtype, False, frozen.stem, frozen.blocks, frozen.layer8, frozen.audio)      # the same tensors

    def unfrozen():
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == "bf16"):
            return G(i_src, frames[:1]) if windows is None else G(i_src, frames[:1], windows[0])

    call = lambda fr, B: (lambda: fr(frames[:B]) if windows is None else fr(frames[:B], windows[:B]))      # noqa: E731
    legs = {"unfrozen": (unfrozen, 1), "frozen_B1": (call(frozen, 1), 1), "frozen_B8": (call(frozen, 8), 8),
            "frozen_B1_nofold": (call(nofold, 1), 1), "frozen_B8_nofold": (call(nofold, 8), 8)}
    return legs, frozen


def modulate_legs(frozen, dev):
    """The 18 layers' modulation alone on the snapshot's maps (layers whose maps are cached; an audio snapshot has 12)
    -> legs: name -> (closure, bytes the ops must move per call), elements per frame."""
    el = frozen.stem[0].element_size()
    layers = []      # (gamma, beta, is the second layer of an "up" block)
    for blk in frozen.blocks:
        for key in ("spade1", "spade2", "spade_s"):
            if blk[key][0] == "maps":
                layers.append(blk[key][1] + (key == "spade2" and blk["how"] == "up",))
    gen = torch.Generator().manual_seed(2)
    xs = {}
    for B in (1, 8):
        xs[B, False] = [torch.randn((B,) + tuple(g.shape[1:]), generator=gen).to(dev, frozen.dtype) for g, _, _ in layers]
        xs[B, True] = [torch.randn(B, g.shape[1], g.shape[2] // 2, g.shape[3] // 2, generator=gen).to(dev, frozen.dtype) if up else x
                       for (g, _, up), x in zip(layers, xs[B, False])]
    elements = sum(g.numel() for g, _, _ in layers)
    legs = {}
    for B in (1, 8):
        for fold in (True, False):
            def run(B=B, fold=fold):
                for (g, b, up), x in zip(layers, xs[B, fold]):
                    ops.spade_modulate_frozen(x, g, b, eps=1e-5, slope=0.2, up=up and fold)
            # per output element: x is read by the statistics pass and by the modulate pass (a quarter of it each when folded), gamma and
            # beta once per batch, out written once
            nbytes = sum(g.numel() * el * (B * (2 * (0.25 if up and fold else 1.0) + 1.0) + 2.0) for g, _, up in layers)
            legs["frozen_op_B%d%s" % (B, "" if fold else "_nofold")] = (run, nbytes, B)

    def per_frame():
        for (g, b, _), x in zip(layers, xs[1, False]):
            ops.spade_modulate(x, g, b, eps=1e-5, slope=0.2)
    legs["per_frame_op_B1"] = (per_frame, sum(g.numel() * el * 5.0 for g, _, _ in layers), 1)
    return legs, elements


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=16, help="frames per timed window (a multiple of 8)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "refine_frames.json"))
    ap.add_argument("--trace", default=None, help="generator:dtype:B -- run that frozen leg alone and exit (for a profiler)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_refine_frames.py needs a GPU: nothing here can be measured on a CPU")
    if args.rounds < 5 or args.frames % 8:
        raise SystemExit("at least 5 rounds, and a multiple of 8 frames per window")
    dev = torch.device("cuda:0")
    if args.trace:
        name, dtype, B = args.trace.split(":")
        fn, per = build(name, dtype, args.size, dev)[0]["frozen_B%d" % int(B)]
        for _ in range(3 + args.frames // per):
            fn()
        torch.cuda.synchronize()
        return
    results = {}
    for name in GENERATORS:
        for dtype in DTYPES:
            legs, frozen = build(name, dtype, args.size, dev)
            with torch.no_grad():
                y0, y1 = legs["unfrozen"][0]().float(), legs["frozen_B1"][0]()
            rec = {"cached_bytes": frozen.cached_bytes, "cached_map_bytes": frozen.cached_map_bytes,
                   "frozen_vs_unfrozen_max_abs_difference": float((y0 - y1).abs().max()), "output_max_abs": float(y0.abs().max()),
                   "launches_per_frame": {}}
            for leg, (fn, per) in legs.items():
                for _ in range(3):
                    fn()
                n = count_launches(fn)
                rec["launches_per_frame"][leg] = n / per if isinstance(n, int) else n
            times = {leg: [] for leg in legs}
            for r in range(args.rounds):
                for leg, (fn, per) in legs.items():
                    times[leg].append(events_ms(fn, args.frames // per) / args.frames)
                print("%s %s round %d: %s" % (name, dtype, r, {k: round(v[-1], 3) for k, v in times.items()}), flush=True)
            rec["legs"] = {leg: summary(ms) for leg, ms in times.items()}
            L = rec["legs"]
            apart = lambda a, b: L[a]["max"] < L[b]["min"] or L[b]["max"] < L[a]["min"]      # noqa: E731
            rec["frozen_B1_faster_than_unfrozen_beyond_spread"] = L["frozen_B1"]["max"] < L["unfrozen"]["min"]
            rec["share_of_unfrozen_frame_time_gone_B1"] = 1.0 - L["frozen_B1"]["median"] / L["unfrozen"]["median"]
            rec["share_of_unfrozen_frame_time_gone_B8"] = 1.0 - L["frozen_B8"]["median"] / L["unfrozen"]["median"]
            rec["fold_upsample_series_apart"] = {"B1": apart("frozen_B1", "frozen_B1_nofold"), "B8": apart("frozen_B8", "frozen_B8_nofold")}
            mlegs, elements = modulate_legs(frozen, dev)
            mt = {leg: [] for leg in mlegs}
            for leg, (fn, _, _) in mlegs.items():
                for _ in range(3):
                    fn()
            for r in range(args.rounds):
                for leg, (fn, _, B) in mlegs.items():
                    mt[leg].append(events_ms(fn, 8 // B) / 8)
            rec["modulation_alone"] = {"gamma_elements": elements, "legs": {}}
            for leg, (_, nbytes, B) in mlegs.items():
                s = summary(mt[leg])
                s["bytes_per_frame_from_shapes"] = nbytes / B
                s["achieved_GB_per_s_at_median"] = nbytes / B / (s["median"] * 1e-3) / 1e9
                rec["modulation_alone"]["legs"][leg] = s
            print("%s %s modulation alone: %s" % (name, dtype, {k: (round(v["median"], 3), round(v["achieved_GB_per_s_at_median"])) for k, v in
                                                              rec["modulation_alone"]["legs"].items()}), flush=True)
            results["%s_%s" % (name, dtype)] = rec
            del legs, frozen, mlegs
            torch.cuda.empty_cache()
    out = {"command": "python tools/time_refine_frames.py --size %d --rounds %d --frames %d" % (args.size, args.rounds, args.frames),
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "workload": "Stage-II inference of %dx%d frames, seeded weights: the generator per frame (unfrozen) against "
                       "spade.freeze_identity's snapshot at 1 and 8 frames per call, with and without fold_upsample" % (args.size, args.size),
           "timing": "ms per frame; HIP events around %d frames of synchronised work per leg and round, %d rounds, the legs alternated, every "
                     "shape warmed up first; launches by torch.profiler outside the timed windows; modulation_alone: the snapshot's cached "
                     "layers' statistics + modulate launches on its own maps, bytes from shapes" % (args.frames, args.rounds),
           "rules": "frozen_B1_faster_than_unfrozen_beyond_spread: max(frozen_B1 rounds) < min(unfrozen rounds); fold_upsample_series_apart: "
                    "the two series' [min, max] intervals do not overlap", "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
