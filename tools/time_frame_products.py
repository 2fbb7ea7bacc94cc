"""Frame products on one GPU: the fused op against evaluation.py's torch functions on the same frames (profiles/frame_products.json).

  python tools/time_frame_products.py [--size 512] [--rounds 5] [--reps 200] [--out profiles/frame_products.json]

Frames: size x size, the renderer's (H, W, 15) output, its disparity and background weight, at B = 1 and B = 8.  Per shape two variants,
alternated round by round in one process, on preallocated inputs:
  * fused: sahs_frame_products through the C ABI on preallocated outputs and workspace -- image, mask, normal (u8 and fp32, as
    render_frames(fused_products=True) asks for them) and disparity planes of all B frames in two launches;
  * torch: per frame, normal_map, label2color and the device part of cast_to_image (twice), of the normal PNG's cast and of
    cast_to_disparity_image -- the expressions of evaluation.py up to where they leave the device.  Its allocations go through torch's
    caching allocator (warm after the first call); its launches are counted with torch.profiler in a call outside the timed windows.
Two timings each: ``device`` -- HIP events around ``reps`` calls, no host copy; ``with_copies`` -- a host clock around calls that end as
evaluation.render_frames ends them, every written plane on the host (fused: four uint8 copies per frame; torch: cast_to_image and the
normal cast copy uint8, cast_to_disparity_image copies its fp32 plane), each call synchronous through its copies.
Reported per variant: the rounds, their median and their min-max spread; no pass mark -- the ratio is what it is.  Also recorded: the
normal map's deviation from the float64 statement (tests/frame_products_reference.py) next to e, the torch functions' own fp32 error on
the CPU, for square maps up to this size.  There is no CPU path: without a GPU this fails.
"""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import frame_products_reference as R      # noqa: E402  (the float64 statement and the inputs the GPU tests use)

pkg = importlib.import_module("sahs-deformable-nerf_amd")
ops, _lib, E = pkg.ops, pkg._lib, pkg.evaluation


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


def host_ms(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


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


def fused_call(rgb, disp, w_bg, focal):
    """rgb (B, H, W, 15), disp, w_bg (B, H, W) -> (closure of one C-ABI call on preallocated buffers, dict of its output tensors)."""
    L, P, st = _lib.lib(), ops._p, ops._stream()
    B, H, W, C = rgb.shape
    dev = rgb.device
    out = dict(image=torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev), seg=torch.empty(B, H, W, 3, dtype=torch.uint8, device=dev),
               normals=torch.empty(B, H - 1, W - 1, 3, dtype=torch.uint8, device=dev), normals_f32=torch.empty(B, H - 1, W - 1, 3, device=dev),
               disparity=torch.empty(B, H, W, dtype=torch.uint8, device=dev))
    need = int(L.sahs_frame_products_workspace_bytes(B, H, W))
    work = torch.empty(need // 4, device=dev)
    strides, intr = (ctypes.c_long * 3)(*rgb.stride()[:3]), (ctypes.c_float * 4)(*[float(v) for v in focal])
    return (lambda: _lib.check(L.sahs_frame_products(P(rgb), C, strides, P(disp), P(w_bg), intr, B, H, W, 1, 0, P(out["image"]), P(out["seg"]),
                                                     P(out["normals"]), P(out["normals_f32"]), P(out["disparity"]), P(work), need, st),
                               "sahs_frame_products")), out


def torch_device_call(rgb, disp, w_bg, focal):
    """evaluation.py's expressions per frame, up to where they leave the device."""
    def one(f, d, w):
        n = E.normal_map(d, focal, w, clean=True)
        return ((f[..., :3].clamp(0.0, 1.0) * 255).to(torch.uint8), (E.label2color(f[..., 3:]).clamp(0.0, 1.0) * 255).to(torch.uint8),
                n.clamp(0, 255).to(torch.uint8), ((d - d.min()) / (d.max() - d.min())).clamp(0, 1) * 255)
    return lambda: [one(rgb[b], disp[b], w_bg[b]) for b in range(rgb.shape[0])]


def torch_copies_call(rgb, disp, w_bg, focal):
    """What render_frames(fused_products=False) does per written frame, host arrays included."""
    def one(f, d, w):
        n = E.normal_map(d, focal, w, clean=True)
        return (E.cast_to_image(f[..., :3]), E.cast_to_image(E.label2color(f[..., 3:])), n.clamp(0, 255).to(torch.uint8).cpu().numpy(),
                E.cast_to_disparity_image(d))
    return lambda: [one(rgb[b], disp[b], w_bg[b]) for b in range(rgb.shape[0])]


def summary(ms):
    return {"rounds_ms": ms, "median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def deviations(sizes, dev):
    """Square maps: e = max |evaluation.normal_map in fp32 on the CPU - float64 statement| and the op's own deviation, non-white entries."""
    rows = {}
    for S in sizes:
        disp, w_bg, focal = R.make_disp(S, S, 3), R.make_w_bg(S, S, 3), R.focal_for(S, S)
        r64, white = R.normals(disp, focal, w_bg), R.white_mask(w_bg)
        rest = np.broadcast_to(~white[..., None], r64.shape)
        t32 = E.normal_map(torch.from_numpy(disp), focal, torch.from_numpy(w_bg), clean=True).numpy()
        got = ops.frame_products(torch.zeros(S, S, 3, device=dev), torch.from_numpy(disp).to(dev), torch.from_numpy(w_bg).to(dev), focal,
                                 float_normals=True)
        f32, u8 = got["normals_f32"].cpu().numpy(), got["normals"].cpu().numpy()
        e = float(np.abs(t32 - r64)[rest].max())
        lo, hi = R.byte_bounds(r64, 4 * e)
        rows["%dx%d" % (S, S)] = {"e_torch_fp32_cpu": e, "op_deviation": float(np.abs(f32 - r64)[rest].max()),
                                  "bytes_outside_4e_interval": int(((u8 < lo) | (u8 > hi)).sum()), "two_byte_share": float((hi > lo)[rest].mean()),
                                  "white_bytes_not_255": int((u8[white] != 255).sum())}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "frame_products.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_frame_products.py needs a GPU: nothing here can be measured on a CPU")
    dev = torch.device("cuda:0")
    S = args.size
    focal = R.focal_for(S, S)
    shapes = {}
    for B in (1, 8):
        rgb = torch.from_numpy(np.stack([R.make_rgb(S, S, 20 + b) for b in range(B)])).to(dev)
        disp = torch.from_numpy(np.stack([R.make_disp(S, S, 20 + b) for b in range(B)])).to(dev)
        w_bg = torch.from_numpy(np.stack([R.make_w_bg(S, S, 20 + b) for b in range(B)])).to(dev)
        fused, out = fused_call(rgb, disp, w_bg, focal)
        fused_copies = lambda: (fused(), [[out[k][b].cpu().numpy() for k in ("image", "seg", "normals", "disparity")] for b in range(B)])      # noqa: E731
        tdev, tcop = torch_device_call(rgb, disp, w_bg, focal), torch_copies_call(rgb, disp, w_bg, focal)
        fused()
        want = tdev()
        agree = {k: int((out[k][b].int() - want[b][j].int()).abs().max()) for j, k in enumerate(("image", "seg", "normals", "disparity")) for b in (B - 1,)}
        treps = max(args.reps // 4, 1)
        rec = {"fused_launches_per_call": count_launches(fused), "torch_launches_per_call": count_launches(tdev), "frames_per_call": B,
               "max_byte_difference_fused_vs_torch_gpu_last_frame": agree,
               "bytes_to_host_per_frame": {"fused": S * S * 3 + S * S * 3 + (S - 1) * (S - 1) * 3 + S * S,      # four uint8 planes
                                           "torch": S * S * 3 + S * S * 3 + (S - 1) * (S - 1) * 3 + S * S * 4}}      # the disparity leaves as fp32
        t = {"fused_device": [], "torch_device": [], "fused_with_copies": [], "torch_with_copies": []}
        for _ in range(args.rounds):
            t["fused_device"].append(events_ms(fused, args.reps))
            t["torch_device"].append(events_ms(tdev, treps))
            t["fused_with_copies"].append(host_ms(fused_copies, treps))
            t["torch_with_copies"].append(host_ms(tcop, treps))
        rec.update({k: summary(v) for k, v in t.items()})
        rec["device_ratio_torch_over_fused_medians"] = rec["torch_device"]["median_ms"] / rec["fused_device"]["median_ms"]
        rec["with_copies_ratio_torch_over_fused_medians"] = rec["torch_with_copies"]["median_ms"] / rec["fused_with_copies"]["median_ms"]
        rec["fused_faster_beyond_spread"] = {"device": rec["fused_device"]["max_ms"] < rec["torch_device"]["min_ms"],
                                             "with_copies": rec["fused_with_copies"]["max_ms"] < rec["torch_with_copies"]["min_ms"]}
        shapes["B%d" % B] = rec
    result = {"command": "python tools/time_frame_products.py --size %d --rounds %d --reps %d" % (S, args.rounds, args.reps),
              "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
              "workload": "image, mask, normal (u8 and fp32) and disparity planes of %dx%d frames from the (H, W, 15) render, its disparity and "
                          "background weight; fused = sahs_frame_products (C ABI, preallocated buffers, all B frames per call), torch = "
                          "evaluation.py's functions frame by frame" % (S, S),
              "timing": "device: HIP events on the launch stream around %d fused and %d torch calls per round; with_copies: host clock around %d "
                        "calls each that end with every written plane on the host; %d rounds, the variants alternated; the frames of one call fit "
                        "the 256 MB last-level cache: the rates are not HBM rates" % (args.reps, max(args.reps // 4, 1), max(args.reps // 4, 1), args.rounds),
              "rule": "fused_faster_beyond_spread: max(fused rounds) < min(torch rounds)", "shapes": shapes,
              "normal_map_deviation_vs_float64": deviations([s for s in (3, 24, 32, 65, 128, 256, 512) if s <= S], dev)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
