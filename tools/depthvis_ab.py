#!/usr/bin/env python
"""Coloured depth frames: the device route against the reference's host route, on the same device images.

Workload: one timestamp of three cameras at 1066 x 1600 -- three fp32 depth images and three fp32 opacity images on the device in,
one uint8 [1066, 4800, 3] strip on the host out -- once with the fixed bounds of the reference's depth_visualizer (lo = 4, hi = 120)
and once with the automatic ones (lo = hi = None: the opacity-weighted 0.5 / 99.5 percentiles of each frame).

  device     three depthvis.depth_colors calls into a device strip, then the strip copied into pinned host memory with a non_blocking
             copy -- what pipeline.evaluate_video(depth_keys=("depth_colors",), host=True) enqueues per timestamp.  Device time between
             two events around all of it; the kernels alone between two events of their own.
  host       the reference's own arithmetic (utils/visualization_tools.py:106-194, restated here in numpy: fp32 log curve, argsort +
             fp32 cumsum + np.interp for the automatic bounds, matplotlib's turbo colormap call, to8b) on `.cpu().numpy()` copies of
             the same device images, concatenated.  Host work with blocking copies: wall clock.

    python tools/depthvis_ab.py [--reps 20] [--warmup 3] [--out profiles/depthvis_ab.txt] [--trace-only N]

The two routes alternate in one process; medians over the repetitions.  The strips are compared: the share of pixels whose bytes differ
and the largest distance in table steps (the host route takes its log and its prefix sums in fp32, so a few pixels sit one step
apart; tests/golden/depthvis.npz records the same for the reference's own code).  There is no speed gate.
--trace-only N: N device-route timestamps of each kind and nothing else, for a `rocprofv3 --kernel-trace --stats` run of its own
(tools/kstats.py prints its kernels: profiles/depthvis_kstats.txt)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H, W, N_CAMS = 1066, 1600, 3
KINDS = {"fixed": (4.0, 120.0), "automatic": (None, None)}


def street(seed):
    """Street-like frame: depth falling with the image row, opacity rising from about 0.2 to 1 (the shape of tests/depthvis_ref.py)."""
    g = torch.Generator().manual_seed(seed)
    row = torch.linspace(0.0, 1.0, H)[:, None]
    depth = (3.0 + 150.0 * (1.0 - row) ** 2) * torch.exp(0.15 * torch.randn(H, W, generator=g))
    alpha = (0.2 + 0.9 * row + 0.05 * torch.randn(H, W, generator=g)).clamp(0.0, 1.0)
    return depth.float()[None], alpha.float()[None]


def host_weighted_percentile(x, w, ps):
    x, w = x.reshape([-1]), w.reshape([-1])
    order = np.argsort(x)
    x, w = x[order], w[order]
    acc = np.cumsum(w)
    return np.interp(np.array(ps) * (acc[-1] / 100), acc, x)


def host_frame(depth, alpha, lo, hi, cmap):
    """visualize_depth(depth, alpha, lo, hi, depth_curve_fn=-log(x + 1e-6)) with matte_background=False, then to8b."""
    curve = lambda v: -np.log(v + 1e-6)
    if lo is None or hi is None:
        lo_auto, hi_auto = host_weighted_percentile(depth, alpha, [0.5, 99.5])
        eps = np.finfo(np.float32).eps
        lo = lo or (lo_auto - eps)
        hi = hi or (hi_auto + eps)
    value, lo, hi = curve(depth), curve(lo), curve(hi)
    value = np.nan_to_num(np.clip((value - np.minimum(lo, hi)) / np.abs(hi - lo), 0, 1))
    value *= alpha
    return (255 * np.clip(cmap(value)[..., :3], 0, 1)).astype(np.uint8)


def host_route(planes, lo, hi, cmap):
    return np.concatenate([host_frame(d[0].cpu().numpy(), a[0].cpu().numpy(), lo, hi, cmap) for d, a in planes], axis=1)


def table_steps(a, b, table):
    code = np.full(1 << 24, -1, np.int32)
    t = table.astype(np.int64)
    code[t[:, 0] << 16 | t[:, 1] << 8 | t[:, 2]] = np.arange(256)
    key = lambda img: code[img[..., 0].astype(np.int64) << 16 | img[..., 1].astype(np.int64) << 8 | img[..., 2].astype(np.int64)]
    ia, ib = key(a), key(b)
    return np.where((ia < 0) | (ib < 0), 1 << 20, np.abs(ia - ib))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depthvis_ab.txt"))
    ap.add_argument("--trace-only", type=int, default=0)
    args = ap.parse_args()
    if args.reps < 20 and not args.trace_only:
        raise SystemExit("depthvis_ab.py reports medians of at least 20 repetitions")
    if not torch.cuda.is_available():
        raise SystemExit("depthvis_ab.py measures on the GPU; there is none here (nothing measured)")
    from s3gaussian_amd import depthvis
    dev = torch.device("cuda:0")
    planes = [tuple(x.to(dev) for x in street(40 + c)) for c in range(N_CAMS)]
    strip = torch.empty((H, N_CAMS * W, 3), dtype=torch.uint8, device=dev)
    pinned = torch.empty(strip.shape, dtype=torch.uint8, pin_memory=True)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]

    def device_route(lo, hi):
        torch.cuda.synchronize()
        ev[0].record()
        for cam, (d, a) in enumerate(planes):
            depthvis.depth_colors(d, a, lo, hi, out=strip, cam=cam, num_cams=N_CAMS)
        ev[1].record()
        pinned.copy_(strip, non_blocking=True)
        ev[2].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), ev[0].elapsed_time(ev[2])

    if args.trace_only:
        for _ in range(args.trace_only):
            for lo, hi in KINDS.values():
                device_route(lo, hi)
        print(f"depthvis_ab.py --trace-only {args.trace_only}: {args.trace_only} timestamps of each kind, nothing timed")
        return
    import matplotlib
    cmap = matplotlib.colormaps["turbo"]
    launches = {"fixed": N_CAMS * depthvis.LAUNCHES_COLORS,
                "automatic": N_CAMS * (depthvis.LAUNCHES_PERCENTILES + depthvis.LAUNCHES_COLORS)}
    lines = [f"# tools/depthvis_ab.py --reps {args.reps} --warmup {args.warmup}: one timestamp of depth_colors, {H} x {W}, {N_CAMS} cameras; routes",
             f"# alternated in one process, medians.  {torch.cuda.get_device_name(0)}; {torch.get_num_threads()} torch threads"]
    for kind, (lo, hi) in KINDS.items():
        times = {"kernels": [], "device": [], "host": []}
        ref = None
        for rep in range(args.warmup + args.reps):
            kernels_ms, device_ms = device_route(lo, hi)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ref = host_route(planes, lo, hi, cmap)
            wall_ms = (time.perf_counter() - t0) * 1e3
            if rep >= args.warmup:
                times["kernels"].append(kernels_ms)
                times["device"].append(device_ms)
                times["host"].append(wall_ms)
        mine = pinned.numpy()
        steps = table_steps(mine, ref, depthvis.TABLE)
        differ = np.any(mine != ref, axis=-1)
        med = {k: statistics.median(v) for k, v in times.items()}
        lines += [f"{kind} bounds ({lo}, {hi}): {launches[kind]} launches per timestamp on the device route",
                  f"  kernels  ms per timestamp (device, events; 3 calls): median {med['kernels']:.4f}  min {min(times['kernels']):.4f}  max {max(times['kernels']):.4f}",
                  f"  device   ms per timestamp (device, events; kernels + {pinned.numel() / 1e6:.1f} MB of uint8 into pinned memory): median {med['device']:.4f}  "
                  f"min {min(times['device']):.4f}  max {max(times['device']):.4f}",
                  f"  host     ms per timestamp (host wall clock; 6 fp32 copies of {H * W * 4 / 1e6:.1f} MB, numpy + matplotlib): median {med['host']:.2f}  "
                  f"min {min(times['host']):.2f}  max {max(times['host']):.2f}",
                  f"  host / device (medians): {med['host'] / med['device']:.1f} x;  pixels whose bytes differ: {int(differ.sum())} of {differ.size} "
                  f"({differ.mean():.2e}), largest distance {int(steps.max())} table step(s)"]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
