#!/usr/bin/env python
"""Evaluation video frames: the native route against the reference's host route, on the same device images.

Workload: one timestamp of the five default keys (gt_rgbs, rgbs, depths, dynamic_rgbs, static_rgbs) at 1066 x 1600, three cameras:
fifteen fp32 images on the device in, five uint8 strips ([1066, 4800, 3], and [1066, 4800, 1] for the depths) on the host out.

  native     three frames.compose calls (one per camera, five jobs each) into device strips, then the five strips copied into pinned
             host memory with non_blocking copies -- what pipeline.evaluate_video(host=True) enqueues per timestamp.  Device time
             between two events around all of it; the compose kernels alone between two events of their own.
  reference  utils/video_utils.py:180-201 and 465-489 on the same device images: `.permute(1, 2, 0).cpu().numpy()` per image, the
             depth `/=` its own max(), np.concatenate of the three cameras, to8b.  Host work with blocking copies: wall clock.

    python tools/frames_ab.py [--reps 20] [--warmup 3] [--out profiles/frames_ab.txt]

The two routes alternate; medians over the repetitions.  numpy and torch stay within the CPUs the job was given.  The compose kernels'
achieved bytes per second (12 B read + 3 B written per RGB pixel; 4 B read twice + 1 B written per depth pixel) is printed beside the
HBM figure of bench.py.  Both routes' strips are compared byte for byte.  There is no speed gate."""
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

KEYS = ("gt_rgbs", "rgbs", "depths", "dynamic_rgbs", "static_rgbs")
H, W, N_CAMS = 1066, 1600, 3


def to8b(x):
    return (255 * np.clip(x, 0, 1)).astype(np.uint8)


def reference_route(images):
    strips = {}
    for k in KEYS:
        frames = []
        for img in images[k]:
            a = img.permute(1, 2, 0).cpu().numpy()
            if k == "depths":
                a /= a.max()
            frames.append(a)
        strips[k] = to8b(np.concatenate(frames, axis=1))
    return strips


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_ab.txt"))
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("frames_ab.py reports medians of at least 20 repetitions")
    if not torch.cuda.is_available():
        raise SystemExit("frames_ab.py measures on the GPU; there is none here (nothing measured)")
    import bench
    from s3gaussian_amd import frames
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    images = {k: [((torch.rand(1, H, W, generator=g) * 76 + 4) if k == "depths" else (torch.rand(3, H, W, generator=g) * 1.4 - 0.2)).to(dev)
                  for _ in range(N_CAMS)] for k in KEYS}
    strips = [torch.empty(frames.strip_shape(H, W, 1 if k == "depths" else 3, N_CAMS), dtype=torch.uint8, device=dev) for k in KEYS]
    pinned = [torch.empty(s.shape, dtype=torch.uint8, pin_memory=True) for s in strips]
    normalize = [k == "depths" for k in KEYS]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]

    def native_route():
        torch.cuda.synchronize()
        ev[0].record()
        for cam in range(N_CAMS):
            frames.compose([images[k][cam] for k in KEYS], strips, cam, normalize=normalize)
        ev[1].record()
        for s, p in zip(strips, pinned):
            p.copy_(s, non_blocking=True)
        ev[2].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), ev[0].elapsed_time(ev[2])

    times = {"compose": [], "native": [], "reference": []}
    ref = None
    for rep in range(args.warmup + args.reps):
        compose_ms, native_ms = native_route()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ref = reference_route(images)
        wall_ms = (time.perf_counter() - t0) * 1e3
        if rep >= args.warmup:
            times["compose"].append(compose_ms)
            times["native"].append(native_ms)
            times["reference"].append(wall_ms)
    same = all(np.array_equal(p.numpy(), ref[k]) for k, p in zip(KEYS, pinned))
    pixels = H * W * N_CAMS
    moved = pixels * (4 * 15 + 4 * 2 + 1)                     # four RGB keys: 12 B + 3 B; depths: 4 B in each pass + 1 B
    out_bytes = sum(p.numel() for p in pinned)
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = [f"# tools/frames_ab.py --reps {args.reps} --warmup {args.warmup}: one timestamp of {len(KEYS)} keys, {H} x {W}, {N_CAMS} cameras; routes",
             f"# alternated, medians.  {torch.cuda.get_device_name(0)}; {torch.get_num_threads()} torch threads",
             f"  compose    ms per timestamp (device, events; 3 calls, 6 launches): median {med['compose']:.4f}  min {min(times['compose']):.4f}  max {max(times['compose']):.4f}",
             f"  native     ms per timestamp (device, events; compose + {out_bytes / 1e6:.1f} MB of uint8 into pinned memory): median {med['native']:.4f}  "
             f"min {min(times['native']):.4f}  max {max(times['native']):.4f}",
             f"  reference  ms per timestamp (host wall clock; 15 fp32 copies of {H * W * 12 / 1e6:.1f} / {H * W * 4 / 1e6:.1f} MB, numpy): median {med['reference']:.2f}  "
             f"min {min(times['reference']):.2f}  max {max(times['reference']):.2f}",
             f"  reference / native (medians): {med['reference'] / med['native']:.1f} x;  strips byte-equal: {same}",
             f"  compose kernels: {moved / 1e6:.1f} MB moved per timestamp -> {moved / 1e6 / med['compose']:.0f} GB/s "
             f"({moved / 1e6 / med['compose'] / bench.PEAK_HBM_GBS:.3f} of the {bench.PEAK_HBM_GBS:.0f} GB/s HBM figure of bench.py)"]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")
    if not same:
        raise SystemExit("the two routes' strips differ")


if __name__ == "__main__":
    main()
