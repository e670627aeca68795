#!/usr/bin/env python
"""Evaluation LPIPS, VGG16 variant: one s3gaussian_amd.lpips_vgg call against the same arithmetic on torch ops, on the same device.

  hip       lpips_vgg(model, image, gt): csrc/lpips_vgg.hip over csrc/lpips_conv.hpp, 24 launches, weights packed once.
  torch     F.conv2d / F.max_pool2d and the normalisation on torch ops, fp32, both images as one batch of 2, weights moved to the
            device ONCE -- kinder to it than the reference's lpips(), which builds the network and reloads both weight files on
            every call (lpipsPyTorch/__init__.py:19-21).  Its backend is free to choose a convolution algorithm (Winograd, say) that
            an exact k-ordered fma chain cannot match; no ratio is promised.

    python tools/lpips_vgg_ab.py [--shapes 1066x1600,640x960] [--reps 20] [--warmup 3] [--out profiles/lpips_vgg_ab.txt]
                                 [--trace-only N] [--layer-table DIR]

Device-event times around each call, routes alternating in one process; medians, minima and maxima over the repetitions.  Weights are
tests/lpips_vgg_ref.synthetic_weights(7): the real ones exist on no machine this runs on, and the arithmetic does not depend on them.
The two routes' values are compared with each other (a float64 evaluation on the CPU takes minutes at these sizes; the tests do it at
theirs).
--trace-only N: N hip calls at the first shape and nothing else, for a `rocprofv3 --kernel-trace --stats` run of its own.
--layer-table DIR: read such a run's kernel_trace.csv, take the launches in start order, and print every layer's time, GFLOP and TF
for the first shape (the thirteen convolutions of a call are told apart by their order: several share one kernel instantiation);
needs no GPU."""
import argparse
import csv
import glob
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import lpips_vgg_ref as lv  # noqa: E402

PEAK_TF = 157.3            # fp32 matrix peak of the MI355X
NAMES = ("conv1_1", "conv1_2", "conv2_1", "conv2_2", "conv3_1", "conv3_2", "conv3_3", "conv4_1", "conv4_2", "conv4_3", "conv5_1",
         "conv5_2", "conv5_3")


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def torch_route(weights, dev):
    conv_w = [torch.from_numpy(w).to(dev) for w in weights["conv_w"]]
    conv_b = [torch.from_numpy(b).to(dev) for b in weights["conv_b"]]
    lin_w = [torch.from_numpy(w).to(dev)[None, :, None, None] for w in weights["lin_w"]]
    mean = torch.tensor(lv.MEAN, device=dev)[None, :, None, None]
    std = torch.tensor(lv.STD, device=dev)[None, :, None, None]

    def run(x, y):
        a = (torch.stack((x, y)) - mean) / std
        taps = []
        for l in range(13):
            a = F.relu(F.conv2d(a, conv_w[l], conv_b[l], padding=1))
            if l in lv.TAP_CONVS:
                n = a / (torch.sqrt((a * a).sum(1, keepdim=True)) + lv.EPS)
                taps.append((((n[0] - n[1]) ** 2)[None] * lin_w[len(taps)]).sum(1).mean())
                if l != 12:
                    a = F.max_pool2d(a, 2, 2)
        return torch.stack(taps)
    return run


def layer_sizes(H, W):
    """[(h, w, flop)] of the thirteen convolutions: both images, 2 flop per multiply-add."""
    out, h, w = [], H, W
    for l, (ci, co) in enumerate(lv.CHANNELS):
        out.append((h, w, 2.0 * 2 * h * w * co * ci * 9))
        if l in lv.TAP_CONVS:
            h, w = h // 2, w // 2
    return out


def layer_table(directory, H, W):
    f = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if not f:
        sys.exit("no kernel_trace.csv under " + directory)
    rows = [r for r in csv.DictReader(open(f[0])) if "lpips" in r["Kernel_Name"] and "pack" not in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    convs = [dur(r) for r in rows if "lpips_conv_kernel" in r["Kernel_Name"]]
    calls = len(convs) // 13
    assert calls > 0 and len(convs) == 13 * calls, len(convs)
    per_layer = np.array(convs).reshape(calls, 13)
    sizes = layer_sizes(H, W)
    lines = [f"# per-layer time (median of {calls} calls), GFLOP and achieved TF against the {PEAK_TF} TF fp32 matrix peak "
             f"({H} x {W}, from {os.path.basename(f[0])})"]
    for l, (ci, co) in enumerate(lv.CHANNELS):
        us = float(np.median(per_layer[:, l]))
        tf = sizes[l][2] / (us * 1e-6) / 1e12
        lines.append(f"{NAMES[l]} {ci:3d} -> {co:3d} at {sizes[l][0]:4d} x {sizes[l][1]:4d}: {us:8.1f} us  {sizes[l][2] / 1e9:7.2f} GFLOP  "
                     f"{tf:6.1f} TF  {100 * tf / PEAK_TF:5.1f} % of peak")
    for tag in ("lpips_vgg_front_kernel", "lpips_pool_kernel", "lpips_tap_kernel", "lpips_finalize_kernel"):
        us = sum(dur(r) for r in rows if tag in r["Kernel_Name"]) / calls
        lines.append(f"{tag}: {us:8.1f} us per call")
    total = sum(dur(r) for r in rows) / calls / 1e3
    flop = sum(s[2] for s in sizes)
    lines.append(f"all kernels of one call: {total:.3f} ms, {flop / 1e12:.3f} TFLOP of convolutions = {flop / (total * 1e-3) / 1e12:.1f} TF "
                 f"over the whole call")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1066x1600,640x960")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_vgg_ab.txt"))
    ap.add_argument("--trace-only", type=int, default=0)
    ap.add_argument("--layer-table", default=None)
    args = ap.parse_args()
    shapes = [tuple(int(v) for v in s.split("x")) for s in args.shapes.split(",")]
    if args.layer_table:
        print("\n".join(layer_table(args.layer_table, *shapes[0])))          # to stdout: profiles/lpips_vgg_kstats.txt is this
        return                                                                # table followed by tools/kstats.py's
    from s3gaussian_amd.lpips_vgg import LPIPSVGG, lpips_vgg
    dev = torch.device("cuda:0")
    weights = lv.synthetic_weights(lv.WEIGHT_SEED)
    model = LPIPSVGG.from_state_dicts(lv.vgg_state_dict(weights), lv.lin_state_dict(weights), dev)
    if args.trace_only:
        H, W = shapes[0]
        x, y = (torch.from_numpy(t).to(dev) for t in lv.images(H, W, lv.image_seed(H, W)))
        for _ in range(args.trace_only):
            lpips_vgg(model, x, y)
        torch.cuda.synchronize()
        return
    run_torch = torch_route(weights, dev)
    lines = [f"# tools/lpips_vgg_ab.py --shapes {args.shapes} --reps {args.reps} --warmup {args.warmup}: device-event ms per call, "
             f"routes alternating in one process; synthetic weights (seed {lv.WEIGHT_SEED})"]
    print(lines[0], flush=True)
    for H, W in shapes:
        first = len(lines)
        x, y = (torch.from_numpy(t).to(dev) for t in lv.images(H, W, lv.image_seed(H, W)))
        times = {"hip": [], "torch": []}
        with torch.no_grad():
            for i in range(args.warmup + args.reps):
                t_hip, rec = events(lambda: lpips_vgg(model, x, y))
                t_torch, taps = events(lambda: run_torch(x, y))
                if i >= args.warmup:
                    times["hip"].append(t_hip)
                    times["torch"].append(t_torch)
        flop = sum(s[2] for s in layer_sizes(H, W))
        lines.append(f"## {H} x {W}: {flop / 1e12:.3f} TFLOP of convolutions per call")
        for name in ("hip", "torch"):
            t = times[name]
            lines.append(f"{name:6s} median {statistics.median(t):8.3f} ms   min {min(t):8.3f}   max {max(t):8.3f}   ({len(t)} repetitions)"
                         f"   {flop / (statistics.median(t) * 1e-3) / 1e12:6.1f} TF")
        ratio = statistics.median(times["torch"]) / statistics.median(times["hip"])
        lines.append(f"torch / hip = {ratio:.3f}  ({'hip is no slower' if ratio >= 1.0 else 'hip is SLOWER than the torch-op route'})")
        got, tor = rec.cpu().numpy(), taps.double().cpu().numpy()
        lines.append(f"hip   total {got[0]:.9g} taps {got[1:]}")
        lines.append(f"torch total {tor.sum():.9g} taps {tor}")
        lines.append(f"hip against torch, relative difference per tap {np.abs(got[1:] - tor) / tor}")
        print("\n".join(lines[first:]), flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
