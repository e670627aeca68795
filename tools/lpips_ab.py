#!/usr/bin/env python
"""Evaluation LPIPS: one s3gaussian_amd.lpips call against the same arithmetic on torch ops, on the same device.

  hip       lpips(model, image, gt): csrc/lpips.hip over csrc/lpips_conv.hpp, 14 launches, weights packed once.
  torch     F.conv2d / F.max_pool2d and the normalisation on torch ops, fp32, both images as one batch of 2, weights moved to the
            device ONCE -- kinder to it than the reference's lpips(), which builds the network and reloads both weight files on
            every call (lpipsPyTorch/__init__.py:19-21).

    python tools/lpips_ab.py [--height 1066] [--width 1600] [--reps 20] [--warmup 3] [--out profiles/lpips_ab.txt]
                             [--errors profiles/lpips_errors.json] [--no-f64] [--trace-only N]

Device-event times around each call, routes alternating in one process; medians, minima and maxima over the repetitions.  Weights are
tests/lpips_ref.synthetic_weights(7): the real ones exist on no machine this runs on, and the arithmetic does not depend on them.
Both routes' values are compared with the float64 restatement evaluated on the CPU (skipped with --no-f64); the bar is the one of
tests/test_lpips_gpu.py (4 x the largest relative error of the float32 restatement over the test cases).  --errors also runs the five
test cases and records the float32 route's errors, the bar and the GPU route's errors.
--trace-only N: N hip calls and nothing else, for a `rocprofv3 --kernel-trace --stats` run of its own (tools/kstats.py reduces it).
--conv-table DIR: read such a run's kernel_stats.csv and append each convolution's time and achieved TF to --out."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import lpips_ref as lr  # noqa: E402

PEAK_TF = 157.3            # fp32 matrix peak of the MI355X


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
    mean = torch.tensor(lr.MEAN, device=dev)[None, :, None, None]
    std = torch.tensor(lr.STD, device=dev)[None, :, None, None]

    def run(x, y):
        a = (torch.stack((x, y)) - mean) / std
        taps = []
        for i, (_, _, _, stride, pad, pool) in enumerate(lr.LAYERS):
            a = F.relu(F.conv2d(a, conv_w[i], conv_b[i], stride=stride, padding=pad))
            n = a / (torch.sqrt((a * a).sum(1, keepdim=True)) + lr.EPS)
            taps.append((((n[0] - n[1]) ** 2)[None] * lin_w[i]).sum(1).mean())
            if pool:
                a = F.max_pool2d(a, 3, 2)
        return torch.stack(taps)
    return run


def layer_sizes(H, W):
    out, h, w = [], H, W
    for co, ci, k, stride, pad, pool in lr.LAYERS:
        h, w = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        out.append((h, w, 2.0 * 2 * h * w * co * ci * k * k))          # both images, 2 flop per multiply-add
        if pool:
            h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    return out


def conv_table(directory, H, W):
    f = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    if not f:
        sys.exit("no kernel_stats.csv under " + directory)
    rows = {r["Name"]: r for r in csv.DictReader(open(f[0]))}
    per_call = {}
    for n, r in rows.items():
        if "lpips_" in n and "pack" not in n:
            per_call[n] = float(r["TotalDurationNs"])
    lines = [f"# per-convolution time and achieved TF against the {PEAK_TF} TF fp32 matrix peak ({H} x {W}, from {os.path.basename(f[0])})"]
    sizes = layer_sizes(H, W)
    for l, (co, ci, k, stride, pad, _) in enumerate(lr.LAYERS):
        tag = f"lpips_conv_kernel<{k}, {stride}, {pad}, {ci}, {co}, 64,"
        hit = [r for n, r in rows.items() if tag in n]
        if not hit:
            lines.append(f"conv{l + 1}: not in the trace")
            continue
        us = float(hit[0]["AverageNs"]) / 1e3
        tf = sizes[l][2] / (us * 1e-6) / 1e12
        lines.append(f"conv{l + 1} {ci:3d} -> {co:3d} k{k:<2d} out {sizes[l][0]} x {sizes[l][1]}: {us:8.1f} us  {sizes[l][2] / 1e9:6.2f} GFLOP  "
                     f"{tf:6.1f} TF  {100 * tf / PEAK_TF:5.1f} % of peak")
    calls = max(int(r["Calls"]) for n, r in rows.items() if "lpips_finalize" in n)
    lines.append(f"all lpips kernels of one call: {sum(per_call.values()) / calls / 1e6:.3f} ms ({calls} calls traced)")
    return lines


def evaluate_share(model, points, H, W, dev, lpips_ms):
    """Wall-clock ms per frame of pipeline.evaluate (8 cameras, one host read at the end) with and without the model."""
    import time
    from types import SimpleNamespace
    from s3gaussian_amd import synth
    from s3gaussian_amd.pipeline import GaussianParams, default_hyper, evaluate
    scn = synth.street_scene(P=points, seed=0, width=W, height=H, n_frames=2)
    hyper = default_hyper()
    pc = GaussianParams(3, hyper)
    gs = scn["gaussians"]
    pc.init_from_tensors(gs["xyz"], gs["log_scales"], gs["rotations_raw"], gs["opacity_logit"], gs["shs"], dev)
    pc._deformation.deformation_net.set_aabb(*scn["aabb"])
    cam = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in scn["cameras"][0].items()}
    cams = [dict(cam, time=t / 8) for t in range(8)]
    gts = [torch.rand(3, H, W, device=dev) for _ in cams]
    pipe = SimpleNamespace(convert_SHs_python=True, compute_cov3D_python=False, debug=False)
    bg = scn["bg"].to(dev)
    out = {}
    for name, m in (("without", None), ("with", model), ("without", None), ("with", model)):      # first pair warms up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        evaluate(pc, cams, gts, pipe, bg, lpips=m)
        torch.cuda.synchronize()
        out[name] = (time.perf_counter() - t0) * 1e3 / len(cams)
    share = 100 * (out["with"] - out["without"]) / out["with"]
    return [f"# pipeline.evaluate, {points} Gaussians, {H} x {W}, 8 cameras: wall-clock ms per frame",
            f"evaluate without lpips {out['without']:.3f} ms/frame, with {out['with']:.3f} ms/frame: LPIPS is {share:.1f} % of a frame "
            f"(the call alone: {lpips_ms:.3f} ms)"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1066)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpips_ab.txt"))
    ap.add_argument("--errors", default=None)
    ap.add_argument("--no-f64", action="store_true")
    ap.add_argument("--trace-only", type=int, default=0)
    ap.add_argument("--conv-table", default=None)
    ap.add_argument("--evaluate", type=int, default=0, metavar="POINTS",
                    help="also time pipeline.evaluate on a synthetic street scene of POINTS Gaussians, with and without the model")
    args = ap.parse_args()
    H, W = args.height, args.width
    if args.conv_table:
        lines = conv_table(args.conv_table, H, W)
        print("\n".join(lines))
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
        return
    from s3gaussian_amd.lpips import LPIPS, lpips
    dev = torch.device("cuda:0")
    weights = lr.synthetic_weights(lr.WEIGHT_SEED)
    model = LPIPS.from_state_dicts(lr.alexnet_state_dict(weights), lr.lin_state_dict(weights), dev)
    x_np, y_np = lr.images(H, W, lr.image_seed(H, W))
    x, y = torch.from_numpy(x_np).to(dev), torch.from_numpy(y_np).to(dev)
    if args.trace_only:
        for _ in range(args.trace_only):
            lpips(model, x, y)
        torch.cuda.synchronize()
        return
    run_torch = torch_route(weights, dev)
    lines = [f"# tools/lpips_ab.py --height {H} --width {W} --reps {args.reps} --warmup {args.warmup}: device-event ms per call, "
             f"routes alternating in one process; synthetic weights (seed {lr.WEIGHT_SEED})"]
    times = {"hip": [], "torch": []}
    with torch.no_grad():
        for i in range(args.warmup + args.reps):
            t_hip, rec = events(lambda: lpips(model, x, y))
            t_torch, taps = events(lambda: run_torch(x, y))
            if i >= args.warmup:
                times["hip"].append(t_hip)
                times["torch"].append(t_torch)
    for name in ("hip", "torch"):
        t = times[name]
        lines.append(f"{name:6s} median {statistics.median(t):8.3f} ms   min {min(t):8.3f}   max {max(t):8.3f}   ({len(t)} repetitions)")
    ratio = statistics.median(times["torch"]) / statistics.median(times["hip"])
    lines.append(f"torch / hip = {ratio:.3f}  ({'hip is no slower' if ratio >= 1.0 else 'hip is SLOWER than the torch-op route'})")
    got = rec.cpu().numpy()
    tor = taps.double().cpu().numpy()
    lines.append(f"hip   total {got[0]:.9g} taps {got[1:]}")
    lines.append(f"torch total {tor.sum():.9g} taps {tor}")
    ref64, rel, bar = lr.float32_route_errors(weights)
    lines.append(f"bar {bar:.3e} = {lr.BAR_FACTOR:g} x the float32 restatement's largest relative error over the test cases ({rel.max():.3e})")
    if not args.no_f64:
        want = lr.lpips_ref(x_np, y_np, weights, torch.float64).numpy()
        e_hip, e_torch = np.abs(got[1:] - want) / want, np.abs(tor - want) / want
        lines.append(f"float64 restatement (CPU) total {want.sum():.12g}")
        lines.append(f"hip   relative error per tap {e_hip} -> {'within' if e_hip.max() <= bar else 'OUTSIDE'} the bar")
        lines.append(f"torch relative error per tap {e_torch} -> {'within' if e_torch.max() <= bar else 'OUTSIDE'} the bar")
    else:
        d = np.abs(got[1:] - tor) / tor
        lines.append(f"hip against torch, relative difference per tap {d} (no float64 evaluation at this size in this run)")
    print("\n".join(lines))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if args.evaluate:
        lines = evaluate_share(model, args.evaluate, H, W, dev, statistics.median(times["hip"]))
        print("\n".join(lines))
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    if args.errors:
        cases = lr.all_cases()
        gpu = []
        for _, _, cx, cy in cases:
            r = lpips(model, torch.from_numpy(cx).to(dev), torch.from_numpy(cy).to(dev)).cpu().numpy()
            gpu.append(r[1:])
        gpu_rel = np.abs(np.stack(gpu) - ref64) / ref64
        doc = {"weights_seed": lr.WEIGHT_SEED, "cases": [f"{h}x{w}" for h, w, _, _ in cases],
               "tap_values_float64": ref64.tolist(), "float32_restatement_relative_error": rel.tolist(),
               "float32_restatement_largest": float(rel.max()), "bar_factor": lr.BAR_FACTOR, "bar": bar,
               "gpu_relative_error": gpu_rel.tolist(), "gpu_largest": float(gpu_rel.max())}
        with open(args.errors, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        print(f"wrote {args.errors}: float32 route largest {rel.max():.3e}, bar {bar:.3e}, GPU largest {gpu_rel.max():.3e}")


if __name__ == "__main__":
    main()
