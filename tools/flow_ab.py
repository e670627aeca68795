#!/usr/bin/env python
"""Scene-flow images: the native route against what a user had before it existed.

  colours   s3gaussian_amd.flow.scene_flow_colors (two kernels, nothing leaves the device) against the arithmetic of the reference's
            utils/visualization_tools.py::scene_flow_to_rgb restated on torch ops ON THE DEVICE: min, max, normalise, hypot, atan2,
            two gathers from the 56-entry wheel, the two radius branches -- about 30 launches.  (The reference itself evaluates this
            on the host and copies 14 MB each way per image at 1.2 M Gaussians; that is not timed here.)  1.2 M points.
  frames    pipeline.render_flows(with_rgb=True) over 4 timestamps x 3 cameras against the reference's loop for the same 12 frames
            (utils/video_utils.py:173, 267, 284): the frame's own render plus two `render(override_color=...)` calls, with the
            colours of both routes evaluated by the native kernel, outside the bracket for the second route -- what is compared is
            the rendering.  BASELINE cfg3 size: 1.2 M Gaussians, 1600 x 1066.  Reported per frame (RGB + two flow images).

    python tools/flow_ab.py [--reps 20] [--warmup 3] [--out profiles/flow_ab.txt] [--points 1200000]

The two routes alternate; every call (colours) or pass over the 12 frames (frames) is bracketed by events on the current stream;
medians over the repetitions.  The two routes' results are compared as well.  There is no speed gate."""
import argparse
import math
import os
import statistics
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def make_wheel(dev):
    hues = torch.tensor([[255, 0, 0], [255, 255, 0], [0, 255, 0], [0, 255, 255], [0, 0, 255], [255, 0, 255], [255, 0, 0]], dtype=torch.float64)
    rows = []
    for k, length in enumerate((15, 6, 4, 11, 13, 6)):
        steps = torch.arange(length, dtype=torch.float64)[:, None] / length
        rows.append((hues[k] + (hues[k + 1] - hues[k]) * steps).to(torch.uint8))
    wheel = torch.cat(rows).float()
    return torch.cat([wheel, wheel[:1]]).to(dev)


def torch_colors(dx_a, dx_b, wheel):
    """scene_flow_to_rgb(dx_b - dx_a, background="bright", flow_max_radius=1.0) op by op, on the device."""
    flow = dx_b - dx_a
    lo, hi = flow.min(), flow.max()
    flow = (flow - lo) / (hi - lo + 1e-6)
    cf = flow[..., 0] + 1j * flow[..., 1]
    radius, angle = torch.abs(cf), torch.angle(cf)
    radius = radius / 1.0
    angle[angle < 0] += 2 * math.pi
    angle = angle * ((wheel.shape[0] - 2) / (2 * math.pi))
    frac, lo_i, hi_i = torch.fmod(angle, 1).unsqueeze(-1), angle.trunc(), torch.ceil(angle)
    hue = wheel[lo_i.long()] * (1 - frac) + wheel[hi_i.long()] * frac
    colors = 255.0 - radius.unsqueeze(-1) * (255.0 - hue)
    over = radius > 1
    colors[over] = hue[over] * (1 / radius[over]).unsqueeze(-1)
    return colors / 255.0


def bracket(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def summary(lines, times, unit):
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        lines.append(f"  {k:8s} ms per {unit}: median {med[k]:.4f}  min {min(v):.4f}  max {max(v):.4f}")
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=1_200_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flow_ab.txt"))
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("flow_ab.py reports medians of at least 20 repetitions")
    if not torch.cuda.is_available():
        raise SystemExit("flow_ab.py measures on the GPU; there is none here (nothing measured)")
    import bench
    from s3gaussian_amd import flow
    from s3gaussian_amd.pipeline import _uniform_time, render, render_flows
    dev = torch.device("cuda:0")
    P = args.points
    lines = [f"# tools/flow_ab.py --reps {args.reps} --warmup {args.warmup} --points {P}: scene-flow colours and flow frames, native route vs the",
             f"# route a user had before, alternated, events around every call / pass, medians.  {torch.cuda.get_device_name(0)}"]

    # ---- colours ------------------------------------------------------------------------------------------------------------------
    g = torch.Generator().manual_seed(0)
    dx_a = (0.05 * torch.randn(P, 3, generator=g)).to(dev)
    dx_b = dx_a + (0.02 * torch.randn(P, 3, generator=g)).to(dev)
    wheel = make_wheel(dev)
    out = torch.empty_like(dx_a)
    times, res = {"native": [], "torch": []}, {}
    for rep in range(args.warmup + args.reps):
        for route in ("native", "torch"):
            fn = (lambda: flow.scene_flow_colors(dx_a, dx_b, out=out)) if route == "native" else (lambda: torch_colors(dx_a, dx_b, wheel))
            ms, res[route] = bracket(fn)
            if rep >= args.warmup:
                times[route].append(ms)
    lines.append(f"colours of {P} Gaussians (36 B per Gaussian + the range pass = {P * 60 / 1e6:.0f} MB moved by the native route)")
    med = summary(lines, times, "call")
    lines.append(f"  torch / native (medians): {med['torch'] / med['native']:.1f} x;  native {P * 60 / 1e6 / med['native']:.0f} GB/s;  "
                 f"|native - torch| max {float((res['native'] - res['torch']).abs().max()):.2e}")

    # ---- frames -------------------------------------------------------------------------------------------------------------------
    W, H, n_frames = 1600, 1066, 4
    pc, cams, hyper, opt, bg = bench.build_scene(P, W, H, n_frames, dev)
    with torch.no_grad():   # a position head that moves the Gaussians, and time planes (all ones at init) that make it depend on time
        for p in pc._deformation.deformation_net.pos_deform.parameters():
            p.add_(0.05 * torch.randn_like(p))
        for p in pc._deformation.deformation_net.grid.grids.parameters():
            p.add_(0.2 * torch.randn_like(p))
    pipe = SimpleNamespace(convert_SHs_python=True, compute_cov3D_python=False, debug=False)
    cams = cams[:3 * n_frames]
    fplan, bplan = flow.frame_plan(len(cams), 3)
    net = pc._deformation.deformation_net
    with torch.no_grad():
        dx = {}
        for cam in cams:
            if cam["time"] not in dx:
                dx[cam["time"]] = net.deform_heads(pc.get_xyz, _uniform_time(cam["time"], dev), uniform_time=True, need_feat=False)[0].clone()
        col = lambda p: flow.scene_flow_colors(dx[cams[p.from_frame]["time"]], dx[cams[p.to_frame]["time"]])
        colors = [(col(f), col(b)) for f, b in zip(fplan, bplan)]

        def reference_loop():
            imgs = []
            for cam, (cf, cb) in zip(cams, colors):
                imgs.append(render(cam, pc, pipe, bg, return_dx=True)["render"])
                imgs.append(render(cam, pc, pipe, bg, override_color=cf)["render"])
                imgs.append(render(cam, pc, pipe, bg, override_color=cb)["render"])
            return imgs

        def native_pass():
            r = render_flows(pc, cams, pipe, bg, num_cams=3, with_rgb=True)
            return [img for trio in zip(r["rgbs"], r["forward_flows"], r["backward_flows"]) for img in trio]

        times, res = {"native": [], "override": []}, {}
        for rep in range(args.warmup + args.reps):
            for route in ("native", "override"):
                ms, res[route] = bracket(native_pass if route == "native" else reference_loop)
                if rep >= args.warmup:
                    times[route].append(ms / len(cams))
    lines.append(f"frames: {P} Gaussians, {H} x {W}, {n_frames} timestamps x 3 cameras, RGB + forward + backward flow image per frame")
    med = summary(lines, times, "frame")
    worst = max(float((a - b).abs().max()) for a, b in zip(res["native"], res["override"]))
    lines.append(f"  override / native (medians): {med['override'] / med['native']:.2f} x;  |native - override| max over the {len(res['native'])} images {worst:.2e}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
