#!/usr/bin/env python
"""The sky-mask loss on the accumulated opacity: what it adds to a training step, on the route built for it and on the only route
the parent commit allows.

Workload: one scene from synth.street_scene at the benchmark shape (1.2 M Gaussians, 1066 x 1600, fine stage, default heads).

  a  plain    pipeline.training_step without the term: the parent's step.
  b  alpha    the same call with sky_mask= and opt.lambda_sky > 0: the two-image rasterizer node also returns the opacity image
              (s3g_raster_alpha), s3g_sky_loss leaves value and gradient image, and the gradient rides in the node's own backward
              (s3g_raster_backward_alpha), fused densify statistics included.
  c  third    the term built from what the parent has: a third rasterizer call with unit colours on a black background on the same
              geometry tensors (one more blend forward through the geometry cache, one more full backward), torch's
              binary_cross_entropy on its red channel, autograd adding the two backward passes.  The densification statistics then
              need the separate pass over the summed viewspace gradient: the two-image node no longer yields the whole of it.

    python tools/alpha_ab.py [--steps 20] [--warmup 3] [--only a|b|c] [--out profiles/alpha_ab.txt]

One model, one process: after the warm-up the three routes alternate step by step; a device synchronise on both sides of every
timed step, wall clock, medians of at least 20.  --only runs one route alone (for a kernel trace).  A record, not a gate."""
import argparse
import math
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

P, W, H = 1_200_000, 1600, 1066
LAMBDA_SKY = 0.05


def sky_mask(dev):
    """Sky above a wavy horizon with a soft ramp of a few pixels, as a bilinearly resized mask has."""
    y = torch.arange(H, dtype=torch.float32, device=dev)[:, None]
    horizon = 0.35 * H + 0.05 * H * torch.sin(torch.arange(W, dtype=torch.float32, device=dev)[None, :] * (2 * math.pi / W))
    return torch.clamp((horizon - y) / 3.0 + 0.5, 0.0, 1.0).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=P)
    ap.add_argument("--only", choices=("a", "b", "c"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alpha_ab.txt"))
    args = ap.parse_args()
    if args.steps < 20 and args.only is None:
        raise SystemExit("alpha_ab.py reports medians of at least 20 steps per route")
    if not torch.cuda.is_available():
        raise SystemExit("alpha_ab.py measures on the GPU; there is none here (nothing measured)")
    import bench
    from s3gaussian_amd import synth
    from s3gaussian_amd.optim import densify_stats
    from s3gaussian_amd.pipeline import GaussianParams, default_hyper, default_opt, render, training_loss, training_step
    from s3gaussian_amd.rasterizer import GaussianRasterizer
    dev = torch.device("cuda:0")
    sc = synth.street_scene(P=args.points, seed=0, width=W, height=H, n_frames=4)
    hyper = default_hyper()
    opt_plain, opt_sky = default_opt(), default_opt(lambda_sky=LAMBDA_SKY)
    torch.manual_seed(0)
    pc = GaussianParams(sc["sh_degree"], hyper)
    gs = sc["gaussians"]
    pc.init_from_tensors(gs["xyz"], gs["log_scales"], gs["rotations_raw"], gs["opacity_logit"], gs["shs"], dev)
    pc._deformation.deformation_net.set_aabb(*sc["aabb"])
    pc.training_setup(opt_plain)
    cams = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in c.items()} for c in sc["cameras"]]
    bg = sc["bg"].to(dev)
    pipe = SimpleNamespace(convert_SHs_python=True, compute_cov3D_python=False, debug=False)
    by_time = {}
    for c in cams:
        by_time.setdefault(float(c["time"]), c)
    views = list(by_time.values())
    targets = [bench.make_targets(pc, c, bg, hyper, seed=i) for i, c in enumerate(views)]
    mask = sky_mask(dev)
    ones = torch.ones(args.points, 3, device=dev)
    black = torch.zeros(3, device=dev)
    stash = {}
    pair = GaussianRasterizer.forward_pair

    def pair_and_third(self, means3D, means2D, opacities, colors_a, colors_b, scales=None, rotations=None, cov3D_precomp=None,
                       densify_accum=None):
        out = pair(self, means3D=means3D, means2D=means2D, opacities=opacities, colors_a=colors_a, colors_b=colors_b, scales=scales,
                   rotations=rotations, cov3D_precomp=cov3D_precomp, densify_accum=densify_accum)
        third = GaussianRasterizer(self.raster_settings._replace(bg=black))
        stash["alpha"] = third(means3D=means3D, means2D=means2D, opacities=opacities, colors_precomp=ones, scales=scales,
                               rotations=rotations, cov3D_precomp=cov3D_precomp)[0][0:1]
        return out

    def step_a(v):
        training_step(pc, views[v], *targets[v], hyper, opt_plain, bg, pipe=pipe, densify_stats=True)

    def step_b(v):
        _, pkg = training_step(pc, views[v], *targets[v], hyper, opt_sky, bg, pipe=pipe, densify_stats=True, sky_mask=mask)
        assert "alpha" in pkg and pkg["densify_stats_fused"]

    def step_c(v):
        GaussianRasterizer.forward_pair = pair_and_third
        try:
            pkg = render(views[v], pc, pipe, bg, stage="fine", return_dx=True, render_feat=True)
        finally:
            GaussianRasterizer.forward_pair = pair
        loss = training_loss(pc, pkg, *targets[v], hyper, opt_plain, "fine")
        loss = loss + LAMBDA_SKY * F.binary_cross_entropy(torch.clamp(stash.pop("alpha")[0], 1e-6, 1 - 1e-6), 1.0 - mask)
        loss.backward()
        densify_stats(pc.xyz_gradient_accum, pc.denom, pc.max_radii2D, pkg["viewspace_points"].grad, pkg["radii"])
        pc.optimizer.step()
        pc.optimizer.zero_grad(set_to_none=True)

    routes = {"a": ("a plain", step_a), "b": ("b alpha", step_b), "c": ("c third", step_c)}
    if args.only:
        routes = {args.only: routes[args.only]}
    times = {name: [] for name, _ in routes.values()}
    for i in range(args.warmup + args.steps):
        for name, step in routes.values():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(i % len(views))
            torch.cuda.synchronize()
            if i >= args.warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = [f"# tools/alpha_ab.py --steps {args.steps} --warmup {args.warmup}: {args.points} Gaussians, {H} x {W}, stage fine, lambda_sky = {LAMBDA_SKY};",
             f"# one model, routes alternated step by step, synchronised wall clock, medians.  {torch.cuda.get_device_name(0)}"]
    for k in times:
        lines.append(f"  step {k:<8} ms: median {med[k]:8.3f}  min {min(times[k]):8.3f}  max {max(times[k]):8.3f}   ({len(times[k])} samples)")
    if len(med) == 3:
        lines.append(f"  b - a = {med['b alpha'] - med['a plain']:.3f} ms, c - a = {med['c third'] - med['a plain']:.3f} ms (medians)")
    text = "\n".join(lines) + "\n"
    if args.only is None:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
