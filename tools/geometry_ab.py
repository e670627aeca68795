#!/usr/bin/env python
"""Scale / rotation / opacity deformation (ModelHiddenParams no_ds = no_dr = no_do = False): the fused deformation route with the
geometry heads (include/s3g_mlp_geom.h) against the library-GEMM route this configuration took before it was admitted to the fused one.

Workload: one scene from synth.street_scene at the benchmark shape (1.2 M Gaussians, 1066 x 1600, fine stage), all three heads on,
their output layers drawn with std 0.02 (xavier leaves ds / dr / do of order 1: a destroyed scene is another rasterizer workload).

  fused     pipeline.training_step as it runs: sampler -> s3g_deform_mlp_forward + s3g_deform_geom_forward on the same features ->
            three small adds -> glue kernel -> two-image rasterizer node, mean|dshs| and the plane regulariser riding on the glue and
            sampler nodes.
  library   the same call with `_fused_ok` and `_fused_geometry_ok` shadowed by `lambda: False` on the module (as
            tests/test_geometry_route_gpu.py forces it): feature_out and the six heads as library GEMMs, `shs + dshs` materialised,
            the glue in PyTorch, the regularisers in sweeps of their own.  No user option selects this; it is what the parent commit
            ran for this configuration.

    python tools/geometry_ab.py [--steps 20] [--warmup 3] [--out profiles/geometry_ab.txt]

One model, one process: after the warm-up the two routes alternate step by step (both compute the same step, so the state they
share moves the same way); a device synchronise on both sides of every timed block, wall clock, medians.  Then render ms/frame under
no_grad both ways, cycling through cameras of different timestamps so that every frame evaluates the deformation field.  A record,
not a gate."""
import argparse
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

P, W, H = 1_200_000, 1600, 1066


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=P)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geometry_ab.txt"))
    args = ap.parse_args()
    if args.steps < 20:
        raise SystemExit("geometry_ab.py reports medians of at least 20 steps per route")
    if not torch.cuda.is_available():
        raise SystemExit("geometry_ab.py measures on the GPU; there is none here (nothing measured)")
    import bench
    from s3gaussian_amd import synth
    from s3gaussian_amd.pipeline import GaussianParams, default_hyper, default_opt, render, training_step
    dev = torch.device("cuda:0")
    sc = synth.street_scene(P=args.points, seed=0, width=W, height=H, n_frames=4)
    hyper, opt = default_hyper(no_ds=False, no_dr=False, no_do=False), default_opt()
    torch.manual_seed(0)
    pc = GaussianParams(sc["sh_degree"], hyper)
    gs = sc["gaussians"]
    pc.init_from_tensors(gs["xyz"], gs["log_scales"], gs["rotations_raw"], gs["opacity_logit"], gs["shs"], dev)
    net = pc._deformation.deformation_net
    net.set_aabb(*sc["aabb"])
    with torch.no_grad():
        for head in (net.scales_deform, net.rotations_deform, net.opacity_deform):
            for p in (head[3].weight, head[3].bias):
                p.normal_(std=0.02)
    pc.training_setup(opt)
    assert net._fused_geometry_ok() and not net._fused_ok()
    cams = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in c.items()} for c in sc["cameras"]]
    bg = sc["bg"].to(dev)
    pipe = SimpleNamespace(convert_SHs_python=True, compute_cov3D_python=False, debug=False)
    by_time = {}
    for c in cams:
        by_time.setdefault(float(c["time"]), c)
    views = list(by_time.values())                      # one camera per timestamp
    targets = [bench.make_targets(pc, c, bg, hyper, seed=i) for i, c in enumerate(views)]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def on_route(fused, fn):
        if fused:
            return timed(fn)
        net._fused_ok = net._fused_geometry_ok = lambda: False
        try:
            return timed(fn)
        finally:
            del net._fused_ok, net._fused_geometry_ok

    times = {"step fused": [], "step library": [], "render fused": [], "render library": []}
    seen = {}
    for i in range(args.warmup + args.steps):
        for fused in (True, False):
            v = i % len(views)

            def step():
                _, pkg = training_step(pc, views[v], *targets[v], hyper, opt, bg, pipe=pipe, densify_stats=True)
                seen[fused] = "dshs_l1" in pkg and "plane_reg" in pkg
            ms = on_route(fused, step)
            if i >= args.warmup:
                times["step fused" if fused else "step library"].append(ms)
    assert seen == {True: True, False: False}, seen     # the two routes really are two routes
    with torch.no_grad():
        for i in range(args.warmup + args.steps):
            for fused in (True, False):
                ms = on_route(fused, lambda: render(views[i % len(views)], pc, pipe, bg, stage="fine"))
                if i >= args.warmup:
                    times["render fused" if fused else "render library"].append(ms)
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = [f"# tools/geometry_ab.py --steps {args.steps} --warmup {args.warmup}: no_ds = no_dr = no_do = False, {args.points} Gaussians, {H} x {W}, stage fine;",
             f"# one model, routes alternated step by step, synchronised wall clock, medians.  {torch.cuda.get_device_name(0)}"]
    for k in times:
        lines.append(f"  {k:<15} ms: median {med[k]:8.3f}  min {min(times[k]):8.3f}  max {max(times[k]):8.3f}   ({len(times[k])} samples)")
    lines.append(f"  library / fused (medians): training step {med['step library'] / med['step fused']:.2f} x, "
                 f"render {med['render library'] / med['render fused']:.2f} x")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
