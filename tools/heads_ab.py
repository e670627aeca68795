#!/usr/bin/env python
"""Networks without the SH head or the feature head (ModelHiddenParams no_dshs / feat_head): the fused deformation route against
the library-GEMM route these configurations took before `Deformation._fused_heads_ok` admitted them to the fused one.

Workload: one scene from synth.street_scene at the benchmark shape (1.2 M Gaussians, 1066 x 1600, fine stage) per configuration:
  feat_head=False                                            training without pre-extracted feature maps
  no_dshs=True
  no_dshs=True, feat_head=False, no_ds=False, no_dr=False    4D-Gaussian-Splatting's default

  fused     pipeline.training_step as it runs: sampler -> s3g_deform_mlp_forward with the absent heads' outputs NULL (the chain
            kernels without the SH head for no_dshs) (+ s3g_deform_geom_forward) -> glue kernel -> rasterizer, the regularisers riding
            on the glue and sampler nodes.
  library   the same call with `_fused_heads_ok = lambda: False` on the module: feature_out and the heads as library GEMMs, the glue
            in PyTorch, the regularisers in sweeps of their own.  No user option selects this; it is what the parent commit ran.

    python tools/heads_ab.py [--steps 20] [--warmup 3] [--out profiles/heads_ab.txt]

One model per configuration, one process: after the warm-up the two routes alternate step by step (both compute the same step, so
the state they share moves the same way); a device synchronise on both sides of every timed block, wall clock, medians.  Then render
ms/frame under no_grad both ways, cycling through cameras of different timestamps so that every frame evaluates the deformation field.
Exit status 1 if the fused route is slower than the library route in any of the six pairs."""
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
CONFIGS = [("feat_head=False", dict(feat_head=False)), ("no_dshs=True", dict(no_dshs=True)),
           ("no_dshs=True feat_head=False no_ds=False no_dr=False", dict(no_dshs=True, feat_head=False, no_ds=False, no_dr=False))]


def measure(name, over, sc, args, dev):
    from s3gaussian_amd import raster_C
    from s3gaussian_amd.pipeline import GaussianParams, default_hyper, default_opt, render, training_step
    hyper, opt = default_hyper(**over), default_opt()
    torch.manual_seed(0)
    pc = GaussianParams(sc["sh_degree"], hyper)
    gs = sc["gaussians"]
    pc.init_from_tensors(gs["xyz"], gs["log_scales"], gs["rotations_raw"], gs["opacity_logit"], gs["shs"], dev)
    net = pc._deformation.deformation_net
    net.set_aabb(*sc["aabb"])
    pc.training_setup(opt)
    assert net._fused_heads_ok()
    cams = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in c.items()} for c in sc["cameras"]]
    bg = sc["bg"].to(dev)
    pipe = SimpleNamespace(convert_SHs_python=True, compute_cov3D_python=False, debug=False)
    by_time = {}
    for c in cams:
        by_time.setdefault(float(c["time"]), c)
    views = list(by_time.values())                      # one camera per timestamp
    targets = []
    for i, c in enumerate(views):                       # ground truth = the render of a perturbed copy of the scene (as bench.py makes it)
        g = torch.Generator(device="cpu").manual_seed(i)
        xyz0 = pc._xyz.data.clone()
        pc._xyz.data.add_(0.01 * torch.randn(xyz0.shape, generator=g).to(dev))
        with torch.no_grad():
            pkg = render(c, pc, pipe, bg, stage="fine", render_feat=hyper.feat_head)
        pc._xyz.data.copy_(xyz0)
        raster_C.invalidate_geometry_cache()
        targets.append((pkg["render"].clamp(0, 1).clone(), pkg["depth"].clone(),
                        pkg["feat"].clone() if hyper.feat_head else torch.zeros_like(pkg["render"])))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def on_route(fused, fn):
        if fused:
            return timed(fn)
        net._fused_heads_ok = lambda: False
        try:
            return timed(fn)
        finally:
            del net._fused_heads_ok

    times = {"step fused": [], "step library": [], "render fused": [], "render library": []}
    seen = {}
    for i in range(args.warmup + args.steps):
        for fused in (True, False):
            v = i % len(views)

            def step():
                _, pkg = training_step(pc, views[v], *targets[v], hyper, opt, bg, pipe=pipe, densify_stats=True)
                seen[fused] = "plane_reg" in pkg
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
    lines = [f"{name}"]
    for k in times:
        lines.append(f"  {k:<15} ms: median {med[k]:8.3f}  min {min(times[k]):8.3f}  max {max(times[k]):8.3f}   ({len(times[k])} samples)")
    ratios = (med["step library"] / med["step fused"], med["render library"] / med["render fused"])
    lines.append(f"  library / fused (medians): training step {ratios[0]:.2f} x, render {ratios[1]:.2f} x")
    return lines, ratios


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=P)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "heads_ab.txt"))
    args = ap.parse_args()
    if args.steps < 20:
        raise SystemExit("heads_ab.py reports medians of at least 20 steps per route")
    if not torch.cuda.is_available():
        raise SystemExit("heads_ab.py measures on the GPU; there is none here (nothing measured)")
    from s3gaussian_amd import synth
    dev = torch.device("cuda:0")
    sc = synth.street_scene(P=args.points, seed=0, width=W, height=H, n_frames=4)
    lines = [f"# tools/heads_ab.py --steps {args.steps} --warmup {args.warmup}: {args.points} Gaussians, {H} x {W}, stage fine; one model per configuration,",
             f"# routes alternated step by step, synchronised wall clock, medians.  {torch.cuda.get_device_name(0)}"]
    worst = float("inf")
    for name, over in CONFIGS:
        block, ratios = measure(name, over, sc, args, dev)
        lines += block
        worst = min(worst, *ratios)
        torch.cuda.empty_cache()
    lines.append(f"# smallest library / fused ratio of the six pairs: {worst:.2f} x ({'fused never slower' if worst >= 1.0 else 'FUSED SLOWER SOMEWHERE'})")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")
    return 0 if worst >= 1.0 else 1


if __name__ == "__main__":
    sys.exit(main())
