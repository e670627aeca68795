#!/usr/bin/env python
"""A batch of the three cameras of one timestamp, three ways.  The deformation field depends on (xyz, t) only: a rig's cameras of
one frame can share its evaluation, the glue's read of the SH block and the Adam step.

Workload: synth.street_scene at the benchmark shape (1.2 M Gaussians, 1066 x 1600, fine stage, default heads).

  (a) three steps   three pipeline.training_step calls on the three cameras of a timestamp -- the only way before
                    training_step_views: three deformation passes, three glue passes, THREE Adam steps, three feature images
  (b) unshared      training_step_views(share_deformation=False): the reference's batch semantics (one loss, one backward, ONE Adam
                    step, the last view's feature image only), the field still evaluated once per view
  (c) shared        training_step_views: the same step with one deformation pass and one glue pass per timestamp

    python tools/rig_step_ab.py [--steps 20] [--warmup 3] [--out profiles/rig_step_ab.txt] [--trace-run]

One model, one process: after the warm-up the routes alternate batch by batch, cycling through the timestamps; a device synchronise
on both sides of every timed block, wall clock, medians (as tools/geometry_ab.py).  --trace-run runs the warm-up (shared steps), then ONE
(a) batch and ONE (c) batch and times nothing: the run to put under `rocprofv3 --kernel-trace --stats` (tools/kstats.py), where the
glue_*_views kernels then stand beside the three single-camera glue launches of the (a) batch.  A record, not a gate: (c) takes one optimizer step where (a)
takes three, and what that does to PSNR per wall-clock hour is NOT measured here."""
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
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rig_step_ab.txt"))
    args = ap.parse_args()
    if args.steps < 20 and not args.trace_run:
        raise SystemExit("rig_step_ab.py reports medians of at least 20 batches per route")
    if not torch.cuda.is_available():
        raise SystemExit("rig_step_ab.py measures on the GPU; there is none here (nothing measured)")
    import bench
    from s3gaussian_amd import deformation, synth
    from s3gaussian_amd.pipeline import GaussianParams, default_hyper, default_opt, rig_batches, training_step, training_step_views
    dev = torch.device("cuda:0")
    sc = synth.street_scene(P=args.points, seed=0, width=W, height=H, n_frames=4)
    hyper, opt = default_hyper(), default_opt()
    torch.manual_seed(0)
    pc = GaussianParams(sc["sh_degree"], hyper)
    gs = sc["gaussians"]
    pc.init_from_tensors(gs["xyz"], gs["log_scales"], gs["rotations_raw"], gs["opacity_logit"], gs["shs"], dev)
    pc._deformation.deformation_net.set_aabb(*sc["aabb"])
    pc.training_setup(opt)
    cams = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in c.items()} for c in sc["cameras"]]
    bg = sc["bg"].to(dev)
    pipe = SimpleNamespace(convert_SHs_python=True, compute_cov3D_python=False, debug=False)
    batches = [b for b in rig_batches(cams, 3) if len(b) == 3]
    targets = [bench.make_targets(pc, c, bg, hyper, seed=i) for i, c in enumerate(cams)]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def three_steps(b):
        for v in b:
            training_step(pc, cams[v], *targets[v], hyper, opt, bg, pipe=pipe, densify_stats=True)

    def batch_step(b, share):
        training_step_views(pc, [cams[v] for v in b], [targets[v][0] for v in b], [targets[v][1] for v in b],
                            [targets[v][2] for v in b], hyper, opt, bg, pipe=pipe, densify_stats=True, share_deformation=share)

    routes = {"(a) three steps": three_steps, "(b) unshared": lambda b: batch_step(b, False), "(c) shared": lambda b: batch_step(b, True)}
    if args.trace_run:
        for i in range(args.warmup):
            batch_step(batches[i % len(batches)], True)
        torch.cuda.synchronize()
        three_steps(batches[args.warmup % len(batches)])
        torch.cuda.synchronize()
        batch_step(batches[args.warmup % len(batches)], True)
        torch.cuda.synchronize()
        return
    times = {k: [] for k in routes}
    evals = {}
    for i in range(args.warmup + args.steps):
        b = batches[i % len(batches)]
        for k, fn in routes.items():
            n0 = deformation.heads_evaluations
            ms = timed(lambda: fn(b))
            evals[k] = deformation.heads_evaluations - n0
            if i >= args.warmup:
                times[k].append(ms)
    assert evals == {"(a) three steps": 3, "(b) unshared": 3, "(c) shared": 1}, evals     # the routes really are three routes
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = [f"# tools/rig_step_ab.py --steps {args.steps} --warmup {args.warmup}: the 3 cameras of one timestamp, {args.points} Gaussians, {H} x {W},",
             f"# stage fine, default heads; one model, routes alternated batch by batch, synchronised wall clock, medians.  {torch.cuda.get_device_name(0)}",
             "# deformation passes per batch: (a) 3, (b) 3, (c) 1.  Adam steps per batch: (a) 3, (b) 1, (c) 1.  Feature images: (a) 3, (b) 1, (c) 1."]
    for k in times:
        lines.append(f"  {k:<16} ms per batch: median {med[k]:8.3f}  min {min(times[k]):8.3f}  max {max(times[k]):8.3f}   "
                     f"per view {med[k] / 3:7.3f}   ({len(times[k])} samples)")
    a, b_, c = (med[k] for k in routes)
    lines.append(f"  (c) / (a) = {c / a:.3f}, (c) / (b) = {c / b_:.3f}, (b) / (a) = {b_ / a:.3f}  (medians, per batch of three views)")
    lines.append("# (c) takes ONE optimizer step where (a) takes three; its effect on PSNR per wall-clock hour is NOT measured here.")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
