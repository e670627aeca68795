#!/usr/bin/env python
"""Pose refinement of the three cameras of one timestamp, on the route the parent commit allows and on the multi-view step.

Workload: synth.street_scene at the benchmark shape (1.2 M Gaussians, 1066 x 1600, fine stage, default heads), the three cameras
of one timestamp as pipeline.rig_batches hands them out, a pose.PoseRefiner with one row per camera.

  (i)   three steps    three pipeline.training_step(pose=, cam_index=) calls: the only route with a refiner before
                       training_step_views took one -- three deformation passes, three glue passes, three Adam steps of the model and
                       three of the refiner
  (ii)  views + pose   training_step_views(pose=, cam_indices=): one deformation pass, one glue pass that also returns the three
                       camera-centre gradients (s3g_glue_backward_views_campos), one s3g_pose_apply_views launch each way, one Adam
                       step each
  (iii) views          training_step_views without a refiner: what (ii) adds to

    python tools/pose_views_ab.py [--steps 20] [--warmup 3] [--only i|ii|iii] [--out profiles/pose_views_ab.txt]

One model, one process: after the warm-up the routes alternate batch by batch, cycling through the timestamps; a device synchronise
on both sides of every timed block, wall clock, medians of at least 20 (as tools/rig_step_ab.py, tools/pose_ab.py).  --only runs
one route alone and writes no record: the run to put under `rocprofv3 --kernel-trace --stats` (tools/kstats.py ->
profiles/pose_views_kstats.txt).  A record, not a gate: (ii) takes one optimizer step where (i) takes three,
and the learning rate is a placeholder that does not enter the timing."""
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
LR = 1e-5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=P)
    ap.add_argument("--only", choices=("i", "ii", "iii"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_views_ab.txt"))
    args = ap.parse_args()
    if args.steps < 20 and args.only is None:
        raise SystemExit("pose_views_ab.py reports medians of at least 20 batches per route")
    if not torch.cuda.is_available():
        raise SystemExit("pose_views_ab.py measures on the GPU; there is none here (nothing measured)")
    import bench
    from s3gaussian_amd import pose, synth
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
    refiner = pose.PoseRefiner(len(cams), dev, lr=LR)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def three_steps(b):
        for v in b:
            training_step(pc, cams[v], *targets[v], hyper, opt, bg, pipe=pipe, densify_stats=True, pose=refiner, cam_index=v)

    def batch_step(b, with_pose):
        training_step_views(pc, [cams[v] for v in b], [targets[v][0] for v in b], [targets[v][1] for v in b],
                            [targets[v][2] for v in b], hyper, opt, bg, pipe=pipe, densify_stats=True,
                            **({"pose": refiner, "cam_indices": list(b)} if with_pose else {}))

    routes = {"(i) three steps": three_steps, "(ii) views + pose": lambda b: batch_step(b, True),
              "(iii) views": lambda b: batch_step(b, False)}
    if args.only:
        routes = {k: fn for k, fn in routes.items() if k.startswith(f"({args.only})")}
    times = {k: [] for k in routes}
    for i in range(args.warmup + args.steps):
        b = batches[i % len(batches)]
        for k, fn in routes.items():
            ms = timed(lambda: fn(b))
            if i >= args.warmup:
                times[k].append(ms)
    assert bool(torch.isfinite(refiner.delta).all())
    assert args.only == "iii" or bool(refiner.delta.detach().any())     # the refiner did step
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = [f"# tools/pose_views_ab.py --steps {args.steps} --warmup {args.warmup}: the 3 cameras of one timestamp, {args.points} Gaussians, "
             f"{H} x {W},",
             f"# stage fine, default heads, a PoseRefiner row per camera; one model, routes alternated batch by batch, synchronised wall "
             f"clock, medians.  {torch.cuda.get_device_name(0)}",
             "# Adam steps per batch (model / refiner): (i) 3 / 3, (ii) 1 / 1, (iii) 1 / 0.  Deformation and glue passes: (i) 3, (ii) 1, (iii) 1."]
    for k in times:
        lines.append(f"  {k:<18} ms per batch: median {med[k]:8.3f}  min {min(times[k]):8.3f}  max {max(times[k]):8.3f}   "
                     f"per view {med[k] / 3:7.3f}   ({len(times[k])} samples)")
    if args.only is None:
        a, b_, c = (med[k] for k in routes)
        lines.append(f"  (ii) / (i) = {b_ / a:.3f}, (ii) - (iii) = {b_ - c:.3f} ms per batch: what the refiner adds to the multi-view step  (medians)")
        lines.append("# (ii) takes ONE optimizer step where (i) takes three; its effect on pose error per wall-clock hour is NOT measured here.")
    text = "\n".join(lines) + "\n"
    if args.only is None:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
