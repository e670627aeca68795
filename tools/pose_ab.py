#!/usr/bin/env python
"""Camera pose refinement: what a refiner adds to a training step, on the route built for it and on the only route the parent
commit allows.

Workload: one scene from synth.street_scene at the benchmark shape (1.2 M Gaussians, 1066 x 1600, fine stage, default heads).

  a  plain    pipeline.training_step without a refiner: the parent's step.
  b  pose     the same call with pose=PoseRefiner, cam_index=: s3g_pose_apply in front, the two-image rasterizer node and the glue
              return the camera gradients (s3g_camera_backward, twice: node and glue), s3g_pose_apply_backward, torch's Adam on
              the [N,6] float64 parameter.
  c  scene    the parent has no gradient for the camera, so the scene is moved instead, in torch ops under autograd: Rodrigues'
              formula on a six-vector, means3D transformed by the move that is equivalent to the camera's, cov3D_precomp built in
              torch from scales and rotations and rotated, handed to the two-image node in place of the (scale, rotation) pair.
              (The colours keep the uncorrected camera centre: the parent's glue returns nothing for it.)

    python tools/pose_ab.py [--steps 20] [--warmup 3] [--only a|b|c] [--out profiles/pose_ab.txt]

One model, one process: after the warm-up the routes alternate step by step; a device synchronise on both sides of every timed
step, wall clock, medians of at least 20.  --only runs one route alone (for a kernel trace: profiles/pose_kstats.txt).  A record,
not a gate; the learning rate is a placeholder (nobody has measured a good one) and does not enter the timing."""
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


def rodrigues(w):
    s = (w * w).sum()
    th = torch.sqrt(s + 1e-24)
    A, B = torch.sin(th) / th, (1.0 - torch.cos(th)) / (s + 1e-24)
    z = torch.zeros((), dtype=w.dtype, device=w.device)
    K = torch.stack([torch.stack([z, -w[2], w[1]]), torch.stack([w[2], z, -w[0]]), torch.stack([-w[1], w[0], z])])
    return torch.eye(3, dtype=w.dtype, device=w.device) + A * K + B * (K @ K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=P)
    ap.add_argument("--only", choices=("a", "b", "c"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_ab.txt"))
    args = ap.parse_args()
    if args.steps < 20 and args.only is None:
        raise SystemExit("pose_ab.py reports medians of at least 20 steps per route")
    if not torch.cuda.is_available():
        raise SystemExit("pose_ab.py measures on the GPU; there is none here (nothing measured)")
    import bench
    from s3gaussian_amd import pose, synth
    from s3gaussian_amd.pipeline import (GaussianParams, covariance_from_scaling_rotation, default_hyper, default_opt, render,
                                         training_loss, training_step)
    from s3gaussian_amd.rasterizer import GaussianRasterizer
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
    by_time = {}
    for c in cams:
        by_time.setdefault(float(c["time"]), c)
    views = list(by_time.values())
    targets = [bench.make_targets(pc, c, bg, hyper, seed=i) for i, c in enumerate(views)]
    refiner = pose.PoseRefiner(len(views), dev, lr=LR)
    scene_delta = torch.nn.Parameter(torch.zeros((len(views), 6), dtype=torch.float32, device=dev))
    scene_opt = torch.optim.Adam([scene_delta], lr=LR)
    pair = GaussianRasterizer.forward_pair
    current = {}

    def pair_on_moved_scene(self, means3D, means2D, opacities, colors_a, colors_b, scales=None, rotations=None, cov3D_precomp=None,
                            densify_accum=None):
        d = scene_delta[current["v"]]
        view = self.raster_settings.viewmatrix
        Rc, tc = view[:3, :3].t(), view[3, :3]                    # x_cam = Rc x + tc
        E = rodrigues(d[:3])
        M = Rc.t() @ E @ Rc                                         # the move of the scene equivalent to the camera's
        moved = means3D @ M.t() + (Rc.t() @ (E @ tc + d[3:] - tc))
        cov = covariance_from_scaling_rotation(scales, self.raster_settings.scale_modifier, rotations)
        full = torch.stack([cov[:, 0], cov[:, 1], cov[:, 2], cov[:, 1], cov[:, 3], cov[:, 4], cov[:, 2], cov[:, 4], cov[:, 5]], 1).view(-1, 3, 3)
        rot = M @ full @ M.t()
        cov6 = torch.stack([rot[:, 0, 0], rot[:, 0, 1], rot[:, 0, 2], rot[:, 1, 1], rot[:, 1, 2], rot[:, 2, 2]], 1)
        return pair(self, means3D=moved, means2D=means2D, opacities=opacities, colors_a=colors_a, colors_b=colors_b,
                    cov3D_precomp=cov6, densify_accum=densify_accum)

    def step_a(v):
        training_step(pc, views[v], *targets[v], hyper, opt, bg, pipe=pipe, densify_stats=True)

    def step_b(v):
        training_step(pc, views[v], *targets[v], hyper, opt, bg, pipe=pipe, densify_stats=True, pose=refiner, cam_index=v)

    def step_c(v):
        current["v"] = v
        GaussianRasterizer.forward_pair = pair_on_moved_scene
        try:
            pkg = render(views[v], pc, pipe, bg, stage="fine", return_dx=True, render_feat=True,
                         densify_accum=(pc.xyz_gradient_accum, pc.denom, pc.max_radii2D))
        finally:
            GaussianRasterizer.forward_pair = pair
        loss = training_loss(pc, pkg, *targets[v], hyper, opt, "fine")
        loss.backward()
        pc.optimizer.step()
        pc.optimizer.zero_grad(set_to_none=True)
        scene_opt.step()
        scene_opt.zero_grad(set_to_none=True)

    routes = {"a": ("a plain", step_a), "b": ("b pose", step_b), "c": ("c scene", step_c)}
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
    lines = [f"# tools/pose_ab.py --steps {args.steps} --warmup {args.warmup}: {args.points} Gaussians, {H} x {W}, stage fine;",
             f"# one model, routes alternated step by step, synchronised wall clock, medians.  {torch.cuda.get_device_name(0)}"]
    for k in times:
        lines.append(f"  step {k:<8} ms: median {med[k]:8.3f}  min {min(times[k]):8.3f}  max {max(times[k]):8.3f}   ({len(times[k])} samples)")
    if len(med) == 3:
        lines.append(f"  b - a = {med['b pose'] - med['a plain']:.3f} ms, c - a = {med['c scene'] - med['a plain']:.3f} ms (medians)")
    text = "\n".join(lines) + "\n"
    if args.only is None:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
