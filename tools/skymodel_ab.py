#!/usr/bin/env python
"""Sky colour model: what it adds to a training step and to a render, on the device route and on the only route the parent commit
allows.

Workload: one scene from synth.street_scene at the benchmark shape (1.2 M Gaussians, 1066 x 1600, fine stage, default heads).

  a  plain    pipeline.training_step / a no_grad render without a sky model.
  b  device   the same calls with sky_model= (skymodel.sky_composite: s3g_sky_pack, s3g_sky_forward, s3g_sky_backward); the camera
              dict carries "viewmatrix_host", so nothing is read back from the device.  The read-back a dict without it costs is
              timed on its own: skymodel._host_camera on an idle device, median of 20.
  c  torch    render(return_alpha=True) over black, then the restatement's torch ops on the GPU under autograd (directions,
              encoding, three linear layers, sigmoid, composite), the loss on the composite, torch's backward; the model's
              parameters are in pc.optimizer in both b and c.

    python tools/skymodel_ab.py [--steps 20] [--warmup 3] [--only a|b|c] [--out profiles/skymodel_ab.txt]

One model, one process: after the warm-up the routes alternate step by step; a device synchronise on both sides of every timed
step, wall clock, medians of at least 20.  --only runs one route alone (for a kernel trace: profiles/skymodel_kstats.txt).  A
record, not a gate."""
import argparse
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

P, W, H = 1_200_000, 1600, 1066
FWD_FLOP = 2 * (33 * 256 + 289 * 256 + 256 * 3)      # per pixel


def torch_sky(model, cam, dev):
    """The restatement (tests/skymodel_ref.py) in float32 torch ops on the device."""
    from s3gaussian_amd import skymodel
    R, fx, fy, cx, cy = skymodel.camera_intrinsics(cam)
    Hh, Ww = cam["image_height"], cam["image_width"]
    x = torch.arange(Ww, device=dev, dtype=torch.float32).repeat(Hh)
    y = torch.arange(Hh, device=dev, dtype=torch.float32).repeat_interleave(Ww)
    d_cam = torch.stack([(x - cx + 0.5) / fx, (y - cy + 0.5) / fy, torch.ones_like(x)], dim=-1)
    d = d_cam @ R.to(dev).float().T
    v = d / (torch.linalg.norm(d, dim=-1, keepdim=True) + 1e-8)
    scales = torch.tensor([1.0, 2.0, 4.0, 8.0, 16.0], device=dev)
    xb = (v[:, None, :] * scales[:, None]).reshape(-1, 15)
    e = torch.cat([v, torch.sin(torch.cat([xb, xb + 0.5 * math.pi], dim=-1))], dim=-1)
    W0, b0, W1, b1, W2, b2 = model.tensors()
    h0 = torch.relu(e @ W0.T + b0)
    h1 = torch.relu(torch.cat([h0, e], dim=-1) @ W1.T + b1)
    return torch.sigmoid(h1 @ W2.T + b2).T.reshape(3, Hh, Ww)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=P)
    ap.add_argument("--only", choices=("a", "b", "c"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skymodel_ab.txt"))
    args = ap.parse_args()
    if args.steps < 20 and args.only is None:
        raise SystemExit("skymodel_ab.py reports medians of at least 20 steps per route")
    if not torch.cuda.is_available():
        raise SystemExit("skymodel_ab.py measures on the GPU; there is none here (nothing measured)")
    from s3gaussian_amd import skymodel, synth
    from s3gaussian_amd.pipeline import (GaussianParams, _finish_step, default_hyper, default_opt, render, training_loss, training_step)
    dev = torch.device("cuda:0")
    scn = synth.street_scene(P=args.points, seed=0, width=W, height=H, n_frames=2)
    hyper, opt = default_hyper(), default_opt()
    pc = GaussianParams(3, hyper)
    gs = scn["gaussians"]
    pc.init_from_tensors(gs["xyz"], gs["log_scales"], gs["rotations_raw"], gs["opacity_logit"], gs["shs"], dev)
    pc._deformation.deformation_net.set_aabb(*scn["aabb"])
    pc.training_setup(opt)
    torch.manual_seed(0)
    model = pc.attach_sky_model(skymodel.SkyModel())
    cam = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in scn["cameras"][0].items()}
    cam_dev = dict(cam)                                    # the rotation on the device only
    cam["viewmatrix_host"] = scn["cameras"][0]["viewmatrix"].clone()
    from types import SimpleNamespace
    pipe = SimpleNamespace(convert_SHs_python=True, compute_cov3D_python=False, debug=False)
    gt, gtd, gtf = torch.rand(3, H, W, device=dev), torch.rand(1, H, W, device=dev) * 50, torch.rand(3, H, W, device=dev)
    bg = torch.zeros(3, device=dev)

    def step_torch():
        pkg = render(cam, pc, pipe, bg, stage="fine", return_dx=True, render_feat=True, return_alpha=True)
        pkg["render"] = pkg["render"] + (1.0 - pkg["alpha"]) * torch_sky(model, cam, dev)
        training_loss(pc, pkg, gt, gtd, gtf, hyper, opt, "fine").backward()
        _finish_step(pc, pkg, None, None)

    def render_torch():
        with torch.no_grad():
            pkg = render(cam, pc, pipe, bg, return_alpha=True)
            return pkg["render"] + (1.0 - pkg["alpha"]) * torch_sky(model, cam, dev)

    def render_with(**kw):
        with torch.no_grad():
            return render(cam, pc, pipe, bg, **kw)["render"]

    routes = {
        "a": ("plain", lambda: training_step(pc, cam, gt, gtd, gtf, hyper, opt, bg), lambda: render_with()),
        "b": ("device", lambda: training_step(pc, cam, gt, gtd, gtf, hyper, opt, bg, sky_model=model), lambda: render_with(sky_model=model)),
        "c": ("torch", step_torch, render_torch),
    }
    keys = [args.only] if args.only else list(routes)
    times = {(k, what): [] for k in keys for what in ("step", "render")}
    for it in range(args.warmup + args.steps):
        for k in keys:
            for what, fn in (("step", routes[k][1]), ("render", routes[k][2])):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if it >= args.warmup:
                    times[(k, what)].append((time.perf_counter() - t0) * 1e3)
    med = {kw: statistics.median(v) for kw, v in times.items()}
    lines = [f"sky colour model A/B: {args.points} Gaussians, {H} x {W}, fine stage; medians of {args.steps} (ms), routes alternated in one process",
             f"forward arithmetic of the model: {FWD_FLOP * H * W / 1e12:.3f} TFLOP per frame"]
    for k in keys:
        lines.append(f"  {k} {routes[k][0]:7s} training_step {med[(k, 'step')]:8.3f}   no_grad render {med[(k, 'render')]:8.3f}")
    if "a" in keys:
        for k in keys:
            if k != "a":
                lines.append(f"  {routes[k][0]} adds {med[(k, 'step')] - med[('a', 'step')]:.3f} ms per training step, "
                             f"{med[(k, 'render')] - med[('a', 'render')]:.3f} ms per render")
    if args.only is None:
        back = []
        for _ in range(20):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            skymodel._host_camera(cam_dev)
            back.append((time.perf_counter() - t0) * 1e3)
        lines.append(f"  camera read-back without viewmatrix_host (idle device): {statistics.median(back):.3f} ms per call, plus the wait for "
                     "whatever the stream still holds")
    text = "\n".join(lines)
    print(text)
    if args.only is None:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
