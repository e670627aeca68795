"""GPU: pose refinement in the multi-view step -- PoseRefiner.corrected_views, pipeline.render_views / training_step_views(pose=).

  * batched pose kernels (s3g_pose_apply_views / _backward_views): corrected_views equals V corrected() calls bit for bit --
    view, proj, campos, and after a backward with random upstream gradients delta.grad; V = 1, 3, 8, 9 (not capped at the glue's 8),
    non-zero corrections on both sides of the series switch at theta^2 = 1e-4, rows that no view names exact zeros.
  * route: the model of tests/test_pose_route_gpu.py, three cameras at one timestamp and one at another, non-zero delta rows,
    loss = sum_v <render_v, gc_v> + <depth_v, gd_v> + <feat_v, gf_v>: refiner.delta.grad after ONE render_views(pose=, cam_indices=)
    + backward is `torch.equal` to the gradient that one render(pose=, cam_index=) + backward per view accumulates -- shared and
    per-view deformation passes, and the library route (pipe.fused_glue=False).  Equality is the right bar: every view's camera
    sees the same forward values either way, the rasterizer nodes are the same nodes, and the shared glue pass returns each view's
    camera-centre gradient in the single-camera route's bits (tests/test_glue_views_campos_gpu.py).
  * identity: three deterministic-mode training_step_views steps that pass pose=None, cam_indices=None leave every parameter and
    densification accumulator bit-identical to three steps that never name them.
  * descent: frozen Gaussians, ground truth rendered at the true poses of three rig cameras, each camera a known offset of its own
    away (of the size of test_pose_route_gpu.DESCENT_OFFSET); after DESCENT_STEPS refiner-only steps through render_views(pose=) ->
    training_loss_views -> pose.step() the loss and every camera's translation error and rotation angle are below step 0's.
"""
import math
from types import SimpleNamespace

import pytest
import torch

from tests.test_camera_grad_cpu import upstream
from tests.test_pose_route_gpu import DESCENT_LR, DESCENT_STEPS, H, W, _model

pytestmark = pytest.mark.gpu

DESCENT_OFFSETS = ((0.0, 0.0, 0.02, 0.0, 0.0, 0.05), (0.0, 0.0, -0.02, 0.0, 0.0, -0.05), (0.0, 0.0, 0.015, 0.0, 0.0, -0.04))
RIG = ((0.0, 0.0, 0.0, 0.0, 0.0, 0.0), (0.0, 0.06, 0.0, 0.25, 0.0, 0.0), (0.0, -0.06, 0.0, -0.25, 0.0, 0.0), (0.01, 0.02, 0.0, 0.1, -0.1, 0.2))


def _moved(cam, delta6, dev, time=None):
    """A camera of its own (no autograd history): `cam` moved by delta6."""
    from s3gaussian_amd import pose
    with torch.no_grad():
        out = pose.apply_pose_delta(torch.tensor(delta6, dtype=torch.float64, device=dev), cam)
    out = {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in out.items()}
    if time is not None:
        out["time"] = time
    return out


def _deltas(N, dev, seed):
    """[N,6] corrections, all non-zero: even rows below the series switch (|omega| = 3e-3, theta^2 = 9e-6), odd rows above it
    (|omega| = 0.05, theta^2 = 2.5e-3)."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(N, 3, generator=g, dtype=torch.float64)
    w = w / w.norm(dim=1, keepdim=True) * torch.where(torch.arange(N) % 2 == 0, 3e-3, 0.05)[:, None]
    return torch.cat([w, 0.03 * torch.randn(N, 3, generator=g, dtype=torch.float64)], 1).to(dev)


@pytest.mark.parametrize("V", [1, 3, 8, 9])
def test_corrected_views_equals_single_camera_calls(gpu_device, V):
    from s3gaussian_amd import pose
    dev = gpu_device
    _, cam, _, _, _ = _model(dev)
    N = V + 2
    g = torch.Generator().manual_seed(V)
    cams = [_moved(cam, (0.1 * torch.randn(6, generator=g)).tolist(), dev) for _ in range(V)]
    indices = [N - 1 - k for k in range(V)]                     # out of order, rows 0 and 1 unnamed, both parities from V = 2 on
    delta = _deltas(N, dev, 50 + V)
    s = (delta[:, :3] ** 2).sum(1)
    assert bool((s > 0).all()) and (V == 1 or (bool((s[indices] < 1e-4).any()) and bool((s[indices] >= 1e-4).any())))
    ups = [(torch.randn(4, 4, generator=g).to(dev), torch.randn(4, 4, generator=g).to(dev), torch.randn(3, generator=g).to(dev))
           for _ in range(V)]
    loss_of = lambda cs: sum((c["viewmatrix"] * u[0]).sum() + (c["projmatrix"] * u[1]).sum() + (c["campos"] * u[2]).sum()
                             for c, u in zip(cs, ups))
    a, b = pose.PoseRefiner(N, dev, lr=1e-3), pose.PoseRefiner(N, dev, lr=1e-3)
    with torch.no_grad():
        a.delta.copy_(delta)
        b.delta.copy_(delta)
    got = a.corrected_views(cams, indices)
    want = [b.corrected(c, i) for c, i in zip(cams, indices)]
    for x, y, c in zip(got, want, cams):
        for k in ("viewmatrix", "projmatrix", "campos"):
            assert x[k].shape == y[k].shape and torch.equal(x[k], y[k]), k
            assert not torch.equal(x[k], c[k])                  # the correction does move the camera
        assert x["time"] == c["time"] and x["image_width"] == c["image_width"]
    loss_of(got).backward()
    loss_of(want).backward()
    assert torch.equal(a.delta.grad, b.delta.grad)
    named = torch.zeros(N, dtype=torch.bool)
    named[indices] = True
    assert bool((a.delta.grad[named.to(dev)] != 0).all()) and not a.delta.grad[~named.to(dev)].any()


def _rig(dev, seed=21):
    """The route model with three cameras at its timestamp and a fourth at another."""
    pc, cam, hyper, opt, bg = _model(dev, seed=seed)
    t0 = float(cam["time"])
    t1 = t0 + 0.25 if t0 < 0.5 else t0 - 0.25
    cams = [_moved(cam, RIG[k], dev, time=(t0 if k < 3 else t1)) for k in range(4)]
    return pc, cams, hyper, opt, bg


def _route_loss(pkgs, ups):
    return sum((p["render"] * u[0]).sum() + (p["depth"] * u[1]).sum() + (p["feat"] * u[2]).sum() for p, u in zip(pkgs, ups))


@pytest.mark.parametrize("route", ["shared", "per_view", "library"])
def test_render_views_gradient_equals_one_render_per_view(gpu_device, route):
    from s3gaussian_amd import pipeline, pose, raster_C
    dev = gpu_device
    pc, cams, hyper, opt, bg = _rig(dev)
    pipe = SimpleNamespace(**vars(pipeline._default_pipe(None)))
    if route == "library":
        pipe.fused_glue = False
    assert pipeline._glue_route(pc, pipe, "fine") == (route != "library") and hyper.feat_head
    N, indices = 5, [3, 0, 4, 1]
    delta = _deltas(N, dev, 60)
    f = lambda t_: t_.float().to(dev)
    ups = [(f(upstream(40 + v, H, W)[0]), f(upstream(40 + v, H, W)[1]), f(upstream(50 + v, H, W)[0])) for v in range(4)]

    def refiner():
        r = pose.PoseRefiner(N, dev, lr=1e-3)
        with torch.no_grad():
            r.delta.copy_(delta)
        return r

    a = refiner()
    raster_C.invalidate_geometry_cache()
    pkgs = pipeline.render_views(cams, pc, pipe, bg, stage="fine", render_feat=True, share_deformation=(route != "per_view"),
                                 pose=a, cam_indices=indices)
    _route_loss(pkgs, ups).backward()
    model_grads = [p.grad.clone() for p in pc.parameters() if p.grad is not None]
    pc.optimizer.zero_grad(set_to_none=True)

    b = refiner()
    singles = []
    for cam, i, u in zip(cams, indices, ups):
        raster_C.invalidate_geometry_cache()
        pkg = pipeline.render(cam, pc, pipe, bg, stage="fine", render_feat=True, pose=b, cam_index=i)
        singles.append(pkg)
        _route_loss([pkg], [u]).backward()
    pc.optimizer.zero_grad(set_to_none=True)

    for p, q in zip(pkgs, singles):
        assert torch.equal(p["render"], q["render"]) and torch.equal(p["depth"], q["depth"]) and torch.equal(p["feat"], q["feat"])
    ga, gb = a.delta.grad, b.delta.grad
    print(route, "d loss / d delta, rows", indices, ga[indices].cpu().numpy())
    assert torch.equal(ga, gb)
    assert bool(torch.isfinite(ga).all()) and bool((ga[indices] != 0).all()) and not ga[2].any()
    assert len(model_grads) > 4 and all(bool(torch.isfinite(g).all()) for g in model_grads)


def _three_steps_views(dev, name_pose):
    from s3gaussian_amd import hexplane, pipeline, raster_C
    pc, cams, hyper, opt, bg = _rig(dev, seed=22)
    g = torch.Generator().manual_seed(5)
    gts = [torch.rand(3, H, W, generator=g).to(dev) for _ in cams]
    gtd = [(torch.rand(1, H, W, generator=g) * 6).to(dev) for _ in cams]
    gtf = [torch.rand(3, H, W, generator=g).to(dev) for _ in cams]
    raster_C.invalidate_geometry_cache()
    extra = dict(pose=None, cam_indices=None) if name_pose else {}
    prev = hexplane.set_deterministic(True)
    try:
        for _ in range(3):
            pipeline.training_step_views(pc, cams, gts, gtd, gtf, hyper, opt, bg, densify_stats=True, **extra)
        torch.cuda.synchronize()
    finally:
        hexplane.set_deterministic(prev)
    return [p.detach().clone() for p in pc.parameters()] + [pc.xyz_gradient_accum.clone(), pc.denom.clone(), pc.max_radii2D.clone()]


def test_training_step_views_without_a_refiner_is_unchanged(gpu_device):
    a = _three_steps_views(gpu_device, False)
    b = _three_steps_views(gpu_device, True)
    assert len(a) == len(b) > 8
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert bool(a[-2].any())                                    # the statistics did move


def descent_trajectories_views(dev):
    from s3gaussian_amd import pipeline, pose
    pc, cams, hyper, opt, bg = _rig(dev, seed=23)
    true = cams[:3]                                             # the three cameras of one timestamp
    V = len(true)
    pipe = pipeline._default_pipe(None)
    with torch.no_grad():
        gt = pipeline.render_views(true, pc, pipe, bg, stage="fine", render_feat=True)
        gts, gtd, gtf = [p["render"].clone() for p in gt], [p["depth"].clone() for p in gt], [p["feat"].clone() for p in gt]
    off = [_moved(c, o, dev) for c, o in zip(true, DESCENT_OFFSETS)]
    refiner = pose.PoseRefiner(V, dev, lr=DESCENT_LR)
    sup = pipeline._supervised_feat_views(V, hyper, "fine", "last")
    traj = dict(loss=[], translation=[[] for _ in range(V)], rotation=[[] for _ in range(V)])
    for step in range(DESCENT_STEPS + 1):
        with torch.no_grad():
            M = refiner.poses(off).double().cpu()
        for v in range(V):
            E = M[v] @ torch.linalg.inv(true[v]["viewmatrix"].t().double().cpu())
            cosang = float(((E[0, 0] + E[1, 1] + E[2, 2]) - 1.0) / 2.0)
            traj["translation"][v].append(float(E[:3, 3].norm()))
            traj["rotation"][v].append(math.acos(max(-1.0, min(1.0, cosang))))
        pkgs = pipeline.render_views(off, pc, pipe, bg, stage="fine", render_feat=sup, pose=refiner, cam_indices=list(range(V)))
        loss = pipeline.training_loss_views(pc, pkgs, gts, gtd, gtf, hyper, opt, "fine")
        traj["loss"].append(float(loss.detach()))
        if step == DESCENT_STEPS:
            break
        loss.backward()
        pc.optimizer.zero_grad(set_to_none=True)                # the Gaussians are frozen: only the refiner steps
        refiner.step()
    return traj


def test_refiner_descends_three_rig_cameras_from_known_offsets(gpu_device):
    traj = descent_trajectories_views(gpu_device)
    print("descent (views): loss", traj["loss"][0], traj["loss"][-1],
          "translation", [(t[0], t[-1]) for t in traj["translation"]], "rotation", [(r[0], r[-1]) for r in traj["rotation"]])
    assert math.isfinite(traj["loss"][-1]) and traj["loss"][-1] < traj["loss"][0]
    for v, o in enumerate(DESCENT_OFFSETS):
        assert abs(traj["rotation"][v][0] - abs(o[2])) < 1e-4 and abs(traj["translation"][v][0] - abs(o[5])) < 1e-3
        for k in ("translation", "rotation"):
            assert math.isfinite(traj[k][v][-1]) and traj[k][v][-1] < traj[k][v][0], (k, v, traj[k][v][0], traj[k][v][-1])
