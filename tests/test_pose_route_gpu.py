"""GPU: pose refinement through the whole route -- pose.PoseRefiner -> pipeline.render / training_step / evaluate.

  * d loss / d delta of pipeline.render(..., pose=) on the glue route, fine stage, default heads, against float64 autograd of the
    composition pose_map_ref -> (SH colours of the glue, torch_ref.rasterize for the RGB + depth and the feature image) on the
    render's own per-Gaussian inputs.  Bar: as tests/test_camera_grad_gpu.py, pushed through the pose map -- the error of
    component k relative to sum_j |J_jk| sum|term_j| is at most 4 x the relative error of the same backward's means3D gradient
    against the same autograd.
  * training_step(pose=None) is the step it was: the parameters after 3 steps equal, bit for bit, those recorded from the parent
    commit (tests/golden/pose_parent_three_steps.json) and those of 3 steps that never name `pose`; pipeline does not import the
    module.
  * descent: 500 frozen Gaussians at 64 x 48, ground truth rendered at the true pose, the refiner's camera a small known offset
    away; after 50 refiner-only steps the loss, the translation error and the rotation angle are each smaller than at step 0.
  * state_dict round trip; evaluate(..., pose=) equals evaluate at the corrected cameras.
"""
import math

import numpy as np
import pytest
import torch

from tests.pose_ref import camera_terms_ref, pose_map_ref  # noqa: F401
from tests.test_camera_grad_cpu import camera_scene, upstream
from tests.test_camera_grad_gpu import _library_backward, _restatement
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

W, H, P = 64, 48, 500
DESCENT_LR = 1e-4
DESCENT_OFFSET = (0.0, 0.0, 0.02, 0.0, 0.0, 0.05)       # a roll and a step along the optical axis
DESCENT_STEPS = 50


def _model(dev, seed=21):
    """500 Gaussians in front of one camera, as a GaussianParams on the default (fused, glue) route."""
    from s3gaussian_amd.pipeline import GaussianParams, default_hyper, default_opt
    s = camera_scene(seed, P=P, W=W, H=H, scale=0.25, spread=2.4, zmin=2.5, zmax=7.0)
    hyper, opt = default_hyper(), default_opt()
    torch.manual_seed(seed)
    pc = GaussianParams(3, hyper)
    pc.init_from_tensors(s["means3D"], torch.log(s["scales"]), s["rotations"], torch.logit(s["opacities"].clamp(0.02, 0.98)), s["shs"], dev)
    lo, hi = s["means3D"].min(0)[0] - 1.0, s["means3D"].max(0)[0] + 1.0
    pc._deformation.deformation_net.set_aabb(hi.tolist(), lo.tolist())
    pc.training_setup(opt)
    cam = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in s["cam"].items()}
    return pc, cam, hyper, opt, s["bg"].to(dev)


def test_gradient_through_the_whole_route(gpu_device):
    from oracle import torch_ref
    from s3gaussian_amd import pipeline, pose, raster_C
    from s3gaussian_amd.glue import activations_and_colors
    dev = gpu_device
    pc, cam, hyper, opt, bg = _model(dev)
    assert hyper.feat_head and pipeline._glue_route(pc, pipeline._default_pipe(None), "fine")
    pipe = pipeline._default_pipe(None)
    refiner = pose.PoseRefiner(3, dev, lr=1e-3)
    delta0 = torch.tensor([0.011, -0.007, 0.013, 0.02, -0.015, 0.03], dtype=torch.float64)
    with torch.no_grad():
        refiner.delta[1] = delta0.to(dev)
    gc, gd = upstream(31, H, W)
    gf, _ = upstream(32, H, W)
    f = lambda t_: t_.float().to(dev)
    raster_C.invalidate_geometry_cache()
    pkg = pipeline.render(cam, pc, pipe, bg, stage="fine", render_feat=True, pose=refiner, cam_index=1)
    loss = (pkg["render"] * f(gc)).sum() + (pkg["depth"] * f(gd)).sum() + (pkg["feat"] * f(gf)).sum()
    loss.backward()
    got = refiner.delta.grad[1].cpu()
    assert not refiner.delta.grad[0].any() and not refiner.delta.grad[2].any() and bool(torch.isfinite(got).all())

    # the render's own per-Gaussian inputs, from the same kernels (under autograd, as the render ran them)
    cam_c = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in refiner.corrected(cam, 1).items()}
    xyz = pc.get_xyz.detach().clone().requires_grad_(True)
    m3f, sc_raw, rot_raw, op_raw, dx, dshs, feat, _ = pipeline._deform_fused(pc, cam["time"], "fine", True, False)
    colors, sc_f, rot_f, op_f = activations_and_colors(pc.active_sh_degree, pc._features_dc, pc._features_rest, dshs, xyz, cam_c["campos"],
                                                       sc_raw, rot_raw, op_raw)
    det = lambda t_: t_.detach().contiguous()
    s = dict(means3D=det(m3f).cpu(), opacities=det(op_f).cpu(), scales=det(sc_f).cpu(), rotations=det(rot_f).cpu(),
             colors_precomp=det(colors).cpu(), bg=bg.cpu(), cam={k: (v.cpu() if torch.is_tensor(v) else v) for k, v in cam_c.items()})
    s["cam"]["tanfovx"], s["cam"]["tanfovy"] = float(np.float32(cam["tanfovx"])), float(np.float32(cam["tanfovy"]))
    b = _library_backward(s, "precomp", dev, gc, gd, colors2=det(feat), gc2=gf)
    colors.backward(b["g_col"])                               # the glue's direction term: g_dir of the camera kernel
    g_dir = xyz.grad
    _, abs_sums = _restatement(b, g_dir=g_dir)

    # float64 truth: pose map -> camera (at the fp32 values the render used, straight-through) -> colours -> two rasterizations
    d64 = lambda t_: t_.detach().double().cpu()
    delta = delta0.clone().requires_grad_(True)
    view, proj, campos = pose_map_ref(delta, cam["viewmatrix"].cpu(), cam["projmatrix"].cpu())
    J = torch.stack([torch.autograd.grad(o, delta, retain_graph=True)[0] for o in torch.cat([view.reshape(-1), proj.reshape(-1), campos])])
    st = lambda v64, v32: v64 + (d64(v32) - v64).detach()
    view, proj, campos = st(view, cam_c["viewmatrix"]), st(proj, cam_c["projmatrix"]), st(campos, cam_c["campos"])
    shs = torch.cat([d64(pc._features_dc), d64(pc._features_rest)], 1) + (0 if dshs is None else d64(dshs))
    col64 = torch_ref._sh_color(pc.active_sh_degree, shs, d64(pc.get_xyz), campos)
    m64 = d64(m3f).requires_grad_(True)
    kw = dict(bg=d64(bg), means3D=m64, opacities=d64(op_f), viewmatrix=view, projmatrix=proj, campos=campos, tanfovx=s["cam"]["tanfovx"],
              tanfovy=s["cam"]["tanfovy"], image_height=H, image_width=W, scales=d64(sc_f), rotations=d64(rot_f))
    color, _, depth = torch_ref.rasterize(**kw, colors_precomp=col64)
    featimg, _, _ = torch_ref.rasterize(**kw, colors_precomp=d64(feat))
    loss64 = (color * gc).sum() + (depth * gd).sum() + (featimg * gf).sum()
    want, truth_m3 = torch.autograd.grad(loss64, (delta, m64))
    means3D_rel = rel_l2(b["g_m3"].cpu().numpy(), truth_m3.numpy())
    scale = (J.abs() * torch.from_numpy(abs_sums)[:, None]).sum(0)
    err = ((got - want).abs() / scale).numpy()
    print("route: d loss / d delta", got.numpy(), "truth", want.numpy(), "err / scale", err, "means3D_rel", means3D_rel)
    assert math.isfinite(means3D_rel) and means3D_rel > 0 and float(want.abs().min()) > 0
    assert (err <= 4 * means3D_rel).all(), (err, means3D_rel)


def _three_steps(dev, name_pose):
    from s3gaussian_amd import hexplane, pipeline, raster_C
    pc, cam, hyper, opt, bg = _model(dev, seed=22)
    g = torch.Generator().manual_seed(5)
    gt, gtd, gtf = torch.rand(3, H, W, generator=g).to(dev), (torch.rand(1, H, W, generator=g) * 6).to(dev), torch.rand(3, H, W, generator=g).to(dev)
    raster_C.invalidate_geometry_cache()
    extra = dict(pose=None, cam_index=None) if name_pose else {}
    prev = hexplane.set_deterministic(True)                 # stable walk orders: two runs from one seed are bit-identical
    try:
        for _ in range(3):
            pipeline.training_step(pc, cam, gt, gtd, gtf, hyper, opt, bg, densify_stats=True, **extra)
        torch.cuda.synchronize()
    finally:
        hexplane.set_deterministic(prev)
    return [p.detach().clone() for p in pc.parameters()] + [pc.xyz_gradient_accum.clone(), pc.denom.clone(), pc.max_radii2D.clone()]


PARENT_STEPS = "tests/golden/pose_parent_three_steps.json"


def tensor_hashes(tensors):
    """sha256 of each tensor's bytes, in order."""
    import hashlib
    return [hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest() for t in tensors]


def test_training_step_without_a_refiner_is_the_parents(gpu_device):
    """The parameters, Adam-visible state included through them, and the densification accumulators after 3 deterministic-mode
    steps from one seed equal, bit for bit, what the parent commit (39d9525, before the camera gradients existed) left on an MI355X:
    tests/golden/pose_parent_three_steps.json holds the sha256 of every tensor, recorded by running _three_steps on a build of that
    commit.  Unlike the test below, this one fails for any change of the plain step's arithmetic."""
    import json
    import os
    want = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), PARENT_STEPS)))
    got = tensor_hashes(_three_steps(gpu_device, False))
    assert len(got) == len(want["sha256"]) > 8
    assert got == want["sha256"], [i for i, (x, y) in enumerate(zip(got, want["sha256"])) if x != y]


def test_training_step_without_a_refiner_is_unchanged(gpu_device):
    import s3gaussian_amd.pipeline as pipeline
    assert "pose" not in vars(pipeline)                     # nothing of the feature is loaded until somebody hands a refiner in
    a = _three_steps(gpu_device, False)
    from s3gaussian_amd import pose
    pose.PoseRefiner(1, gpu_device, lr=1e-3)
    b = _three_steps(gpu_device, True)
    assert len(a) == len(b) > 8
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def _pose_errors(refiner, cam_off, cam_true):
    """(translation error, rotation angle) of the corrected camera against the true one, in float64."""
    M = refiner.poses([cam_off])[0].double().cpu()
    Mt = cam_true["viewmatrix"].t().double().cpu()
    E = M @ torch.linalg.inv(Mt)
    cosang = float(((E[0, 0] + E[1, 1] + E[2, 2]) - 1.0) / 2.0)
    return float(E[:3, 3].norm()), math.acos(max(-1.0, min(1.0, cosang)))


def descent_trajectories(dev):
    from s3gaussian_amd import pipeline, pose, raster_C
    pc, cam_true, hyper, opt, bg = _model(dev, seed=23)
    pipe = pipeline._default_pipe(None)
    with torch.no_grad():
        gt = pipeline.render(cam_true, pc, pipe, bg, stage="fine")
        gt_img, gt_depth = gt["render"].clone(), gt["depth"].clone()
        cam_off = {k: (v.detach().clone() if torch.is_tensor(v) else v)
                   for k, v in pose.apply_pose_delta(torch.tensor(DESCENT_OFFSET, dtype=torch.float64, device=dev), cam_true).items()}
    refiner = pose.PoseRefiner(1, dev, lr=DESCENT_LR)
    hits = raster_C._geom_cache_hits
    traj = dict(loss=[], translation=[], rotation=[])
    for step in range(DESCENT_STEPS + 1):
        t_err, r_err = _pose_errors(refiner, cam_off, cam_true)
        pkg = pipeline.render(cam_off, pc, pipe, bg, stage="fine", pose=refiner, cam_index=0)
        loss = (pkg["render"] - gt_img).abs().mean() + 0.1 * (pkg["depth"] - gt_depth).abs().mean()
        traj["loss"].append(float(loss.detach()))
        traj["translation"].append(t_err)
        traj["rotation"].append(r_err)
        if step == DESCENT_STEPS:
            break
        loss.backward()
        pc.optimizer.zero_grad(set_to_none=True)            # the Gaussians are frozen: only the refiner steps
        refiner.step()
    # a fresh corrected matrix each step: the geometry cache (keyed on the camera tensors) never served a stale geometry
    assert raster_C._geom_cache_hits == hits
    return traj


def test_refiner_descends_from_a_known_offset(gpu_device):
    traj = descent_trajectories(gpu_device)
    print("descent:", {k: (v[0], v[-1]) for k, v in traj.items()})
    assert abs(traj["rotation"][0] - 0.02) < 1e-4 and abs(traj["translation"][0] - 0.05) < 1e-3
    for k, v in traj.items():
        assert math.isfinite(v[-1]) and v[-1] < v[0], (k, v[0], v[-1])


def test_state_dict_round_trip_and_evaluate_at_refined_poses(gpu_device):
    from s3gaussian_amd import pipeline, pose
    dev = gpu_device
    pc, cam, hyper, opt, bg = _model(dev, seed=24)
    pipe = pipeline._default_pipe(None)
    cams = [cam, dict(cam)]
    a = pose.PoseRefiner(2, dev, lr=1e-3)
    with torch.no_grad():
        a.delta.copy_(torch.tensor([[0.01, 0.0, -0.02, 0.03, 0.0, 0.01], [0.0, 0.02, 0.0, -0.01, 0.02, 0.0]], dtype=torch.float64))
    loss = a.corrected(cam, 0)["viewmatrix"].sum() + a.corrected(cam, 1)["campos"].sum()
    loss.backward()
    a.step()                                                 # so that the optimizer has state to carry
    b = pose.PoseRefiner(2, dev, lr=1e-3)
    b.load_state_dict(a.state_dict())
    assert torch.equal(a.delta.detach(), b.delta.detach()) and torch.equal(a.poses(cams), b.poses(cams))
    sa, sb = a.optimizer.state_dict()["state"][0], b.optimizer.state_dict()["state"][0]
    assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])
    with torch.no_grad():
        gts = [pipeline.render(c, pc, pipe, bg, stage="fine")["render"] for c in cams]
        refined = [{k: (v.detach() if torch.is_tensor(v) else v) for k, v in b.corrected(c, i).items()} for i, c in enumerate(cams)]
        assert not torch.equal(pipeline.render(refined[0], pc, pipe, bg, stage="fine")["render"], gts[0])      # the pose does move the image
    r_pose = pipeline.evaluate(pc, cams, gts, pipe, bg, pose=b)
    r_at = pipeline.evaluate(pc, refined, gts, pipe, bg)
    r_plain = pipeline.evaluate(pc, cams, gts, pipe, bg)
    psnr_ssim = lambda r: r["per_frame"][:, :2]             # (the masked columns are NaN without masks)
    assert torch.equal(psnr_ssim(r_pose), psnr_ssim(r_at)) and not torch.equal(psnr_ssim(r_pose), psnr_ssim(r_plain))
    assert bool(torch.isfinite(psnr_ssim(r_pose)).all())
    assert b.delta.grad is None                              # no gradient flows there
