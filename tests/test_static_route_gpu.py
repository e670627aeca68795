"""Static scenes (ModelHiddenParams no_dx=True, the reference's arguments/static_nvs.py) on the fused deformation route: the module
against the reference restatement, pipeline.render fused against forced-unfused, two training steps, the evaluation entry points and
the zero-edit route.  "Forced-unfused" = tests.util.library_route (`_fused_any = lambda: False` on the module): the library-GEMM
branch this configuration took before it was admitted to the fused route."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.util import library_route, rel_l2

pytestmark = pytest.mark.gpu

PIPE = dict(convert_SHs_python=True, compute_cov3D_python=False, debug=False)


def _model(scn, hyper, dev, opt=None, seed=0):
    from s3gaussian_amd.pipeline import GaussianParams
    torch.manual_seed(seed)
    pc = GaussianParams(3, hyper)
    gs = scn["gaussians"]
    pc.init_from_tensors(gs["xyz"], gs["log_scales"], gs["rotations_raw"], gs["opacity_logit"], gs["shs"], dev)
    pc._deformation.deformation_net.set_aabb(*scn["aabb"])
    if opt is not None:
        pc.training_setup(opt)
    return pc


def _cam(scn, i, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in scn["cameras"][i].items()}


def test_static_deformation_module_takes_the_fused_path_and_matches_the_restatement(gpu_device):
    """The set-up and bars of test_deformation_module_uses_fused_path_and_matches_golden with no_dx=True."""
    from oracle import hexplane_ref as hr
    from s3gaussian_amd.deformation import deform_network
    torch.manual_seed(0)
    hyper = hr.default_hyper(no_dx=True, kplanes_config=dict(grid_dimensions=2, input_coordinate_dim=4, output_coordinate_dim=32,
                                                             resolution=[8, 8, 8, 5]))
    ref = hr.deform_network(hyper)
    with torch.no_grad():
        for p in ref.deformation_net.grid.grids.parameters():
            p.add_(0.2 * torch.randn_like(p))
    mine = deform_network(hyper)
    mine.load_state_dict(ref.state_dict())
    mine = mine.to(gpu_device)
    assert mine.deformation_net._fused_ok()
    P = 777
    g = torch.Generator().manual_seed(3)
    xyz = torch.rand(P, 3, generator=g) * 3 - 1.5
    sc, rot, op = torch.randn(P, 3, generator=g), torch.randn(P, 4, generator=g), torch.randn(P, 1, generator=g)
    shs = torch.randn(P, 16, 3, generator=g)
    t = torch.full((P, 1), 0.41)
    xr, sr = xyz.clone().requires_grad_(True), shs.clone().requires_grad_(True)
    outs_r = ref(xr, sc, rot, op, sr, t)
    assert outs_r[5] is None
    ws = [None if o is None else torch.randn(o.shape, generator=g) for o in outs_r]
    sum((o * w).sum() for o, w in zip(outs_r, ws) if o is not None).backward()
    dev = gpu_device
    xg, sg = xyz.to(dev).requires_grad_(True), shs.to(dev).requires_grad_(True)
    outs_g = mine(xg, sc.to(dev), rot.to(dev), op.to(dev), sg, t.to(dev))
    assert len(outs_g) == len(outs_r) == 8
    assert outs_g[5] is None                                   # dx, in the reference's tuple order
    assert torch.equal(outs_g[0].detach(), xg.detach())        # means3D is xyz itself
    sum((o * w.to(dev)).sum() for o, w in zip(outs_g, ws) if o is not None).backward()
    for a, b in zip(outs_g, outs_r):
        assert (a is None) == (b is None)
        if a is not None:
            np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().numpy(), rtol=1e-4, atol=2e-5)
    assert rel_l2(xg.grad.cpu().numpy(), xr.grad.numpy()) < 1e-4
    assert rel_l2(sg.grad.cpu().numpy(), sr.grad.numpy()) < 1e-5
    gr = dict(ref.named_parameters())
    compared = 0
    for k, p in mine.named_parameters():
        if "pos_deform" in k:
            assert p.grad is None and gr[k].grad is None, k
        elif gr[k].grad is not None:
            assert rel_l2(p.grad.cpu().numpy(), gr[k].grad.numpy()) < 1e-4, k
            compared += 1
    assert compared >= 12 + 6        # feature_out, shs_deform, dino_head + the six planes of at least one level


def test_static_render_fused_and_unfused_paths_agree(gpu_device):
    """The scene and bars of test_render_fused_and_unfused_paths_agree with hyper.no_dx = True."""
    from s3gaussian_amd import synth
    from s3gaussian_amd.pipeline import default_hyper, render
    dev = gpu_device
    scn = synth.street_scene(P=5000, seed=1, width=160, height=112, n_frames=2)
    pc = _model(scn, default_hyper(no_dx=True), dev)
    cam = _cam(scn, 1, dev)
    pipe = SimpleNamespace(**PIPE)
    bg = scn["bg"].to(dev)

    def run(force_unfused):
        for p in pc.parameters():
            p.grad = None
        if force_unfused:
            with library_route(pc):
                pkg = render(cam, pc, pipe, bg, stage="fine", return_dx=True, render_feat=True)
        else:
            pkg = render(cam, pc, pipe, bg, stage="fine", return_dx=True, render_feat=True)
        assert "dx" in pkg and pkg["dx"] is None
        (pkg["render"].sum() + 0.1 * pkg["depth"].sum() + pkg["feat"].sum() + pkg["dshs"].abs().sum()).backward()
        return pkg, {n: p.grad.clone() for n, p in pc.named_parameters() if p.grad is not None}

    pk1, g1 = run(False)
    pk2, g2 = run(True)
    assert "dshs_l1" in pk1 and "plane_reg" in pk1               # the fused route's by-products
    assert "dshs_l1" not in pk2 and "plane_reg" not in pk2
    assert torch.equal(pk1["radii"], pk2["radii"])
    for k in ("render", "depth", "feat", "dshs"):
        np.testing.assert_allclose(pk1[k].detach().cpu().numpy(), pk2[k].detach().cpu().numpy(), rtol=1e-4, atol=1e-5)
    assert set(g1) == set(g2) and not any("pos_deform" in k for k in g1)
    for k in g1:
        assert rel_l2(g1[k].cpu().numpy(), g2[k].cpu().numpy()) < 2e-4, k
    for grad in (True, False):           # with a position head these would add render_d / render_s; the reference guards on dx
        with torch.set_grad_enabled(grad):
            pkg = render(cam, pc, pipe, bg, stage="fine", return_decomposition=True, return_dx=True)
        assert "render_d" not in pkg and "render_s" not in pkg and pkg["dx"] is None


def test_static_training_steps_fused_equal_forced_unfused(gpu_device):
    """Two training_step(densify_stats=True) from the same state on both routes.  Statistics at the bars of
    test_training_step_densify_stats_fused_equals_separate_pass (denom / max_radii2D equal, the gradient accumulator rtol 1e-4);
    that test has no bar for the loss and the parameters: relative L2 < 2e-4, the gradient bar of the render test above."""
    from s3gaussian_amd import synth
    from s3gaussian_amd.pipeline import default_hyper, default_opt, training_step
    dev = gpu_device
    scn = synth.street_scene(P=20_000, seed=0, width=320, height=208, n_frames=2)
    hyper, opt = default_hyper(no_dx=True), default_opt()
    H, W = 208, 320
    g = torch.Generator().manual_seed(0)
    gt = [torch.rand(3, H, W, generator=g).to(dev), (torch.rand(1, H, W, generator=g) * 50).to(dev), torch.rand(3, H, W, generator=g).to(dev)]
    cam = _cam(scn, 0, dev)
    res = {}
    for fused in (True, False):
        pc = _model(scn, hyper, dev, opt)
        net = pc._deformation.deformation_net
        pos0 = [p.detach().clone() for p in net.pos_deform.parameters()]
        pipe = SimpleNamespace(**PIPE)
        for _ in range(2):
            if fused:
                loss, pkg = training_step(pc, cam, *gt, hyper, opt, scn["bg"].to(dev), pipe=pipe, densify_stats=True)
            else:
                with library_route(pc):
                    loss, pkg = training_step(pc, cam, *gt, hyper, opt, scn["bg"].to(dev), pipe=pipe, densify_stats=True)
            assert ("dshs_l1" in pkg) == fused and pkg["dx"] is None and pkg["densify_stats_fused"]
        for p, p0 in zip(net.pos_deform.parameters(), pos0):
            assert torch.equal(p.detach(), p0)
            assert p not in pc.optimizer.state or not pc.optimizer.state[p]       # no moments, no step count
        stepped = [p for p in net.shs_deform.parameters() if pc.optimizer.state.get(p)]
        assert len(stepped) == 4                                                  # (the live heads do have a state)
        res[fused] = (float(loss), {n: p.detach().clone() for n, p in pc.named_parameters()}, pc.xyz_gradient_accum.clone(),
                      pc.denom.clone(), pc.max_radii2D.clone())
    a, b = res[True], res[False]
    assert abs(a[0] - b[0]) <= 2e-4 * abs(b[0])
    for n in a[1]:
        assert rel_l2(a[1][n].cpu().numpy(), b[1][n].cpu().numpy()) < 2e-4, n
    assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4]) and float(a[3].max()) == 2.0
    np.testing.assert_allclose(a[2].cpu().numpy(), b[2].cpu().numpy(), rtol=1e-4, atol=1e-9)


@pytest.fixture(scope="module")
def static_scene(gpu_device):
    """2 000 Gaussians, 96 x 64, 2 timestamps x 3 cameras, enlarged so that the small image is covered (the scene of
    tests/test_frames_gpu.py with no_dx=True)."""
    import math
    from s3gaussian_amd import synth
    from s3gaussian_amd.pipeline import GaussianParams, default_hyper
    dev = gpu_device
    scn = synth.street_scene(P=2000, seed=4, width=96, height=64, n_frames=2)
    gs = scn["gaussians"]
    torch.manual_seed(0)
    pc = GaussianParams(3, default_hyper(no_dx=True))
    pc.init_from_tensors(gs["xyz"], gs["log_scales"] + math.log(12.0), gs["rotations_raw"], gs["opacity_logit"], gs["shs"], dev)
    net = pc._deformation.deformation_net
    net.set_aabb(*scn["aabb"])
    with torch.no_grad():
        for p in list(net.shs_deform.parameters()) + list(net.grid.grids.parameters()):
            p.add_(0.2 * torch.randn_like(p))
    cams = [_cam(scn, i, dev) for i in range(len(scn["cameras"]))]
    assert len(cams) == 6 and len({c["time"] for c in cams}) == 2
    g = torch.Generator().manual_seed(21)
    gts = [torch.rand(3, 64, 96, generator=g).to(dev) for _ in range(6)]
    return SimpleNamespace(pc=pc, cams=cams, gts=gts, pipe=SimpleNamespace(**PIPE), bg=torch.tensor([0.1, 0.2, 0.3], device=dev))


def test_static_evaluation_renders_use_the_inference_cache(static_scene, monkeypatch):
    from s3gaussian_amd import deformation, raster_C
    from s3gaussian_amd.pipeline import render
    s = static_scene
    assert s.cams[0]["time"] == s.cams[1]["time"]
    monkeypatch.setattr(deformation, "deform_infer", lambda *a, **k: pytest.fail("deform_infer called for a no_dx network"))
    out = {}
    with torch.no_grad():
        for cache in (True, False):
            monkeypatch.setattr(deformation, "INFER_CACHE", cache)
            raster_C.invalidate_geometry_cache()              # (also drops the deformation's cached evaluation)
            h0 = deformation.infer_cache_hits
            out[cache] = [render(cam, s.pc, s.pipe, s.bg, stage="fine", return_dx=True) for cam in s.cams[:2]]
            assert deformation.infer_cache_hits - h0 == (1 if cache else 0)
    for a, b in zip(out[True], out[False]):
        assert a["dx"] is None and b["dx"] is None
        for k in ("render", "depth", "radii", "dshs"):
            assert torch.equal(a[k], b[k]), k
    assert not torch.equal(out[True][0]["render"], out[True][1]["render"])


def test_static_evaluate_and_evaluate_video(static_scene):
    from s3gaussian_amd.pipeline import evaluate, evaluate_video, render
    s = static_scene
    keys = ("gt_rgbs", "rgbs", "depths")
    res = evaluate_video(s.pc, s.cams, s.gts, s.pipe, s.bg, num_cams=3, keys=keys)
    assert res["num_timestamps"] == 2 and tuple(res["frames"]) == keys
    for k in keys:
        assert len(res["frames"][k]) == 2
        for strip in res["frames"][k]:
            assert strip.is_cuda and strip.dtype == torch.uint8 and tuple(strip.shape) == (64, 3 * 96, 1 if k == "depths" else 3)
    with torch.no_grad():
        img = render(s.cams[4], s.pc, s.pipe, s.bg, stage="fine")["render"]
    want = (255 * img.clamp(0, 1).permute(1, 2, 0)).to(torch.uint8)          # to8b of camera 1 of timestamp 1
    assert int((res["frames"]["rgbs"][1][:, 96:192].int() - want.int()).abs().max()) <= 1
    m = evaluate(s.pc, s.cams, s.gts, s.pipe, s.bg)
    assert torch.equal(m["per_frame"][:, :2], res["per_frame"][:, :2])       # PSNR, SSIM (no masks given: the masked columns are NaN)
    assert m["psnr"] == res["psnr"] and m["psnr"] > 0 and m["ssim"] == res["ssim"]


def test_flows_and_decomposition_are_refused_for_a_static_model(static_scene):
    from s3gaussian_amd.pipeline import evaluate_video, render_flows
    s = static_scene
    with pytest.raises(RuntimeError, match="no_dx"):
        render_flows(s.pc, s.cams, s.pipe, s.bg, num_cams=3)
    for key in ("forward_flows", "backward_flows", "dynamic_rgbs", "static_rgbs"):
        with pytest.raises(RuntimeError, match="no_dx"):
            evaluate_video(s.pc, s.cams, s.gts, s.pipe, s.bg, num_cams=3, keys=("rgbs", key))


def test_one_static_train_py_iteration_on_the_replacements_equals_the_fused_step(gpu_device):
    """The set-up and bars of tests/test_patch_gpu.py::test_one_train_py_iteration_on_the_replacements_equals_the_fused_step with
    no_dx=True: `--configs arguments/static_nvs.py` on the zero-edit route."""
    import bench
    from s3gaussian_amd import synth
    from s3gaussian_amd.pipeline import default_hyper, default_opt, training_step
    dev = gpu_device
    scn = synth.street_scene(P=15_000, seed=3, width=240, height=160, n_frames=2)
    hyper, opt = default_hyper(no_dx=True), default_opt()
    H, W = 160, 240
    g = torch.Generator().manual_seed(0)
    gts = (torch.rand(3, H, W, generator=g).to(dev), (torch.rand(1, H, W, generator=g) * 60).to(dev), torch.rand(3, H, W, generator=g).to(dev))
    cam = _cam(scn, 1, dev)
    res = {}
    for path in ("fused", "patched"):
        pc = _model(scn, hyper, dev, opt)
        assert pc._deformation.deformation_net._fused_ok()
        if path == "fused":
            loss, _ = training_step(pc, cam, *gts, hyper, opt, scn["bg"].to(dev), densify_stats=True)
        else:
            loss = bench.patched_reference_step(pc, bench.camera_object(cam, gts), hyper, opt, scn["bg"].to(dev))
        res[path] = (float(loss), {n: p.detach().clone() for n, p in pc.named_parameters()}, pc.xyz_gradient_accum.clone(),
                     pc.denom.clone(), pc.max_radii2D.clone())
    assert abs(res["fused"][0] - res["patched"][0]) <= 1e-5 * abs(res["fused"][0])
    for n, p in res["fused"][1].items():
        # (an element whose gradient is a cancellation to round-off may take the other sign of the first Adam step: that test's bar)
        close = torch.isclose(p, res["patched"][1][n], rtol=1e-4, atol=1e-6)
        assert float((~close).float().mean()) < 1e-3, n
    assert torch.equal(res["fused"][3], res["patched"][3]) and torch.equal(res["fused"][4], res["patched"][4])
    np.testing.assert_allclose(res["fused"][2].cpu().numpy(), res["patched"][2].cpu().numpy(), rtol=1e-4, atol=1e-9)
