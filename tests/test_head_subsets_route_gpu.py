"""Networks without the SH head (no_dshs) or without the feature head (feat_head off) on the fused deformation route
(`Deformation._fused_heads_ok`): the module against the reference restatement, pipeline.render and two training steps fused against
forced-library, and the evaluation entry points.  "Forced-library" = tests.util.library_route (`_fused_any = lambda: False` on
the module), as tests/test_static_route_gpu.py forces it: the library-GEMM branch these configurations took before they were admitted.
Bars: those of tests/test_static_route_gpu.py and tests/test_geometry_route_gpu.py."""
import contextlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.util import library_route, rel_l2

pytestmark = pytest.mark.gpu

PIPE = dict(convert_SHs_python=True, compute_cov3D_python=False, debug=False)
CONFIGS = {
    "no_feat_head": dict(feat_head=False),
    "no_dshs": dict(no_dshs=True),
    "4dgs_default": dict(no_dshs=True, feat_head=False, no_ds=False, no_dr=False),
}
SMALL = dict(grid_dimensions=2, input_coordinate_dim=4, output_coordinate_dim=32, resolution=[8, 8, 8, 5])


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


@contextlib.contextmanager
def _library(pc):
    """with _library(pc): library_route, for a module that only the third family of head switches admits to the fused route."""
    net = pc._deformation.deformation_net
    assert net._fused_heads_ok() and not net._fused_ok() and not net._fused_geometry_ok()
    with library_route(pc):
        assert not net._fused_any()
        yield


@pytest.fixture(scope="module")
def scene():
    from s3gaussian_amd import synth
    return synth.street_scene(P=5000, seed=1, width=160, height=112, n_frames=2)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_module_takes_the_fused_path_and_matches_the_restatement(gpu_device, name, monkeypatch):
    """The set-up and bars of test_static_deformation_module_takes_the_fused_path_and_matches_the_restatement."""
    from oracle import hexplane_ref as hr
    from s3gaussian_amd import deformation
    from s3gaussian_amd.deformation import deform_network
    over = CONFIGS[name]
    torch.manual_seed(0)
    hyper = hr.default_hyper(kplanes_config=SMALL, **over)
    ref = hr.deform_network(hyper)
    with torch.no_grad():
        for p in ref.deformation_net.grid.grids.parameters():
            p.add_(0.2 * torch.randn_like(p))
    mine = deform_network(hyper)
    mine.load_state_dict(ref.state_dict())
    mine = mine.to(gpu_device)
    net = mine.deformation_net
    assert net._fused_heads_ok() and not net._fused_ok() and not net._fused_geometry_ok()
    calls = []
    real = deformation.deform_mlp
    monkeypatch.setattr(deformation, "deform_mlp", lambda *a, **k: (calls.append(k), real(*a, **k))[1])
    P = 777
    g = torch.Generator().manual_seed(3)
    xyz = torch.rand(P, 3, generator=g) * 3 - 1.5
    sc, rot, op = torch.randn(P, 3, generator=g), torch.randn(P, 4, generator=g), torch.randn(P, 1, generator=g)
    shs = torch.randn(P, 16, 3, generator=g)
    t = torch.full((P, 1), 0.41)
    xr, sr = xyz.clone().requires_grad_(True), shs.clone().requires_grad_(True)
    outs_r = ref(xr, sc, rot, op, sr, t)
    assert (outs_r[7] is None) == bool(over.get("no_dshs")) and (outs_r[6] is None) == (not over.get("feat_head", True))
    ws = [None if o is None else torch.randn(o.shape, generator=g) for o in outs_r]
    sum((o * w).sum() for o, w in zip(outs_r, ws) if o is not None).backward()
    dev = gpu_device
    xg, sg = xyz.to(dev).requires_grad_(True), shs.to(dev).requires_grad_(True)
    outs_g = mine(xg, sc.to(dev), rot.to(dev), op.to(dev), sg, t.to(dev))
    assert len(calls) == 1 and calls[0]["need_dshs"] == (not over.get("no_dshs", False))      # the fused branch ran
    assert len(outs_g) == len(outs_r) == 8
    sum((o * w.to(dev)).sum() for o, w in zip(outs_g, ws) if o is not None).backward()
    for a, b in zip(outs_g, outs_r):
        assert (a is None) == (b is None)                      # absent outputs are None, in the reference's tuple order
        if a is not None:
            np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().numpy(), rtol=1e-4, atol=2e-5)
    assert rel_l2(xg.grad.cpu().numpy(), xr.grad.numpy()) < 1e-4
    assert rel_l2(sg.grad.cpu().numpy(), sr.grad.numpy()) < 1e-5
    gr = dict(ref.named_parameters())
    compared = 0
    for k, p in mine.named_parameters():
        if gr[k].grad is None:
            assert p.grad is None, k
        else:
            assert p.grad is not None and rel_l2(p.grad.cpu().numpy(), gr[k].grad.numpy()) < 1e-4, k
            compared += 1
    assert compared >= 2 + 4 + 6        # feature_out, at least one head + the six planes of at least one level


@pytest.mark.parametrize("name", list(CONFIGS))
def test_render_fused_and_library_routes_agree(gpu_device, scene, name):
    """The bars of test_static_render_fused_and_unfused_paths_agree."""
    from s3gaussian_amd.pipeline import default_hyper, render
    dev = gpu_device
    hyper = default_hyper(**CONFIGS[name])
    pc = _model(scene, hyper, dev)
    cam = _cam(scene, 1, dev)
    pipe = SimpleNamespace(**PIPE)
    bg = scene["bg"].to(dev)

    def run(library):
        for p in pc.parameters():
            p.grad = None
        if library:
            with _library(pc):
                pkg = render(cam, pc, pipe, bg, stage="fine", return_dx=True, render_feat=hyper.feat_head)
        else:
            pkg = render(cam, pc, pipe, bg, stage="fine", return_dx=True, render_feat=hyper.feat_head)
        assert pkg["dx"] is not None and (pkg["dshs"] is None) == hyper.no_dshs and ("feat" in pkg) == hyper.feat_head
        loss = pkg["render"].sum() + 0.1 * pkg["depth"].sum() + pkg["dx"].abs().sum()
        if hyper.feat_head:
            loss = loss + pkg["feat"].sum()
        if not hyper.no_dshs:
            loss = loss + pkg["dshs"].abs().sum()
        loss.backward()
        return pkg, {n: p.grad.clone() for n, p in pc.named_parameters() if p.grad is not None}

    pk1, g1 = run(False)
    pk2, g2 = run(True)
    assert "plane_reg" in pk1 and "plane_reg" not in pk2                # the fused route's by-products
    assert ("dshs_l1" in pk1) == (not hyper.no_dshs) and "dshs_l1" not in pk2
    assert torch.equal(pk1["radii"], pk2["radii"])
    for k in ("render", "depth", "dx") + (("feat",) if hyper.feat_head else ()) + (() if hyper.no_dshs else ("dshs",)):
        np.testing.assert_allclose(pk1[k].detach().cpu().numpy(), pk2[k].detach().cpu().numpy(), rtol=1e-4, atol=1e-5)
    assert set(g1) == set(g2)
    assert not any("dino_head" in k for k in g1) or hyper.feat_head
    assert not any("shs_deform" in k for k in g1) or not hyper.no_dshs
    for k in g1:
        assert rel_l2(g1[k].cpu().numpy(), g2[k].cpu().numpy()) < 2e-4, k
    with torch.no_grad():                # inference render: same image from the kernels without a stash, decomposition included
        a = render(cam, pc, pipe, bg, stage="fine", return_decomposition=True, return_dx=True)
        with _library(pc):
            b = render(cam, pc, pipe, bg, stage="fine", return_decomposition=True, return_dx=True)
    for k in ("render", "render_d", "render_s"):
        np.testing.assert_allclose(a[k].cpu().numpy(), b[k].cpu().numpy(), rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_training_steps_fused_equal_forced_library(gpu_device, scene, name):
    """Two training_step(densify_stats=True) from the same state on both routes, at the bars of
    test_static_training_steps_fused_equal_forced_unfused.  Without a feature head there is one image node and the statistics take
    the separate pass."""
    from s3gaussian_amd.pipeline import default_hyper, default_opt, training_step
    dev = gpu_device
    hyper, opt = default_hyper(**CONFIGS[name]), default_opt()
    H, W = 112, 160
    g = torch.Generator().manual_seed(0)
    gt = [torch.rand(3, H, W, generator=g).to(dev), (torch.rand(1, H, W, generator=g) * 50).to(dev), torch.rand(3, H, W, generator=g).to(dev)]
    cam = _cam(scene, 0, dev)
    res = {}
    for fused in (True, False):
        pc = _model(scene, hyper, dev, opt)
        net = pc._deformation.deformation_net
        pipe = SimpleNamespace(**PIPE)
        for _ in range(2):
            if fused:
                loss, pkg = training_step(pc, cam, *gt, hyper, opt, scene["bg"].to(dev), pipe=pipe, densify_stats=True)
            else:
                with _library(pc):
                    loss, pkg = training_step(pc, cam, *gt, hyper, opt, scene["bg"].to(dev), pipe=pipe, densify_stats=True)
            assert ("plane_reg" in pkg) == fused and pkg["dx"] is not None and (pkg["dshs"] is None) == hyper.no_dshs
            assert pkg["densify_stats_fused"] == hyper.feat_head and ("feat" in pkg) == hyper.feat_head
        if hyper.no_dshs:
            for p in net.shs_deform.parameters():
                assert p not in pc.optimizer.state or not pc.optimizer.state[p]       # no moments, no step count
        assert len([p for p in net.pos_deform.parameters() if pc.optimizer.state.get(p)]) == 4
        res[fused] = (float(loss), {n: p.detach().clone() for n, p in pc.named_parameters()}, pc.xyz_gradient_accum.clone(),
                      pc.denom.clone(), pc.max_radii2D.clone())
    a, b = res[True], res[False]
    assert abs(a[0] - b[0]) <= 2e-4 * abs(b[0])
    for n in a[1]:
        assert rel_l2(a[1][n].cpu().numpy(), b[1][n].cpu().numpy()) < 2e-4, n
    assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4]) and float(a[3].max()) == 2.0
    np.testing.assert_allclose(a[2].cpu().numpy(), b[2].cpu().numpy(), rtol=1e-4, atol=1e-9)


def _eval_scene(dev, **over):
    """2 000 Gaussians, 96 x 64, 2 timestamps x 3 cameras, enlarged so that the small image is covered (the scene of
    tests/test_static_route_gpu.py's evaluation tests)."""
    import math
    from s3gaussian_amd import synth
    from s3gaussian_amd.pipeline import GaussianParams, default_hyper
    scn = synth.street_scene(P=2000, seed=4, width=96, height=64, n_frames=2)
    gs = scn["gaussians"]
    torch.manual_seed(0)
    pc = GaussianParams(3, default_hyper(**over))
    pc.init_from_tensors(gs["xyz"], gs["log_scales"] + math.log(12.0), gs["rotations_raw"], gs["opacity_logit"], gs["shs"], dev)
    net = pc._deformation.deformation_net
    net.set_aabb(*scn["aabb"])
    with torch.no_grad():
        for p in list(net.pos_deform.parameters()) + list(net.grid.grids.parameters()):
            p.add_(0.2 * torch.randn_like(p))
    cams = [_cam(scn, i, dev) for i in range(len(scn["cameras"]))]
    g = torch.Generator().manual_seed(21)
    gts = [torch.rand(3, 64, 96, generator=g).to(dev) for _ in range(6)]
    return SimpleNamespace(pc=pc, cams=cams, gts=gts, pipe=SimpleNamespace(**PIPE), bg=torch.tensor([0.1, 0.2, 0.3], device=dev))


@pytest.mark.parametrize("name", list(CONFIGS))
def test_entry_points_run_where_a_dx_exists(gpu_device, name, tmp_path):
    from s3gaussian_amd.pipeline import evaluate, evaluate_video, render, save_split_point_clouds
    s = _eval_scene(gpu_device, **CONFIGS[name])
    keys = ("gt_rgbs", "rgbs", "depths", "dynamic_rgbs")
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
    assert torch.equal(m["per_frame"][:, :2], res["per_frame"][:, :2])
    assert m["psnr"] == res["psnr"] and m["psnr"] > 0 and m["ssim"] == res["ssim"]
    out = save_split_point_clouds(s.pc, s.cams[0]["time"], str(tmp_path / "dynamic.ply"), str(tmp_path / "static.ply"))
    assert out["n_dynamic"] + out["n_static"] == 2000 and out["n_dynamic"] > 0


@pytest.mark.parametrize("name", list(CONFIGS))
def test_entry_points_refuse_without_a_dx_and_name_the_switch(gpu_device, name, tmp_path):
    from s3gaussian_amd.pipeline import evaluate_video, render_flows, save_split_point_clouds
    s = _eval_scene(gpu_device, no_dx=True, **CONFIGS[name])
    assert s.pc._deformation.deformation_net._fused_heads_ok()
    with pytest.raises(RuntimeError, match="no_dx"):
        render_flows(s.pc, s.cams, s.pipe, s.bg, num_cams=3)
    for key in ("forward_flows", "dynamic_rgbs"):
        with pytest.raises(RuntimeError, match="no_dx"):
            evaluate_video(s.pc, s.cams, s.gts, s.pipe, s.bg, num_cams=3, keys=("rgbs", key))
    with pytest.raises(RuntimeError, match="no_dx"):
        save_split_point_clouds(s.pc, s.cams[0]["time"], str(tmp_path / "dynamic.ply"), str(tmp_path / "static.ply"))
    res = evaluate_video(s.pc, s.cams, s.gts, s.pipe, s.bg, num_cams=3, keys=("rgbs", "depths"))      # what needs no dx still runs
    assert res["num_timestamps"] == 2
