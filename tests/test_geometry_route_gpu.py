"""Scale / rotation / opacity deformation (ModelHiddenParams no_ds = no_dr = no_do = False, once more with apply_rotation) on the
fused deformation route: the module against the reference restatement and against a golden of the reference's own module,
pipeline.render fused against forced-library, two training steps, and the evaluation entry points.
"Forced-library" = tests.util.library_route (`_fused_any = lambda: False` on the module): the library-GEMM branch of forward_dynamic and
the torch glue, which this configuration took before it was admitted to the fused route.
The three heads' output layers are re-initialised with std 0.02 (xavier leaves ds / dr / do of order 1, which destroys the scene)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.test_static_route_gpu import PIPE, _cam, _model
from tests.util import library_route, rel_l2

pytestmark = pytest.mark.gpu

GEOMETRY = dict(no_ds=False, no_dr=False, no_do=False)
VARIANTS = [pytest.param(False, id="add"), pytest.param(True, id="apply_rotation")]


def _hyper(apply_rotation, **over):
    from s3gaussian_amd.pipeline import default_hyper
    return default_hyper(apply_rotation=apply_rotation, **GEOMETRY, **over)


def _small_geometry_heads(net, seed=17):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for head in (net.scales_deform, net.rotations_deform, net.opacity_deform):
            for p in (head[3].weight, head[3].bias):
                p.copy_((0.02 * torch.randn(p.shape, generator=g)).to(p.device))


def _geometry_model(scn, hyper, dev, opt=None, seed=0):
    pc = _model(scn, hyper, dev, opt, seed)
    _small_geometry_heads(pc._deformation.deformation_net)
    return pc


@pytest.fixture
def geometry_calls(monkeypatch):
    """Counts the calls of the fused geometry-heads operator made through the deformation module."""
    from s3gaussian_amd import deformation
    calls = []
    real = deformation.geometry_heads
    monkeypatch.setattr(deformation, "geometry_heads", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


@pytest.mark.parametrize("apply_rotation", VARIANTS)
def test_geometry_module_takes_the_fused_path_and_matches_the_restatement(gpu_device, apply_rotation, geometry_calls):
    """The set-up and bars of test_static_deformation_module_takes_the_fused_path_and_matches_the_restatement at four levels with all
    heads on.  The restatement adds dr; with apply_rotation its rotation entry is rebuilt as the normalised quaternion product of the
    input and that same dr (utils/graphics_utils.py:154-177), on the CPU."""
    from oracle import hexplane_ref as hr
    from s3gaussian_amd.deformation import batch_quaternion_multiply, deform_network
    torch.manual_seed(0)
    hyper = hr.default_hyper(apply_rotation=apply_rotation, kplanes_config=dict(grid_dimensions=2, input_coordinate_dim=4,
                                                                                output_coordinate_dim=32, resolution=[8, 8, 8, 5]), **GEOMETRY)
    assert list(hyper.multires) == [1, 2, 4, 8]
    ref = hr.deform_network(hyper)
    with torch.no_grad():
        for p in ref.deformation_net.grid.grids.parameters():
            p.add_(0.2 * torch.randn_like(p))
    _small_geometry_heads(ref.deformation_net)
    mine = deform_network(hyper)
    mine.load_state_dict(ref.state_dict())
    mine = mine.to(gpu_device)
    assert mine.deformation_net._fused_geometry_ok() and not mine.deformation_net._fused_ok()
    P = 777
    g = torch.Generator().manual_seed(3)
    xyz = torch.rand(P, 3, generator=g) * 3 - 1.5
    sc, rot, op = torch.randn(P, 3, generator=g), torch.randn(P, 4, generator=g), torch.randn(P, 1, generator=g)
    shs = torch.randn(P, 16, 3, generator=g)
    t = torch.full((P, 1), 0.41)
    xr, sr = xyz.clone().requires_grad_(True), shs.clone().requires_grad_(True)
    outs_r = list(ref(xr, sc, rot, op, sr, t))
    if apply_rotation:
        outs_r[2] = batch_quaternion_multiply(rot, outs_r[2] - rot)
    ws = [torch.randn(o.shape, generator=g) for o in outs_r]
    sum((o * w).sum() for o, w in zip(outs_r, ws)).backward()
    dev = gpu_device
    xg, sg = xyz.to(dev).requires_grad_(True), shs.to(dev).requires_grad_(True)
    outs_g = mine(xg, sc.to(dev), rot.to(dev), op.to(dev), sg, t.to(dev))
    assert len(geometry_calls) == 1                                   # the fused route was taken
    assert len(outs_g) == len(outs_r) == 8 and all(o is not None for o in outs_g)
    for i, raw in ((1, sc), (2, rot), (3, op)):                       # and the three heads do deform
        assert float((outs_g[i].detach().cpu() - raw).abs().max()) > 1e-3
    sum((o * w.to(dev)).sum() for o, w in zip(outs_g, ws)).backward()
    for a, b in zip(outs_g, outs_r):
        np.testing.assert_allclose(a.detach().cpu().numpy(), b.detach().numpy(), rtol=1e-4, atol=2e-5)
    assert rel_l2(xg.grad.cpu().numpy(), xr.grad.numpy()) < 1e-4
    assert rel_l2(sg.grad.cpu().numpy(), sr.grad.numpy()) < 1e-5
    gr = dict(ref.named_parameters())
    compared = 0
    for k, p in mine.named_parameters():
        if gr[k].grad is not None:
            assert p.grad is not None, k
            assert rel_l2(p.grad.cpu().numpy(), gr[k].grad.numpy()) < 1e-4, k
            compared += 1
    assert compared >= 28 + 6        # feature_out, the six heads + the six planes of at least one level


@pytest.mark.parametrize("tag", ["all_heads", "all_heads_apply_rotation"])
def test_full_width_geometry_module_matches_the_reference_golden(gpu_device, tag, geometry_calls):
    """tests/golden/deform_geometry.npz (make_golden_geometry.py: the reference's own scene/deformation.py, four levels, every head on)
    at the bars of test_non_default_deformation_switches_match_reference_golden -- whose all_heads / apply_rotation variants have
    two levels (64 features) and stay on the library route."""
    from s3gaussian_amd.deformation import deform_network
    from s3gaussian_amd.pipeline import default_hyper
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "deform_geometry.npz"))
    hyper = default_hyper(kplanes_config=dict(grid_dimensions=2, input_coordinate_dim=4, output_coordinate_dim=32, resolution=[4, 4, 4, 3]),
                          multires=[1, 2, 4, 8], apply_rotation=tag.endswith("apply_rotation"), **GEOMETRY)
    net = deform_network(hyper)
    net.deformation_net.set_aabb([2.0, 1.5, 1.0], [-1.0, -1.5, -0.5])
    net.load_state_dict({k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd::")})
    net = net.to(gpu_device)
    assert net.deformation_net._fused_geometry_ok()
    t = lambda k: torch.from_numpy(z[k]).to(gpu_device)
    xyz = t("xyz").clone().requires_grad_(True)
    assert xyz.shape[0] == 100
    outs = net(xyz, t("scales"), t("rotations"), t("opacity"), t("shs"), t("time"))
    assert len(geometry_calls) == 1 and len(outs) == 8
    loss = 0
    for n, o in zip(["means3D", "scales", "rotations", "opacity", "shs", "dx", "feat", "dshs"], outs):
        np.testing.assert_allclose(o.detach().cpu().numpy(), z[f"{tag}::out_{n}"], rtol=1e-4, atol=3e-5, err_msg=n)
        loss = loss + (o * t(f"{tag}::w_{n}")).sum()
    loss.backward()
    assert rel_l2(xyz.grad.cpu().numpy(), z[f"{tag}::grad_xyz"]) < 1e-4


@pytest.mark.parametrize("apply_rotation", VARIANTS)
def test_geometry_render_fused_and_library_paths_agree(gpu_device, apply_rotation, geometry_calls):
    """The scene and bars of test_static_render_fused_and_unfused_paths_agree.  Scales differ by round-off between the routes (glue
    kernel against torch.exp), so a radius may differ by exactly 1 on at most 5 of the 5000 Gaussians."""
    from s3gaussian_amd import synth
    from s3gaussian_amd.pipeline import render
    dev = gpu_device
    scn = synth.street_scene(P=5000, seed=1, width=160, height=112, n_frames=2)
    pc = _geometry_model(scn, _hyper(apply_rotation), dev)
    cam = _cam(scn, 1, dev)
    pipe = SimpleNamespace(**PIPE)
    bg = scn["bg"].to(dev)

    def run(library):
        for p in pc.parameters():
            p.grad = None
        if library:
            with library_route(pc):
                pkg = render(cam, pc, pipe, bg, stage="fine", return_dx=True, render_feat=True)
        else:
            pkg = render(cam, pc, pipe, bg, stage="fine", return_dx=True, render_feat=True)
        (pkg["render"].sum() + 0.1 * pkg["depth"].sum() + pkg["feat"].sum() + pkg["dshs"].abs().sum()).backward()
        return pkg, {n: p.grad.clone() for n, p in pc.named_parameters() if p.grad is not None}

    pk1, g1 = run(False)
    assert len(geometry_calls) == 1
    pk2, g2 = run(True)
    assert len(geometry_calls) == 1
    assert "dshs_l1" in pk1 and "plane_reg" in pk1               # the fused route's by-products
    assert "dshs_l1" not in pk2 and "plane_reg" not in pk2
    diff = (pk1["radii"].int() - pk2["radii"].int()).abs()
    print("radii that differ:", int((diff > 0).sum()), "largest difference:", int(diff.max()))
    assert int(diff.max()) <= 1 and int((diff > 0).sum()) <= 5
    for k in ("render", "depth", "feat", "dshs"):
        np.testing.assert_allclose(pk1[k].detach().cpu().numpy(), pk2[k].detach().cpu().numpy(), rtol=1e-4, atol=1e-5)
    assert set(g1) == set(g2)
    for head in ("scales_deform", "rotations_deform", "opacity_deform"):
        assert sum(head in k for k in g1) == 4, head
    figures = {k: rel_l2(g1[k].cpu().numpy(), g2[k].cpu().numpy()) for k in g1}
    print("gradients, fused against library:", figures)
    for k in g1:
        assert figures[k] < 2e-4, (k, figures[k])


def test_geometry_training_steps_fused_equal_forced_library(gpu_device):
    """Two training_step(densify_stats=True) from the same state on both routes, on this file's scene, at the bars of
    test_static_training_steps_fused_equal_forced_unfused.  Measured on one MI355X: loss equal, no radius differs, the gradient
    accumulator's largest relative difference 4.7e-5 (bar 1e-4).  ds / dr / do differ by fp32 round-off between the routes and a few
    accumulator entries -- sums of signed per-pixel terms -- amplify that: on that test's own scene (20 000 Gaussians, 320 x 208)
    3 of 20 000 entries exceed 1e-4 (2.0e-4) after two steps and 4 (1.6e-4) after one step from identical parameters, while two
    fused runs are bit-identical."""
    from s3gaussian_amd import synth
    from s3gaussian_amd.pipeline import default_opt, training_step
    dev = gpu_device
    scn = synth.street_scene(P=5000, seed=1, width=160, height=112, n_frames=2)
    hyper, opt = _hyper(False), default_opt()
    H, W = 112, 160
    g = torch.Generator().manual_seed(0)
    gt = [torch.rand(3, H, W, generator=g).to(dev), (torch.rand(1, H, W, generator=g) * 50).to(dev), torch.rand(3, H, W, generator=g).to(dev)]
    cam = _cam(scn, 1, dev)
    res = {}
    for fused in (True, False):
        pc = _geometry_model(scn, hyper, dev, opt)
        net = pc._deformation.deformation_net
        pipe = SimpleNamespace(**PIPE)
        for _ in range(2):
            if fused:
                loss, pkg = training_step(pc, cam, *gt, hyper, opt, scn["bg"].to(dev), pipe=pipe, densify_stats=True)
            else:
                with library_route(pc):
                    loss, pkg = training_step(pc, cam, *gt, hyper, opt, scn["bg"].to(dev), pipe=pipe, densify_stats=True)
            assert ("dshs_l1" in pkg) == fused and pkg["dx"] is not None and pkg["densify_stats_fused"]
        for head in (net.scales_deform, net.rotations_deform, net.opacity_deform):
            assert len([p for p in head.parameters() if pc.optimizer.state.get(p)]) == 4        # the three heads are trained
        res[fused] = (float(loss), {n: p.detach().clone() for n, p in pc.named_parameters()}, pc.xyz_gradient_accum.clone(),
                      pc.denom.clone(), pc.max_radii2D.clone())
    a, b = res[True], res[False]
    accum = np.abs(a[2].cpu().numpy() - b[2].cpu().numpy()) / np.maximum(np.abs(b[2].cpu().numpy()), 1e-30)
    print("loss fused / library:", a[0], b[0], "gradient accumulator: entries beyond rtol 1e-4 / atol 1e-9:",
          int((~np.isclose(a[2].cpu().numpy(), b[2].cpu().numpy(), rtol=1e-4, atol=1e-9)).sum()), "largest relative difference:",
          float(accum[b[2].cpu().numpy() > 1e-5].max()))
    assert abs(a[0] - b[0]) <= 2e-4 * abs(b[0])
    for n in a[1]:
        assert rel_l2(a[1][n].cpu().numpy(), b[1][n].cpu().numpy()) < 2e-4, n
    assert torch.equal(a[3], b[3]) and torch.equal(a[4], b[4]) and float(a[3].max()) == 2.0
    np.testing.assert_allclose(a[2].cpu().numpy(), b[2].cpu().numpy(), rtol=1e-4, atol=1e-9)


@pytest.fixture(scope="module", params=VARIANTS)
def geometry_scene(request, gpu_device):
    """This file's scene (5 000 Gaussians, 160 x 112, 2 timestamps x 3 cameras) with the geometry heads on, a position head, and the
    planes and the SH head perturbed as in tests/test_static_route_gpu.py::static_scene."""
    from s3gaussian_amd import synth
    from s3gaussian_amd.pipeline import GaussianParams
    dev = gpu_device
    scn = synth.street_scene(P=5000, seed=1, width=160, height=112, n_frames=2)
    gs = scn["gaussians"]
    torch.manual_seed(0)
    pc = GaussianParams(3, _hyper(request.param))
    pc.init_from_tensors(gs["xyz"], gs["log_scales"], gs["rotations_raw"], gs["opacity_logit"], gs["shs"], dev)
    net = pc._deformation.deformation_net
    net.set_aabb(*scn["aabb"])
    with torch.no_grad():
        for p in list(net.shs_deform.parameters()) + list(net.grid.grids.parameters()):
            p.add_(0.2 * torch.randn_like(p))
    _small_geometry_heads(net)
    cams = [_cam(scn, i, dev) for i in range(len(scn["cameras"]))]
    assert len(cams) == 6 and len({c["time"] for c in cams}) == 2
    g = torch.Generator().manual_seed(21)
    gts = [torch.rand(3, 112, 160, generator=g).to(dev) for _ in range(6)]
    return SimpleNamespace(pc=pc, cams=cams, gts=gts, pipe=SimpleNamespace(**PIPE), bg=torch.tensor([0.1, 0.2, 0.3], device=dev))


def test_geometry_evaluate_and_evaluate_video(geometry_scene):
    from s3gaussian_amd.pipeline import evaluate, evaluate_video, render
    s = geometry_scene
    keys = ("rgbs", "depths")
    res = evaluate_video(s.pc, s.cams, s.gts, s.pipe, s.bg, num_cams=3, keys=keys)
    assert res["num_timestamps"] == 2 and tuple(res["frames"]) == keys
    with torch.no_grad():
        pkg = render(s.cams[4], s.pc, s.pipe, s.bg, stage="fine")
    want = (255 * pkg["render"].clamp(0, 1).permute(1, 2, 0)).to(torch.uint8)          # to8b of camera 1 of timestamp 1
    assert int((res["frames"]["rgbs"][1][:, 160:320].int() - want.int()).abs().max()) <= 1
    depth = pkg["depth"] / pkg["depth"].max()
    want_d = (255 * depth.clamp(0, 1).permute(1, 2, 0)).to(torch.uint8)
    assert int((res["frames"]["depths"][1][:, 160:320].int() - want_d.int()).abs().max()) <= 1
    m = evaluate(s.pc, s.cams, s.gts, s.pipe, s.bg)
    assert torch.equal(m["per_frame"][:, :2], res["per_frame"][:, :2])       # PSNR, SSIM: both loops saw render's images
    assert m["psnr"] == res["psnr"] and m["psnr"] > 0 and m["ssim"] == res["ssim"]


def test_geometry_flows_and_split_export_accept_the_model(geometry_scene, tmp_path):
    from s3gaussian_amd.pipeline import render, render_flows, save_split_point_clouds
    s = geometry_scene
    res = render_flows(s.pc, s.cams, s.pipe, s.bg, num_cams=3, with_rgb=True)
    assert len(res["rgbs"]) == len(res["forward_flows"]) == len(res["backward_flows"]) == 6
    with torch.no_grad():
        for i in (0, 4):
            assert torch.equal(res["rgbs"][i], render(s.cams[i], s.pc, s.pipe, s.bg, stage="fine")["render"]), i
    assert float((res["forward_flows"][0] - res["forward_flows"][0][:, :1, :1]).abs().max()) > 0       # a flow image, not a flat colour
    info = save_split_point_clouds(s.pc, s.cams[0]["time"], str(tmp_path / "dynamic.ply"), str(tmp_path / "static.ply"))
    assert info["n_dynamic"] + info["n_static"] == 5000 and info["n_dynamic"] > 0
    assert os.path.exists(tmp_path / "dynamic.ply") and os.path.exists(tmp_path / "static.ply")
