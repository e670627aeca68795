"""The opacity image and the sky term through the pipeline's routes: render(return_alpha=True) on every deformation route,
training_step / training_step_views with lambda_sky > 0 against the float64 chain of tests/step_ref.py (+ the sky term's own chain,
tests/alpha_ref.sky_step: by linearity the gradients add) on the bar of tests/test_step_gradients_gpu.py, lambda_sky = 0 launching
nothing new, and evaluate_video's three new keys byte for byte against the numpy restatement of utils/video_utils.py:461-489."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import alpha_ref as R
from tests import step_ref as sr
from tests import step_ref_views as srv
from tests.util import library_route

pytestmark = pytest.mark.gpu
PIPE = dict(convert_SHs_python=True, compute_cov3D_python=False, debug=False)
SMALL = dict(grid_dimensions=2, input_coordinate_dim=4, output_coordinate_dim=32, resolution=[8, 8, 8, 5])
LAMBDA_SKY = 0.05
LOSS_BAR = sr.BAR_MARGIN * sr.LOSS_YARDSTICK_MAX


@pytest.fixture(scope="module")
def scene():
    from s3gaussian_amd import synth
    return synth.street_scene(P=5000, seed=1, width=90, height=61, n_frames=2)


def _model(scn, hyper, dev, opt=None, scale=0.0):
    from s3gaussian_amd.pipeline import GaussianParams
    torch.manual_seed(0)
    pc = GaussianParams(3, hyper)
    gs = scn["gaussians"]
    pc.init_from_tensors(gs["xyz"], gs["log_scales"] + scale, gs["rotations_raw"], gs["opacity_logit"], gs["shs"], dev)
    pc._deformation.deformation_net.set_aabb(*scn["aabb"])
    if opt is not None:
        pc.training_setup(opt)
    return pc


def _cam(scn, i, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in scn["cameras"][i].items()}


ROUTES = {
    "coarse": (dict(), "coarse", False),
    "fine_default": (dict(), "fine", False),
    "no_dx": (dict(no_dx=True), "fine", False),
    "geometry_heads": (dict(no_ds=False, no_dr=False, no_do=False), "fine", False),
    "library": (dict(), "fine", True),
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_render_returns_the_opacity_on_every_route(gpu_device, scene, route):
    from s3gaussian_amd.pipeline import default_hyper, render
    import contextlib
    dev = gpu_device
    over, stage, lib = ROUTES[route]
    pc = _model(scene, default_hyper(kplanes_config=SMALL, **over), dev, scale=1.0)
    pipe = SimpleNamespace(**PIPE)
    cam = _cam(scene, 1, dev)
    H, W = cam["image_height"], cam["image_width"]
    b = torch.tensor([0.3, 0.6, 0.1], device=dev)
    with (library_route(pc) if lib else contextlib.nullcontext()), torch.no_grad():
        plain = render(cam, pc, pipe, b, stage=stage, render_feat=(stage == "fine"))
        assert "alpha" not in plain
        out = render(cam, pc, pipe, b, stage=stage, render_feat=(stage == "fine"), return_alpha=True)      # the pair node in "fine"
        single = render(cam, pc, pipe, b, stage=stage, return_alpha=True)                                  # the single node
        black = render(cam, pc, pipe, torch.zeros(3, device=dev), stage=stage, return_alpha=True)
        over_c = render(cam, pc, pipe, b, stage=stage, override_color=torch.rand(5000, 3, device=dev), return_alpha=True)
    a = out["alpha"]
    assert a.shape == (1, H, W) and float(a.min()) >= 0.0 and float(a.max()) <= 1.0 and 0.01 < float(a.mean()) < 0.999
    for k in ("render", "depth", "radii") + (("feat",) if stage == "fine" else ()):
        assert torch.equal(out[k], plain[k]), k
    assert torch.equal(single["alpha"], a) and torch.equal(black["alpha"], a)
    assert float(((out["render"] - black["render"]) - (1.0 - a) * b.view(3, 1, 1)).abs().max()) <= 1e-4
    assert over_c["alpha"].shape == (1, H, W)
    if stage == "fine" and not lib:
        # evaluation route: full + dynamic + static renders from one geometry, the opacity is the full render's
        with torch.no_grad():
            dec = render(cam, pc, pipe, b, stage=stage, return_decomposition=True, return_alpha=True)
        if "render_d" in dec:
            assert torch.equal(dec["alpha"], a)


def test_render_without_gaussians_gives_zero_opacity(gpu_device, scene):
    from s3gaussian_amd.pipeline import GaussianParams, default_hyper, render
    dev = gpu_device
    pc = GaussianParams(3, default_hyper(kplanes_config=SMALL))
    z = torch.zeros(0, 3)
    pc.init_from_tensors(z, z, torch.zeros(0, 4), torch.zeros(0, 1), torch.zeros(0, 16, 3), dev)
    cam = _cam(scene, 0, dev)
    with torch.no_grad():
        out = render(cam, pc, SimpleNamespace(**PIPE), torch.ones(3, device=dev), stage="coarse", return_alpha=True)
    assert out["alpha"].shape == (1, cam["image_height"], cam["image_width"]) and float(out["alpha"].abs().max()) == 0.0


# ---------------------------------------------------------------- training steps ----------------------------------------------------
def _load(case, dev, lambda_sky):
    from s3gaussian_amd.pipeline import GaussianParams
    L, hyper = case["leaves"], case["hyper"]
    opt = SimpleNamespace(**vars(case["opt"]), lambda_sky=lambda_sky)
    pc = GaussianParams(3, hyper)
    pc.init_from_tensors(L["_xyz"], L["_scaling"], L["_rotation"], L["_opacity"], torch.cat([L["_features_dc"], L["_features_rest"]], 1), dev)
    pc._deformation.load_state_dict(case["state"])
    pc.training_setup(opt)
    return pc, opt


def _check(label, ref, yardstick, got):
    bar = sr.BAR_MARGIN * yardstick
    errs = {k: sr.rel_l2(got["grads"][k], v) for k, v in ref["grads"].items() if v is not None and got["grads"][k] is not None}
    errs.update(got["extra_errs"])
    gap = abs(got["loss"] - ref["loss"]) / abs(ref["loss"])
    print(f"{label}: worst {max(errs.values()):.3e} ({max(errs, key=errs.get)}), bar {bar:.3e}, yardstick {yardstick:.3e}, loss gap {gap:.3e}")
    assert bar <= 1e-4
    assert {k for k, v in got["grads"].items() if v is None} == {k for k, v in ref["grads"].items() if v is None}
    outside = {k: v for k, v in errs.items() if not v <= bar}
    assert not outside, (bar, outside)
    assert gap <= LOSS_BAR, (got["loss"], ref["loss"])


@pytest.mark.parametrize("name", ["loud", "coarse"])
def test_training_step_with_the_sky_term_vs_float64(gpu_device, name):
    """`loud`: the pair node with the fused densify statistics; `coarse`: the single node, statistics by the separate pass."""
    from s3gaussian_amd.pipeline import training_step
    dev = gpu_device
    case = sr.build_case(name)
    mask = R.sky_mask_for(sr.H, sr.W)
    both = lambda dt: R.add_steps(sr.reference_step(case, dt), R.sky_step(case, mask, LAMBDA_SKY, dt))
    r64, r32 = both(torch.float64), both(torch.float32)
    yardstick = max(sr.distances(r32, r64).values())
    plain64 = sr.reference_step(case, torch.float64)
    assert max(sr.distances(plain64, r64).values()) > 100 * sr.BAR_MARGIN * yardstick       # the term is audible on this case
    pc, opt = _load(case, dev, LAMBDA_SKY)
    cam = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in case["camera"].items()}
    gt, gtd, gtf = (t.to(dev) for t in case["targets"])
    params = {n: p for n, p in pc.named_parameters() if p.requires_grad}
    n = lambda t: t.detach().cpu().double().numpy()
    got = {}

    def hook(pc_, pkg):
        got["grads"] = {k: (None if p.grad is None else n(p.grad.clone())) for k, p in params.items()}
        got["viewspace"] = n(pkg["viewspace_points"].grad.clone())

    loss, pkg = training_step(pc, cam, gt, gtd, gtf if case["stage"] == "fine" else None, case["hyper"], opt, case["bg"].to(dev),
                              stage=case["stage"], densify_stats=True, grad_hook=hook, sky_mask=mask.to(dev))
    assert pkg.get("densify_stats_fused", False) == (name == "loud") and "alpha" in pkg
    got["loss"] = float(loss)
    accum, denom, max_radii = sr.densify_stats(r64["dL_dmeans2D"], r64["radii"])
    got["extra_errs"] = {"viewspace": sr.rel_l2(got["viewspace"], r64["dL_dmeans2D"]),
                         "xyz_gradient_accum": sr.rel_l2(n(pc.xyz_gradient_accum), accum)}
    _check(f"sky step {name}", r64, yardstick, got)
    np.testing.assert_array_equal(pkg["radii"].cpu().numpy(), r64["radii"])
    np.testing.assert_array_equal(n(pc.denom), denom)
    np.testing.assert_array_equal(n(pc.max_radii2D), max_radii)


def test_training_step_views_with_the_sky_term_vs_float64(gpu_device):
    """The rig batch (three cameras of one timestamp): the sky term is ONE mean over V*H*W, every view supervised with weight 1/V."""
    from s3gaussian_amd.pipeline import training_step_views
    dev = gpu_device
    case = srv.build_case("rig")
    V = len(case["cameras"])
    masks = [R.sky_mask_for(sr.H, sr.W, seed=v) for v in range(V)]

    def both(dt):
        base = srv.reference_step_views(case, dt)
        sky = [R.sky_step(case, masks[v], LAMBDA_SKY, dt, camera=case["cameras"][v], weight_of_view=1.0 / V) for v in range(V)]
        out = R.add_steps(base, *sky)
        out["dL_dmeans2D_views"] = [b + s["dL_dmeans2D"] for b, s in zip(base["dL_dmeans2D_views"], sky)]
        out["stats"] = srv.densify_stats_views(out["dL_dmeans2D_views"], base["radii"])
        return out

    r64, r32 = both(torch.float64), both(torch.float32)
    yardstick = max(srv.distances(r32, r64).values())
    pc, opt = _load(case, dev, LAMBDA_SKY)
    cams = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in cam.items()} for cam in case["cameras"]]
    gts = [tuple(t.to(dev) for t in tv) for tv in case["targets_views"]]
    params = {n: p for n, p in pc.named_parameters() if p.requires_grad}
    n = lambda t: t.detach().cpu().double().numpy()
    got = {}

    def hook(pc_, pkgs):
        got["grads"] = {k: (None if p.grad is None else n(p.grad.clone())) for k, p in params.items()}
        got["viewspace"] = [n(p["viewspace_points"].grad.clone()) for p in pkgs]

    loss, pkgs = training_step_views(pc, cams, [g[0] for g in gts], [g[1] for g in gts], [g[2] for g in gts], case["hyper"], opt,
                                     case["bg"].to(dev), stage="fine", densify_stats=True, grad_hook=hook,
                                     sky_masks=[m.to(dev) for m in masks])
    assert all("alpha" in p for p in pkgs)
    got["loss"] = float(loss)
    got["extra_errs"] = {f"viewspace[{v}]": sr.rel_l2(g, r) for v, (g, r) in enumerate(zip(got["viewspace"], r64["dL_dmeans2D_views"]))}
    got["extra_errs"]["xyz_gradient_accum"] = sr.rel_l2(n(pc.xyz_gradient_accum), r64["stats"][0])
    _check("sky step views rig", r64, yardstick, got)
    np.testing.assert_array_equal(n(pc.denom), r64["stats"][1])
    np.testing.assert_array_equal(n(pc.max_radii2D), r64["stats"][2])


def test_lambda_sky_zero_launches_nothing_new(gpu_device, monkeypatch):
    from s3gaussian_amd import hexplane, raster_C, sky
    from s3gaussian_amd.pipeline import training_step, training_step_views
    dev = gpu_device
    calls = {"alpha": 0, "backward_alpha": 0, "sky": 0}

    def counted(key, fn):
        def wrapper(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return wrapper

    monkeypatch.setattr(raster_C, "raster_alpha", counted("alpha", raster_C.raster_alpha))
    monkeypatch.setattr(raster_C, "rasterize_gaussians_backward_alpha", counted("backward_alpha", raster_C.rasterize_gaussians_backward_alpha))
    monkeypatch.setattr(sky, "sky_loss_raw", counted("sky", sky.sky_loss_raw))
    case = sr.build_case("default")
    vcase = srv.build_case("rig")
    mask = R.sky_mask_for(sr.H, sr.W).to(dev)
    prev = hexplane.set_deterministic(True)          # the plane gradients' atomics aside, a step is bit-reproducible
    try:
        def one(lambda_sky, **kw):
            pc, opt = _load(case, dev, lambda_sky)
            cam = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in case["camera"].items()}
            gt, gtd, gtf = (t.to(dev) for t in case["targets"])
            loss, _ = training_step(pc, cam, gt, gtd, gtf, case["hyper"], opt, case["bg"].to(dev), densify_stats=True, **kw)
            return [loss] + [p.detach().clone() for p in pc.parameters()] + [pc.xyz_gradient_accum.clone()]

        def views(lambda_sky, **kw):
            pc, opt = _load(vcase, dev, lambda_sky)
            cams = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in cam.items()} for cam in vcase["cameras"]]
            gts = [tuple(t.to(dev) for t in tv) for tv in vcase["targets_views"]]
            loss, _ = training_step_views(pc, cams, [g[0] for g in gts], [g[1] for g in gts], [g[2] for g in gts], vcase["hyper"], opt,
                                          vcase["bg"].to(dev), densify_stats=True, **kw)
            return [loss] + [p.detach().clone() for p in pc.parameters()] + [pc.xyz_gradient_accum.clone()]

        for run, arg in ((one, dict(sky_mask=mask)), (views, dict(sky_masks=[mask] * 3))):
            base = run(0.0)
            off = run(0.0, **arg)                      # the mask is there, the weight is 0
            unused = run(LAMBDA_SKY)                   # the weight is there, no mask
            assert calls == {"alpha": 0, "backward_alpha": 0, "sky": 0}, calls
            for x, y, z in zip(base, off, unused):
                assert torch.equal(x, y) and torch.equal(x, z)
            on = run(LAMBDA_SKY, **arg)
            assert calls["alpha"] > 0 and calls["backward_alpha"] > 0 and calls["sky"] > 0, calls
            assert not torch.equal(on[0], base[0])
            for k in calls:
                calls[k] = 0
    finally:
        hexplane.set_deterministic(prev)


# ---------------------------------------------------------------- evaluate_video ----------------------------------------------------
@pytest.mark.parametrize("W", [96, 90], ids=["W%4==0", "W%4!=0"])
def test_evaluate_video_sky_keys_byte_for_byte(gpu_device, W):
    from s3gaussian_amd import synth
    from s3gaussian_amd.pipeline import default_hyper, evaluate_video, render
    dev = gpu_device
    H = 61
    scn = synth.street_scene(P=3000, seed=4, width=W, height=H, n_frames=2)
    pc = _model(scn, default_hyper(kplanes_config=SMALL), dev, scale=2.0)
    pipe = SimpleNamespace(**PIPE)
    cams = [_cam(scn, i, dev) for i in range(6)]                         # 2 timestamps x 3 cameras
    assert sorted({c["time"] for c in cams}) == [0.0, 1.0] or len({c["time"] for c in cams}) == 2
    bg = torch.tensor([0.1, 0.2, 0.3], device=dev)
    g = torch.Generator().manual_seed(5)
    gts = [torch.rand(3, H, W, generator=g).to(dev) for _ in cams]
    sky_masks = [R.sky_mask_for(H, W, seed=i).to(dev) for i in range(6)]
    with torch.no_grad():
        alphas = [render(c, pc, pipe, bg, return_alpha=True)["alpha"][0].cpu().numpy() for c in cams]
    assert all(0.02 < a.mean() < 0.98 for a in alphas)
    want = R.video_strips(alphas, [m.cpu().numpy() for m in sky_masks], 3)
    res = evaluate_video(pc, cams, gts, pipe, bg, keys=("rgbs",), sky_keys=R.VIDEO_KEYS, sky_masks=sky_masks, compute_metrics=False)
    assert list(res["frames"]) == ["rgbs", *R.VIDEO_KEYS]
    assert res["num_timestamps"] == 2
    for t in range(2):
        assert res["frames"]["opacities"][t].shape == (H, 3 * W, 1)
        assert np.array_equal(res["frames"]["opacities"][t].cpu().numpy()[..., 0], want["opacities"][t])
        for k in ("sky_masks", "gt_sky_masks"):
            assert res["frames"][k][t].shape == (H, 3 * W, 3)
            assert np.array_equal(res["frames"][k][t].cpu().numpy(), want[k][t]), (k, t)
    assert np.array_equal(res["middle"]["sky_masks"].cpu().numpy(), want["sky_masks"][1])
    host = evaluate_video(pc, cams, gts, pipe, bg, keys=(), sky_keys=("sky_masks", "opacities"), compute_metrics=False, host=True)
    assert np.array_equal(host["frames"]["sky_masks"][0], want["sky_masks"][0])
    # with the decomposition and flow keys beside them (the fused evaluation route, render_flows' loop)
    mixed = evaluate_video(pc, cams, gts, pipe, bg, keys=("static_rgbs", "forward_flows"), sky_keys=("opacities",), compute_metrics=False)
    assert np.array_equal(mixed["frames"]["opacities"][1].cpu().numpy()[..., 0], want["opacities"][1])
    with pytest.raises(RuntimeError, match="gt_sky_masks"):
        evaluate_video(pc, cams, gts, pipe, bg, sky_keys=("gt_sky_masks",), compute_metrics=False)
    with pytest.raises(RuntimeError, match="sky_keys"):
        evaluate_video(pc, cams, gts, pipe, bg, keys=("rgbs", "opacities"), compute_metrics=False)      # not a name of keys=
    with pytest.raises(RuntimeError, match="sky_keys"):
        evaluate_video(pc, cams, gts, pipe, bg, sky_keys=("rgbs",), compute_metrics=False)
