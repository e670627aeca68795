"""The sky colour model through the pipeline: render(sky_model=) against the stand-alone calls, one training step against the float64
chain of the composite on the same render_fg / alpha, the "sky_model" param group through a densify and a prune, the camera loops
(render_views, evaluate, evaluate_video) frame by frame against single renders, and the refusals."""
from types import SimpleNamespace

import pytest
import torch

from tests import alpha_ref as A
from tests import skymodel_ref as R
from tests import step_ref as sr

pytestmark = pytest.mark.gpu
PIPE = dict(convert_SHs_python=True, compute_cov3D_python=False, debug=False)
SMALL = dict(grid_dimensions=2, input_coordinate_dim=4, output_coordinate_dim=32, resolution=[8, 8, 8, 5])
SIZES = ((37, 53), (64, 48))         # H, W of the two camera sets of the loop test
P = 3000


def _scene(H, W):
    from s3gaussian_amd import synth
    return synth.street_scene(P=P, seed=2, width=W, height=H, n_frames=3)


@pytest.fixture(scope="module")
def scenes():
    return {hw: _scene(*hw) for hw in SIZES + ((30, 40),)}


def _pc(scn, dev, opt=None, **hyper):
    from s3gaussian_amd.pipeline import GaussianParams, default_hyper
    torch.manual_seed(0)
    pc = GaussianParams(3, default_hyper(kplanes_config=SMALL, **hyper))
    gs = scn["gaussians"]
    pc.init_from_tensors(gs["xyz"], gs["log_scales"] + 1.0, gs["rotations_raw"], gs["opacity_logit"], gs["shs"], dev)
    pc._deformation.deformation_net.set_aabb(*scn["aabb"])
    if opt is not None:
        pc.training_setup(opt)
    return pc


def _cam(scn, i, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in scn["cameras"][i].items()}


def _sky(dev, seed=4):
    from s3gaussian_amd import skymodel
    torch.manual_seed(seed)
    return skymodel.SkyModel().to(dev)


def test_render_equals_the_stand_alone_calls(gpu_device, scenes):
    from s3gaussian_amd import skymodel
    from s3gaussian_amd.pipeline import render
    dev = gpu_device
    scn = scenes[SIZES[0]]
    pc, m, pipe = _pc(scn, dev), _sky(dev), SimpleNamespace(**PIPE)
    cam = _cam(scn, 1, dev)
    bg = torch.tensor([0.3, 0.6, 0.1], device=dev)                 # not used with a sky model
    with torch.no_grad():
        out = render(cam, pc, pipe, bg, sky_model=m)
        black = render(cam, pc, pipe, torch.zeros(3, device=dev), return_alpha=True)
        sky = skymodel.sky_image(m, cam)
        plain = render(cam, pc, pipe, bg)
    assert "render_fg" not in plain and "alpha" not in plain
    assert torch.equal(out["render_fg"], black["render"]) and torch.equal(out["alpha"], black["alpha"])
    assert 0.02 < float(out["alpha"].mean()) < 0.98
    assert torch.equal(out["render"], out["render_fg"] + (1.0 - out["alpha"]) * sky)
    assert torch.equal(out["depth"], plain["depth"]) and torch.equal(out["radii"], plain["radii"])


def test_training_step_moves_the_sky_model_and_matches_float64(gpu_device, scenes):
    """Stage "coarse" with the DSSIM and depth weights at 0: loss = mean|composite - gt| + lambda_sky * the sky cross entropy, a chain
    the restatements cover end to end from the step's own render_fg and alpha."""
    from s3gaussian_amd.pipeline import default_opt, training_step
    dev = gpu_device
    H, W = SIZES[0]
    scn = scenes[SIZES[0]]
    lam = 0.05
    opt = default_opt(lambda_dssim=0.0, lambda_depth=0.0, lambda_sky=lam)
    pc = _pc(scn, dev, opt)
    m = _sky(dev)
    cam = _cam(scn, 0, dev)
    g = torch.Generator().manual_seed(9)
    gt = torch.rand(3, H, W, generator=g)
    mask = A.sky_mask_for(H, W)
    hyper = pc._deformation.deformation_net.args
    with pytest.raises(RuntimeError, match="not attached"):
        training_step(pc, cam, gt.to(dev), None, None, hyper, opt, torch.zeros(3, device=dev), stage="coarse", sky_model=m,
                      sky_mask=mask.to(dev))
    pc.attach_sky_model(m)
    before = [t.detach().clone() for t in m.tensors()]
    got = {}

    def hook(pc_, pkg):
        got["grads"] = [t.grad.detach().clone() for t in m.tensors()]

    loss, pkg = training_step(pc, cam, gt.to(dev), torch.zeros(1, H, W, device=dev), None, hyper, opt, torch.ones(3, device=dev),
                              stage="coarse", sky_model=m, sky_mask=mask.to(dev), grad_hook=hook)
    torch.cuda.synchronize()
    assert all(t.grad is None for t in m.tensors())                # cleared with the optimizer's other groups
    for b, t in zip(before, m.tensors()):
        assert not torch.equal(b, t.detach())                      # every tensor of the model moved
    fg, alpha = pkg["render_fg"].detach().cpu(), pkg["alpha"].detach().cpu()
    camrec = (cam["viewmatrix"][:3, :3].cpu(), W / (2.0 * cam["tanfovx"]), H / (2.0 * cam["tanfovy"]), W / 2.0, H / 2.0)

    def chain(dtype):
        w = [b.cpu().to(dtype).requires_grad_(True) for b in before]
        img = R.composite(w, *camrec, fg.to(dtype), alpha.to(dtype))
        sky_loss, _ = A.sky_loss_ref(alpha, mask, dtype)
        total = (img - gt.to(dtype)).abs().mean() + lam * float(sky_loss)
        total.backward()
        return float(total.detach()), [t.grad for t in w]

    l64, g64 = chain(torch.float64)
    l32, g32 = chain(torch.float32)
    gap, yard = abs(float(loss) - l64) / abs(l64), abs(l32 - l64) / abs(l64)
    print(f"sky training step: loss {float(loss):.8f} float64 {l64:.8f} gap {gap:.3e} (float32 chain {yard:.3e})")
    assert yard <= sr.LOSS_YARDSTICK_MAX
    assert gap <= sr.BAR_MARGIN * sr.LOSS_YARDSTICK_MAX
    for name, a, t, y in zip(("dW0", "db0", "dW1", "db1", "dW2", "db2"), got["grads"], g64, g32):
        d, dy = R.rel_l2(a, t), R.rel_l2(y, t)
        print(f"  {name}: gpu {d:.3e} yardstick {dy:.3e}")
        assert d <= sr.BAR_MARGIN * dy, (name, d, dy)


def test_densify_and_prune_leave_the_sky_group_intact(gpu_device, scenes):
    from s3gaussian_amd import skymodel
    from s3gaussian_amd.pipeline import default_opt, training_step
    dev = gpu_device
    H, W = SIZES[0]
    scn = scenes[SIZES[0]]
    opt = default_opt()
    pc = _pc(scn, dev, opt)
    m = pc.attach_sky_model(_sky(dev))
    cam = _cam(scn, 0, dev)
    hyper = pc._deformation.deformation_net.args
    g = torch.Generator().manual_seed(3)
    training_step(pc, cam, torch.rand(3, H, W, generator=g).to(dev), torch.rand(1, H, W, generator=g).to(dev) * 50, None, hyper, opt,
                  torch.zeros(3, device=dev), stage="coarse", sky_model=m, densify_stats=True)
    group = skymodel.attached_group(pc.optimizer, m)
    assert group is not None

    def snapshot():
        return [(id(p), p.detach().clone(), {k: (v.clone() if torch.is_tensor(v) else v) for k, v in pc.optimizer.state[p].items()})
                for p in group["params"]]

    snap = snapshot()
    assert all("exp_avg" in st and float(st["exp_avg"].abs().max()) > 0 for _, _, st in snap)
    out = pc.densify(1e-12, 0.005, 100.0, None, seed=1)
    assert out["clone"] + out["split"] > 0 and pc._xyz.shape[0] == out["P"] > P
    out = pc.prune(0.0002, 0.5, 100.0, None)
    assert out["drop"] > 0 and pc._xyz.shape[0] == out["P"]
    assert skymodel.attached_group(pc.optimizer, m) is group and group["name"] == "sky_model" and group["lr"] == 0.0025
    for (pid, value, state), (pid2, value2, state2) in zip(snap, snapshot()):
        assert pid == pid2 and torch.equal(value, value2) and state.keys() == state2.keys()
        for k, v in state.items():
            assert torch.equal(v, state2[k]) if torch.is_tensor(v) else v == state2[k], k
    # and the model still trains with the new Gaussians
    before = m.tensors()[0].detach().clone()
    training_step(pc, cam, torch.rand(3, H, W, generator=g).to(dev), torch.rand(1, H, W, generator=g).to(dev) * 50, None, hyper, opt,
                  torch.zeros(3, device=dev), stage="coarse", sky_model=m)
    assert not torch.equal(before, m.tensors()[0].detach())


def test_camera_loops_frame_by_frame(gpu_device, scenes):
    """Six cameras alternating between two image sizes through render_views, evaluate and evaluate_video, after plain renders at a
    third size in the same process: every frame equals the single-camera render(sky_model=) of its camera."""
    from s3gaussian_amd.pipeline import evaluate, evaluate_video, render, render_views
    from s3gaussian_amd import frames, metrics
    dev = gpu_device
    pipe = SimpleNamespace(**PIPE)
    pc, m = _pc(scenes[SIZES[0]], dev), _sky(dev)
    bg = torch.tensor([0.2, 0.4, 0.6], device=dev)
    with torch.no_grad():
        for i in range(3):
            render(_cam(scenes[(30, 40)], i, dev), pc, pipe, bg)
    cams = [_cam(scenes[SIZES[i % 2]], i, dev) for i in range(6)]
    assert [(c["image_height"], c["image_width"]) for c in cams] == [SIZES[i % 2] for i in range(6)]
    g = torch.Generator().manual_seed(1)
    gts = [torch.rand(3, c["image_height"], c["image_width"], generator=g).to(dev) for c in cams]
    with torch.no_grad():
        single = [render(c, pc, pipe, bg, sky_model=m) for c in cams]
        views = render_views(cams, pc, pipe, bg, sky_model=m)
    for s, v in zip(single, views):
        for k in ("render", "render_fg", "alpha"):
            assert torch.equal(s[k], v[k]), k
    assert any(float((s["render"] - s["render_fg"]).abs().max()) > 0.05 for s in single)       # the sky is visible in them
    res = evaluate(pc, cams, gts, pipe, bg, sky_model=m)
    want = torch.empty((6, metrics.RECORD), dtype=torch.float64, device=dev)
    for i, s in enumerate(single):
        metrics.image_metrics(s["render"], gts[i], None, out=want[i])
    same = lambda a, b: torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))    # no mask: the masked columns are NaN
    assert same(res["per_frame"], want.cpu())
    vid = evaluate_video(pc, cams, gts, pipe, bg, num_cams=1, keys=("rgbs",), sky_model=m)
    assert same(vid["per_frame"], want.cpu()) and vid["num_timestamps"] == 6
    for i, s in enumerate(single):
        strip = vid["frames"]["rgbs"][i]
        H, W = SIZES[i % 2]
        assert strip.shape == (H, W, 3)
        want_strip = frames.compose(s["render"], torch.empty(frames.strip_shape(H, W, 3, 1), dtype=torch.uint8, device=dev), 0)
        assert torch.equal(strip, want_strip)
    torch.cuda.synchronize()


def test_refusals(gpu_device, scenes):
    from s3gaussian_amd.pipeline import evaluate_video, render, training_step, default_opt
    dev = gpu_device
    scn = scenes[SIZES[0]]
    opt = default_opt()
    pc, m, pipe = _pc(scn, dev, opt), _sky(dev), SimpleNamespace(**PIPE)
    cam = _cam(scn, 0, dev)
    bg = torch.zeros(3, device=dev)
    with pytest.raises(RuntimeError, match=r"render\(sky_model=..., pose=...\)"):
        render(cam, pc, pipe, bg, sky_model=m, pose=object(), cam_index=0)
    with pytest.raises(RuntimeError, match=r"render\(sky_model=..., override_color=...\)"):
        render(cam, pc, pipe, bg, sky_model=m, override_color=torch.rand(P, 3, device=dev))
    with pytest.raises(RuntimeError, match=r"evaluate_video\(sky_model=..., pose=...\)"):
        evaluate_video(pc, [cam], [torch.rand(3, *SIZES[0], device=dev)], pipe, bg, num_cams=1, sky_model=m, pose=object())
    pc.attach_sky_model(m)
    with pytest.raises(RuntimeError, match=r"training_step\(sky_model=..., pose=...\)"):
        training_step(pc, cam, None, None, None, pc._deformation.deformation_net.args, opt, bg, sky_model=m, pose=object(), cam_index=0)
    from s3gaussian_amd import skymodel
    with pytest.raises(NotImplementedError, match="mlp_width"):
        skymodel.SkyModel({"mlp_width": 128})
