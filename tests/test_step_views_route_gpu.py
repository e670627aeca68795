"""Routes of `pipeline.training_step_views` / `render_views`:

  sharing     the deformation field is evaluated once per TIMESTAMP of the batch (deformation.heads_evaluations): `rig` +1 per step
              (+3 with share_deformation=False), `mixed` +2; the shared and the unshared step agree within the case's bar (the
              HexPlane scatter's float atomics forbid bit equality)
  networks    a head subset with geometry heads, a no_dx network and a library-route network (grid_pe) each run a step that agrees
              with V single `render` packages fed to the same loss.  Bar: 1e-4, the cap every per-tensor bar of the step tests is
              held under -- both sides compute the same sums in another order, nothing else
  replay      run_training_steps with V = 3 forwards per iteration: the capacity policy is doctored as in
              tests/test_cfg5_flow_gpu.py::test_an_overflow_after_a_densify_event_is_replayed_not_dropped so that the middle view of
              a batch overflows (the handled overflow); the issued-iteration log shows the rewind and the run ends where runs with
              ample capacity end, at that test's tolerance"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import step_ref as sr
from tests import step_ref_views as srv
from tests.test_step_views_gpu import run_step

pytestmark = pytest.mark.gpu


def _yardstick(name):
    case = srv.build_case(name)
    r64, r32 = srv.reference_step_views(case, torch.float64), srv.reference_step_views(case, torch.float32)
    return case, max(srv.distances(r32, r64).values())


@pytest.mark.parametrize("name,timestamps", [("rig", 1), ("mixed", 2)])
def test_one_deformation_pass_per_timestamp(gpu_device, name, timestamps):
    from s3gaussian_amd import deformation
    case, yard = _yardstick(name)
    V = len(case["cameras"])
    n0 = deformation.heads_evaluations
    shared = run_step(case, gpu_device)
    n1 = deformation.heads_evaluations
    unshared = run_step(case, gpu_device, share_deformation=False)
    n2 = deformation.heads_evaluations
    assert (n1 - n0, n2 - n1) == (timestamps, V)
    bar = sr.BAR_MARGIN * yard
    errs = {k: sr.rel_l2(shared["grads"][k], v) for k, v in unshared["grads"].items() if v is not None}
    errs["xyz_gradient_accum"] = sr.rel_l2(shared["stats"][0], unshared["stats"][0])
    print(f"{name}: shared vs unshared worst {max(errs.values()):.3e} ({max(errs, key=errs.get)}), bar {bar:.3e}")
    assert {k for k, v in shared["grads"].items() if v is None} == {k for k, v in unshared["grads"].items() if v is None}
    assert max(errs.values()) <= bar, errs
    assert abs(shared["loss"] - unshared["loss"]) <= sr.BAR_MARGIN * sr.LOSS_YARDSTICK_MAX * abs(unshared["loss"])
    for a, b in zip(shared["radii"] + list(shared["stats"][1:]), unshared["radii"] + list(unshared["stats"][1:])):
        np.testing.assert_array_equal(a, b)


NETWORKS = {"geometry_heads": (dict(no_dshs=True, feat_head=False, no_ds=False, no_dr=False), True),
            "no_dx": (dict(no_dx=True), True),
            "grid_pe": (dict(grid_pe=2), False)}


@pytest.mark.parametrize("name", sorted(NETWORKS))
def test_other_networks_step_like_single_renders_fed_to_the_same_loss(gpu_device, name):
    from s3gaussian_amd import synth
    from s3gaussian_amd.pipeline import GaussianParams, default_hyper, default_opt, render, training_loss_views, training_step_views
    dev = gpu_device
    over, fused = NETWORKS[name]
    scn = synth.street_scene(P=4001, seed=4, width=128, height=96, n_frames=3)
    hyper, opt = default_hyper(kplanes_config=sr.PLANES["kplanes_config"], **over), default_opt(lambda_dx=0.05, lambda_dshs=0.05)
    gs = scn["gaussians"]
    cams = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in scn["cameras"][i].items()} for i in (3, 4, 5)]
    g = torch.Generator().manual_seed(11)
    gts = [(torch.rand(3, 96, 128, generator=g).to(dev), (60 * torch.rand(1, 96, 128, generator=g)).to(dev),
            torch.rand(3, 96, 128, generator=g).to(dev)) for _ in cams]
    bg = scn["bg"].to(dev)
    pipe = SimpleNamespace(convert_SHs_python=True, compute_cov3D_python=False, debug=False)

    def model():
        torch.manual_seed(0)
        pc = GaussianParams(3, hyper)
        pc.init_from_tensors(gs["xyz"], gs["log_scales"] + 0.9, gs["rotations_raw"], gs["opacity_logit"], gs["shs"], dev)
        pc._deformation.deformation_net.set_aabb(*scn["aabb"])
        with torch.no_grad():        # heads off their zero initialisation, so that every head's gradient is alive
            gen = torch.Generator().manual_seed(2)
            for p in pc._deformation.parameters():
                p.add_((0.05 * torch.randn(p.shape, generator=gen)).to(dev))
        pc.training_setup(opt)
        return pc

    pc = model()
    assert pc._deformation.deformation_net._fused_any() == fused
    got = {}

    def hook(pc_, pkgs):
        got["grads"] = {k: p.grad.clone() for k, p in pc_.named_parameters() if p.grad is not None}

    args = ([t[0] for t in gts], [t[1] for t in gts], [t[2] for t in gts] if hyper.feat_head else None, hyper, opt)
    loss, pkgs = training_step_views(pc, cams, *args, bg, pipe=pipe, grad_hook=hook, densify_stats=True)
    ref = model()
    V = len(cams)
    singles = [render(cam, ref, pipe, bg, stage="fine", return_dx=True, render_feat=bool(hyper.feat_head and v == V - 1))
               for v, cam in enumerate(cams)]
    ref_loss = training_loss_views(ref, singles, *args, stage="fine")
    ref_loss.backward()
    want = {k: p.grad for k, p in ref.named_parameters() if p.grad is not None}
    assert set(got["grads"]) == set(want) and len(want) > 6
    errs = {k: sr.rel_l2(got["grads"][k].cpu().numpy(), v.cpu().numpy()) for k, v in want.items() if float(v.abs().max()) > 0}
    print(f"{name}: worst {max(errs.values()):.3e} ({max(errs, key=errs.get)}), loss {float(loss):.7f} vs {float(ref_loss.detach()):.7f}")
    assert max(errs.values()) <= 1e-4, errs
    assert abs(float(loss) - float(ref_loss.detach())) <= 4e-6 * abs(float(ref_loss.detach()))
    for a, b in zip(pkgs, singles):
        assert torch.equal(a["radii"], b["radii"]) and set(a.keys()) == set(b.keys())
    total = torch.zeros_like(singles[0]["viewspace_points"])
    for p in singles:
        total = total + p["viewspace_points"].grad
    vis = torch.stack([p["radii"] > 0 for p in singles]).any(0)
    accum = torch.where(vis, total[:, :2].norm(dim=1), torch.zeros_like(vis, dtype=torch.float32))
    assert sr.rel_l2(pc.xyz_gradient_accum[:, 0].cpu().numpy(), accum.cpu().numpy()) <= 1e-4
    assert torch.equal(pc.denom[:, 0], vis.float())


def test_an_overflow_in_one_view_of_a_batch_is_replayed_with_the_whole_batch(gpu_device, monkeypatch):
    from s3gaussian_amd import hexplane, raster_C
    from s3gaussian_amd.pipeline import run_training_steps, training_step_views
    from tests.test_cfg5_flow_gpu import _setup
    dev = gpu_device
    batches = ([1, 0, 2], [4, 3, 5])        # a timestamp's cameras, the front one (by far the most instances) in the middle
    res = {}
    for mode in ("ample", "ample_again", "replay"):
        prev_async = raster_C.set_async(True)
        # the HexPlane scatter in its ordered mode: two runs of one procedure then agree far better than the tolerance below (with
        # float atomics their not-close fraction was seen at 2e-4 and at 2.6e-3 between pairs of ample runs, either side of it)
        prev_deterministic = hexplane.set_deterministic(True)
        raster_C._async_states.pop(dev.index or 0, None)
        raster_C.invalidate_geometry_cache()
        try:
            pc, cams, targets, hyper, opt, bg = _setup(dev, P=20_000, W=320, H=208, seed=5)
            losses = {}

            def issue(i):
                b = batches[i % 2]
                loss, _ = training_step_views(pc, [cams[v] for v in b], [targets[v][0] for v in b], [targets[v][1] for v in b],
                                              [targets[v][2] for v in b], hyper, opt, bg, stage="fine", densify_stats=True)
                losses[i] = loss

            log = []
            out1 = run_training_steps(issue, 1, 4, optimizer=pc.optimizer, device=dev, log=log)
            assert out1["rewinds"] == [] and log == [1, 2, 3, 4]
            torch.cuda.synchronize()
            first_forward = raster_C.async_issued(dev)
            if mode == "replay":
                st = raster_C._async_state(dev)
                st.drain(block=True)
                key = (320, 208)
                true_R = st.hist[key][0]                                    # the front camera's
                monkeypatch.setattr(raster_C, "_ASYNC_MIN_INSTANCES", 1)
                st.hist[key] = [true_R // 8, true_R // 8, st.hist[key][2]]   # 4 x headroom = half the front camera's count
                assert st.caps(key)[0] < true_R
            log = []
            out2 = run_training_steps(issue, 5, 8, optimizer=pc.optimizer, device=dev, log=log)
            torch.cuda.synchronize()
            if mode == "replay":
                stt = raster_C.async_status(dev, block=True)
                print("replay:", out2, "issue order:", log, "overflowed forwards:", stt["overflows"], "frozen:", stt["frozen"],
                      "first forward of the segment:", first_forward)
                assert len(out2["rewinds"]) >= 1 and out2["rewinds"][0][0] == 5, out2      # iteration 5's batch was re-issued
                assert log[0] == 5 and log.count(5) >= 2 and log[-1] == 8 and out2["issued"] == len(log) > 4
                assert stt["overflows"] and stt["overflows"][0] == first_forward + 1      # the batch's MIDDLE view overflowed
                assert first_forward + 2 in stt["frozen"]                                 # ... and froze the view after it
                assert int(raster_C._async_state(dev).sticky_dev.item()) == 0             # thawed
            else:
                assert out2["rewinds"] == [] and log == [5, 6, 7, 8]
            assert all(float(s["step"]) == 8.0 for s in pc.optimizer.state.values() if "step" in s)      # ONE Adam step per batch
            res[mode] = dict(losses=[float(losses[i]) for i in range(1, 9)], params={n: p.detach().clone() for n, p in pc.named_parameters()},
                             denom=pc.denom.clone(), accum=pc.xyz_gradient_accum.clone(), max_radii=pc.max_radii2D.clone())
        finally:
            raster_C.set_async(prev_async)
            hexplane.set_deterministic(prev_deterministic)
            raster_C._async_states.pop(dev.index or 0, None)
            raster_C.invalidate_geometry_cache()

    def distance(a, b):
        ta, tb = dict(a["params"], xyz_gradient_accum=a["accum"]), dict(b["params"], xyz_gradient_accum=b["accum"])
        frac = max(float((~torch.isclose(ta[n], tb[n], rtol=1e-4, atol=1e-6)).float().mean()) for n in ta)
        lrel = max(abs(x - y) / abs(x) for x, y in zip(a["losses"], b["losses"]))
        return frac, lrel

    floor = distance(res["ample"], res["ample_again"])
    got = distance(res["ample"], res["replay"])
    print("not-close fraction / max relative loss difference: ample vs ample", floor, " ample vs replay", got)
    assert got[0] <= max(2e-3, 3 * floor[0]) and got[1] <= max(1e-4, 3 * floor[1]), (got, floor)
    assert torch.equal(res["ample"]["denom"], res["replay"]["denom"]) and float(res["replay"]["denom"].sum()) > 0
    assert torch.equal(res["ample"]["max_radii"], res["replay"]["max_radii"])
