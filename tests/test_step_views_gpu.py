"""One `pipeline.training_step_views` on the GPU against the float64 reference chain of tests/step_ref_views.py, tensor by
tensor, the way tests/test_step_gradients_gpu.py checks `training_step`:

  per tensor   rel_l2(gpu, float64) <= BAR_MARGIN x the case's yardstick (the float32 chain's largest distance from the float64
               chain, from the reference alone; <= step_ref.YARDSTICK_MAX by tests/test_step_views_cpu.py), asserted <= 1e-4.  The
               smallest wrong reading of a batch seam moves a tensor by more than 600 bars (test_step_views_cpu.py).
  connection   a parameter has no gradient exactly where the reference gives none
  viewspace    every view's pkg["viewspace_points"].grad against that view's raster passes, same bar
  statistics   xyz_gradient_accum (norm of the SUMMED viewspace gradient) on the same bar; denom, max_radii2D and every view's radii
               exactly
  loss         within BAR_MARGIN x LOSS_YARDSTICK_MAX of the float64 loss: the bound on the float32 chain's own loss distance
               (asserted for these cases in test_step_views_cpu.py), as step_ref.LOSS_BAR is formed
  step size    after the ONE Adam step max|delta p| of every tensor is its group's learning rate, at test_step_gradients_gpu.py's
               tolerance; a parameter without a gradient does not move

Cases: rig (3 cameras of one timestamp: one deformation pass), mixed (2 timestamps: "the last view" matters), coarse; and
feat_views="all" on rig against the helper's corresponding variant.  Measured numbers go through step_ref.record (committed copy
of a run: profiles/step_views_parity.jsonl)."""
import numpy as np
import pytest
import torch

from tests import step_ref as sr
from tests import step_ref_views as srv
from tests.test_step_gradients_gpu import F32_EPS, _learning_rate

pytestmark = pytest.mark.gpu
LOSS_BAR = sr.BAR_MARGIN * sr.LOSS_YARDSTICK_MAX


@pytest.fixture(scope="module")
def reference():
    """(case, float64 result, yardstick) per (case name, feat_views), evaluated once."""
    cache = {}

    def get(name, feat_views="last"):
        key = (name, feat_views)
        if key not in cache:
            case = srv.build_case(name)
            r64 = srv.reference_step_views(case, torch.float64, feat_views=feat_views)
            r32 = srv.reference_step_views(case, torch.float32, feat_views=feat_views)
            cache[key] = (case, r64, max(srv.distances(r32, r64).values()))
        return cache[key]

    return get


def run_step(case, dev, feat_views="last", share_deformation=True):
    """The product's batch step on a model loaded with the case's state -> everything the checks read, on the host."""
    from s3gaussian_amd.pipeline import GaussianParams, training_step_views
    L, opt, hyper = case["leaves"], case["opt"], case["hyper"]
    pc = GaussianParams(3, hyper)
    pc.init_from_tensors(L["_xyz"], L["_scaling"], L["_rotation"], L["_opacity"], torch.cat([L["_features_dc"], L["_features_rest"]], 1), dev)
    pc._deformation.load_state_dict(case["state"])
    pc.training_setup(opt)
    cams = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in cam.items()} for cam in case["cameras"]]
    gts = [tuple(t.to(dev) for t in tv) for tv in case["targets_views"]]
    params = {n: p for n, p in pc.named_parameters() if p.requires_grad}
    n = lambda t: t.detach().cpu().double().numpy()
    got = dict(before={k: n(p) for k, p in params.items()})

    def hook(pc_, pkgs):
        assert isinstance(pkgs, list) and len(pkgs) == len(cams)
        got["grads"] = {k: (None if p.grad is None else n(p.grad.clone())) for k, p in params.items()}
        got["viewspace"] = [None if p["viewspace_points"].grad is None else n(p["viewspace_points"].grad.clone()) for p in pkgs]

    fine = case["stage"] == "fine"
    loss, pkgs = training_step_views(pc, cams, [g[0] for g in gts], [g[1] for g in gts], [g[2] for g in gts] if fine else None,
                                     hyper, opt, case["bg"].to(dev), stage=case["stage"], densify_stats=True, grad_hook=hook,
                                     feat_views=feat_views, share_deformation=share_deformation)
    got["after"] = {k: n(p) for k, p in params.items()}
    got["stats"] = (n(pc.xyz_gradient_accum), n(pc.denom), n(pc.max_radii2D))
    got["loss"] = float(loss)
    got["radii"] = [p["radii"].cpu().numpy() for p in pkgs]
    got["has_feat"] = ["feat" in p for p in pkgs]
    return got


def check(label, config, case, r64, yardstick, got):
    opt = case["opt"]
    bar = sr.BAR_MARGIN * yardstick
    ref = r64["grads"]
    errs = {k: sr.rel_l2(got["grads"][k], v) for k, v in ref.items() if v is not None and got["grads"][k] is not None}
    for v, (g, r) in enumerate(zip(got["viewspace"], r64["dL_dmeans2D_views"])):
        if g is not None:
            errs[f"viewspace[{v}]"] = sr.rel_l2(g, r)
    errs["xyz_gradient_accum"] = sr.rel_l2(got["stats"][0], r64["stats"][0])
    loss_gap = abs(got["loss"] - r64["loss"]) / abs(r64["loss"])
    steps = {k: float(np.abs(got["after"][k] - got["before"][k]).max()) / _learning_rate(k, opt) for k in ref}
    row = dict(test="gpu_step_views", case=label, config=config, views=list(case["views"]), yardstick=yardstick, bar=bar,
               worst=max(errs.values()), worst_tensor=max(errs, key=errs.get), per_tensor=errs, loss_gpu=got["loss"],
               loss_f64=r64["loss"], rel_loss_gap=loss_gap, loss_bar=LOSS_BAR, max_step_over_lr=steps)
    print(f"{label} {config}: worst {row['worst']:.3e} ({row['worst_tensor']}), bar {bar:.3e}, yardstick {yardstick:.3e}, "
          f"loss gap {loss_gap:.3e} (bar {LOSS_BAR:.3e})")
    sr.record(row)
    assert bar <= 1e-4
    assert {k for k, v in got["grads"].items() if v is None} == {k for k, v in ref.items() if v is None}
    assert set(got["grads"]) == set(ref)
    assert all(g is not None for g in got["viewspace"])
    outside = {k: v for k, v in errs.items() if not v <= bar}
    assert not outside, (bar, outside)
    for a, b in zip(got["radii"], r64["radii"]):
        np.testing.assert_array_equal(a, b)
    assert loss_gap <= LOSS_BAR, (got["loss"], r64["loss"])
    np.testing.assert_array_equal(got["stats"][1], r64["stats"][1])
    np.testing.assert_array_equal(got["stats"][2], r64["stats"][2])
    for k, v in ref.items():
        lr, before = _learning_rate(k, opt), got["before"][k]
        delta = float(np.abs(got["after"][k] - before).max())
        if v is None:
            assert delta == 0.0, k
        else:
            assert np.abs(v).max() > 1e-9, k         # |g| >> eps = 1e-15 somewhere in the tensor
            assert abs(delta - lr) <= 1e-4 * lr + F32_EPS * float(np.abs(before).max()), (k, delta, lr)


@pytest.mark.parametrize("name", ["rig", "mixed", "coarse"])
def test_batch_step_gradients_vs_float64(gpu_device, reference, name):
    from s3gaussian_amd import mlp
    case, r64, yard = reference(name)
    got = run_step(case, gpu_device)
    V = len(case["cameras"])
    # feat_views="last": only the last view rasterizes a feature image (none in the coarse stage)
    assert got["has_feat"] == [case["stage"] == "fine" and v == V - 1 for v in range(V)]
    check(name, f"{mlp.get_mlp_arithmetic()}, feat_views=last", case, r64, yard, got)


def test_rig_step_with_every_feature_image_supervised(gpu_device, reference):
    from s3gaussian_amd import mlp
    case, r64, yard = reference("rig", "all")
    got = run_step(case, gpu_device, feat_views="all")
    assert got["has_feat"] == [True, True, True]
    check("rig", f"{mlp.get_mlp_arithmetic()}, feat_views=all", case, r64, yard, got)
