"""One `pipeline.training_step` on the GPU against the float64 reference chain of tests/step_ref.py, tensor by tensor.

The step is what bench.py times; its gradients were so far compared with an independent route only after Adam (PSNR parity, which
a gradient off by a constant factor or short of a small additive term passes) or with the step's own other routes.  Here the
`.grad` of every parameter, captured by `grad_hook` between backward and the optimizer step, is compared with the derivative the
reference's algorithm gives in double precision:

  per tensor   rel_l2(gpu, float64) <= 4 x the largest distance of the float32 chain from the float64 chain over the case's tensors
               (the yardstick; computed here from the reference alone, <= 1e-4 by tests/test_step_gradients_cpu.py).  The margin of 4
               covers the GPU's own exp / rcp, the order of atomic sums and the bf16x3 chains; the smallest wrong reading of a seam
               moves a tensor of `loud` by more than 600 bars (test_step_gradients_cpu.py).
  connection   a parameter has no gradient exactly where the reference gives none (coarse stage: the whole deformation network)
  viewspace    pkg["viewspace_points"].grad against the two raster passes' summed dL_dmeans2D, same bar
  statistics   xyz_gradient_accum on the same bar; denom, max_radii2D and radii exactly
  loss         within step_ref.LOSS_BAR of the float64 loss (how that bar is formed: step_ref.py), which is at most a tenth of the
               smallest loss shift a wrong reading causes (asserted in test_step_gradients_cpu.py, where they are evaluated)
  step size    after the step max|delta p| of every tensor is its group's learning rate (scene/gaussian_model.py:177-189): the first
               bias-corrected Adam step moves an element with |g| >> eps by lr * g / (|g| + eps).  Tolerance: 1e-4 lr for the fp32
               bias correction 1 - 0.999 (relative rounding 2^-24 / 1e-3 = 6e-5, halved by the square root, plus the update's own
               roundings) and one ulp of the largest |p| for the rounding of the stored parameter.  A parameter without a gradient
               does not move.

Every measured number goes to step_ref.RECORD (committed copy of a run: profiles/step_gradient_parity.jsonl)."""
import numpy as np
import pytest
import torch

from tests import step_ref as sr

pytestmark = pytest.mark.gpu
F32_EPS = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def reference():
    """(case, float64 result, {tensor: float32-chain distance}) per (case name, scale modifier), evaluated once."""
    cache = {}

    def get(name, scale_modifier=1.0):
        key = (name, scale_modifier)
        if key not in cache:
            case = sr.build_case(name)
            if scale_modifier != 1.0:
                case["scale_modifier"] = scale_modifier
            r64 = sr.reference_step(case, torch.float64)
            cache[key] = (case, r64, sr.distances(sr.reference_step(case, torch.float32), r64))
        return cache[key]

    return get


def _learning_rate(name, opt):
    leaf = {"_xyz": opt.position_lr_init, "_features_dc": opt.feature_lr, "_features_rest": opt.feature_lr / 20.0,
            "_opacity": opt.opacity_lr, "_scaling": opt.scaling_lr, "_rotation": opt.rotation_lr}
    if name in leaf:
        return leaf[name]
    return opt.grid_lr_init if "grid" in name else opt.deformation_lr_init


def _run(case, dev, through_step=True):
    """The product's step on a model loaded with the case's state -> everything the checks read, on the host."""
    from types import SimpleNamespace
    from s3gaussian_amd.pipeline import GaussianParams, render, training_loss, training_step
    L, opt, hyper = case["leaves"], case["opt"], case["hyper"]
    pc = GaussianParams(3, hyper)
    pc.init_from_tensors(L["_xyz"], L["_scaling"], L["_rotation"], L["_opacity"], torch.cat([L["_features_dc"], L["_features_rest"]], 1), dev)
    pc._deformation.load_state_dict(case["state"])
    pc.training_setup(opt)
    cam = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in case["camera"].items()}
    gt, gtd, gtf = (t.to(dev) for t in case["targets"])
    bg = case["bg"].to(dev)
    params = {n: p for n, p in pc.named_parameters() if p.requires_grad}
    n = lambda t: t.detach().cpu().double().numpy()
    got = dict(before={k: n(p) for k, p in params.items()})

    def hook(pc_, pkg):
        got["grads"] = {k: (None if p.grad is None else n(p.grad.clone())) for k, p in params.items()}
        vg = pkg["viewspace_points"].grad
        got["viewspace"] = None if vg is None else n(vg.clone())

    if through_step:
        loss, pkg = training_step(pc, cam, gt, gtd, gtf if case["stage"] == "fine" else None, hyper, opt, bg, stage=case["stage"],
                                  densify_stats=True, grad_hook=hook)
        got["after"] = {k: n(p) for k, p in params.items()}
        got["stats"] = (n(pc.xyz_gradient_accum), n(pc.denom), n(pc.max_radii2D))
    else:       # training_step takes no scaling modifier: its three stages called directly
        pipe = SimpleNamespace(convert_SHs_python=True, compute_cov3D_python=False, debug=False)
        pkg = render(cam, pc, pipe, bg, scaling_modifier=case["scale_modifier"], stage=case["stage"], return_dx=True, render_feat=True)
        loss = training_loss(pc, pkg, gt, gtd, gtf, hyper, opt, case["stage"])
        loss.backward()
        hook(pc, pkg)
    got["loss"] = float(loss.detach())
    got["radii"] = pkg["radii"].cpu().numpy()
    return got


def _check(label, config, case, r64, yard, got):
    opt = case["opt"]
    yardstick = max(yard.values())
    bar = sr.BAR_MARGIN * yardstick
    ref = r64["grads"]
    errs = {k: sr.rel_l2(got["grads"][k], v) for k, v in ref.items() if v is not None and got["grads"][k] is not None}
    if got["viewspace"] is not None:
        errs["viewspace"] = sr.rel_l2(got["viewspace"], r64["dL_dmeans2D"])
    loss_gap = abs(got["loss"] - r64["loss"]) / abs(r64["loss"])
    row = dict(test="gpu_step", case=label, config=config, yardstick=yardstick, bar=bar, worst=max(errs.values()),
               worst_tensor=max(errs, key=errs.get), per_tensor=errs, loss_gpu=got["loss"], loss_f64=r64["loss"], rel_loss_gap=loss_gap,
               loss_bar=sr.LOSS_BAR[label])
    if "stats" in got:
        accum, denom, max_radii = sr.densify_stats(r64["dL_dmeans2D"], r64["radii"])
        row["xyz_gradient_accum"] = sr.rel_l2(got["stats"][0], accum)
        steps = {}
        for k, v in ref.items():
            delta = float(np.abs(got["after"][k] - got["before"][k]).max())
            steps[k] = delta / _learning_rate(k, opt)
        row["max_step_over_lr"] = steps
    print(f"{label} {config}: worst {row['worst']:.3e} ({row['worst_tensor']}), bar {bar:.3e}, yardstick {yardstick:.3e}, "
          f"loss gap {loss_gap:.3e} (bar {sr.LOSS_BAR[label]:.3e})")
    sr.record(row)
    assert bar <= 1e-4
    # no disconnected and no extra parameter
    assert {k for k, v in got["grads"].items() if v is None} == {k for k, v in ref.items() if v is None}
    assert set(got["grads"]) == set(ref)
    assert got["viewspace"] is not None and errs["viewspace"] <= bar, errs["viewspace"]
    outside = {k: v for k, v in errs.items() if not v <= bar}
    assert not outside, (bar, outside)
    np.testing.assert_array_equal(got["radii"], r64["radii"])
    assert loss_gap <= sr.LOSS_BAR[label], (got["loss"], r64["loss"])
    if "stats" in got:
        assert row["xyz_gradient_accum"] <= bar
        np.testing.assert_array_equal(got["stats"][1], denom)
        np.testing.assert_array_equal(got["stats"][2], max_radii)
        for k, v in ref.items():
            lr, before = _learning_rate(k, opt), got["before"][k]
            delta = float(np.abs(got["after"][k] - before).max())
            if v is None:
                assert delta == 0.0, k
            else:
                assert np.abs(v).max() > 1e-9, k         # |g| >> eps = 1e-15 somewhere in the tensor
                assert abs(delta - lr) <= 1e-4 * lr + F32_EPS * float(np.abs(before).max()), (k, delta, lr)


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("arithmetic", ["f32", "bf16x3"])
def test_loud_step_gradients_vs_float64(gpu_device, reference, arithmetic, deterministic):
    """Every seam at weights that make it audible, under both arithmetics of the MLP chains and both HexPlane backward modes."""
    from s3gaussian_amd import hexplane, mlp
    case, r64, yard = reference("loud")
    prev_arithmetic, prev_deterministic = mlp.get_mlp_arithmetic(), hexplane.set_deterministic(deterministic)
    try:
        mlp.set_mlp_arithmetic(arithmetic)
        got = _run(case, gpu_device)
    finally:
        mlp.set_mlp_arithmetic(prev_arithmetic)
        hexplane.set_deterministic(prev_deterministic)
    _check("loud", f"{arithmetic}, deterministic={deterministic}", case, r64, yard, got)


@pytest.mark.parametrize("name", ["default", "coarse"])
def test_step_gradients_vs_float64(gpu_device, reference, name):
    """The reference's default weights (what bench.py runs) and the coarse stage (one image, no deformation, statistics by the
    separate pass), at the default arithmetic and HexPlane mode."""
    from s3gaussian_amd import mlp
    case, r64, yard = reference(name)
    got = _run(case, gpu_device)
    _check(name, f"{mlp.get_mlp_arithmetic()}, defaults", case, r64, yard, got)


def test_loud_gradients_with_scaling_modifier_vs_float64(gpu_device, reference):
    """scale_modifier = 1.7 through render -> training_loss -> backward: the modifier passes the two-image node forward and
    backward (dL/dscales carries it) and every seam of the step behind it."""
    case, r64, yard = reference("loud", 1.7)
    base = reference("loud")[1]
    assert r64["num_rendered"] > 1.3 * base["num_rendered"]          # the modifier does something on this scene
    got = _run(case, gpu_device, through_step=False)
    _check("loud_scale_1.7", "render + training_loss, scaling_modifier=1.7", case, r64, yard, got)
