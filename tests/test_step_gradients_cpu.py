"""The checker of tests/test_step_gradients_gpu.py, checked: how far the float64 reference chain of one training step
(tests/step_ref.py) can be trusted, and whether the bar derived from it would notice a wrong seam.  No GPU.

  yardstick   float32 chain against float64 chain, per gradient tensor and case: at most step_ref.YARDSTICK_MAX = 2.5e-5, so that the
              GPU bar (4 x the case's largest) stays at or below 1e-4, the rasterizer-gradient bar of test_raster_gpu.py.  Both chains
              must also blend the same (tile, Gaussian) instances with the same radii: a pixel on a skip threshold is no yardstick.
  mutants     `loud`: each of the twelve wrong readings of a seam (step_ref.MUTANTS) moves at least one tensor by 10 x the GPU bar or
              more, and the loss -- where the reading changes it -- by 10 x the widest loss bar of the GPU test
              (step_ref.LOSS_BAR) or more.  The mutants are evaluated
              in float32 against the float32 chain (0.4 s instead of 1.6 s each); its own error is 1/40 of the threshold at most.
  default     the same twelve at the reference's default weights: the ones that stay below the bar are recorded, and are the reason the
              `loud` case exists (figures: the `cpu_mutant` rows of profiles/step_gradient_parity.jsonl).
  names       the reference's gradient dict has exactly the product's trainable parameter names (GaussianParams on the CPU), None
              where no gradient arrives; the restated weights equal pipeline.default_opt() / default_hyper()."""
import numpy as np
import pytest
import torch

from tests import step_ref as sr

_cache = {}


def chains(name):
    """(case, float64 result, float32 result, yardstick) of a case, evaluated once per session."""
    if name not in _cache:
        case = sr.build_case(name)
        r64, r32 = sr.reference_step(case, torch.float64), sr.reference_step(case, torch.float32)
        _cache[name] = (case, r64, r32, max(sr.distances(r32, r64).values()))
    return _cache[name]


@pytest.mark.parametrize("name", sr.CASES)
def test_float32_chain_is_within_the_yardstick_of_the_float64_chain(name):
    case, r64, r32, yard = chains(name)
    d = sr.distances(r32, r64)
    worst = max(d, key=d.get)
    print(f"{name}: yardstick {yard:.3e} ({worst}), loss {r64['loss']:.9f} vs {r32['loss']:.9f}, R = {r64['num_rendered']}, "
          f"visible = {int((r64['radii'] > 0).sum())}")
    sr.record(dict(test="cpu_yardstick", case=name, yardstick=yard, worst_tensor=worst, gpu_bar=sr.BAR_MARGIN * yard, per_tensor=d,
                   loss_f64=r64["loss"], loss_f32=r32["loss"], num_rendered=r64["num_rendered"], visible=int((r64["radii"] > 0).sum())))
    assert np.array_equal(r64["radii"], r32["radii"]) and r64["num_rendered"] == r32["num_rendered"]
    assert int((r64["radii"] > 0).sum()) > 400 and r64["num_rendered"] > 1000      # the view sees something
    assert {k for k, v in r64["grads"].items() if v is None} == {k for k, v in r32["grads"].items() if v is None}
    assert all(np.isfinite(v).all() and np.linalg.norm(v) > 0 for v in r64["grads"].values() if v is not None)
    assert yard <= sr.YARDSTICK_MAX, d
    assert sr.BAR_MARGIN * yard <= 1e-4
    assert abs(r32["loss"] - r64["loss"]) <= sr.LOSS_YARDSTICK_MAX * abs(r64["loss"])


def _shifts(name, mutant):
    case, r64, r32, yard = chains(name)
    mut = sr.reference_step(case, torch.float32, mutate=mutant)
    assert {k for k, v in mut["grads"].items() if v is None} == {k for k, v in r32["grads"].items() if v is None}
    d = sr.distances(mut, r32)
    return d, abs(mut["loss"] - r32["loss"]) / abs(r32["loss"]), sr.BAR_MARGIN * yard


@pytest.mark.parametrize("mutant", sorted(sr.MUTANTS))
def test_loud_case_exposes_every_wrong_reading(mutant):
    d, loss_shift, bar = _shifts("loud", mutant)
    worst = max(d, key=d.get)
    print(f"loud / {mutant}: {worst} moves by {d[worst]:.3e} (bar {bar:.3e}), loss by {loss_shift:.3e}")
    sr.record(dict(test="cpu_mutant", case="loud", mutant=mutant, largest_shift=d[worst], tensor=worst, gpu_bar=bar,
                   tensors_beyond_10_bars=sum(v >= 10 * bar for v in d.values()), rel_loss_shift=loss_shift))
    assert d[worst] >= 10 * bar, d
    if sr.MUTANTS[mutant]:
        assert loss_shift >= 10 * max(sr.LOSS_BAR.values()), loss_shift      # no case's loss bar is wider than a tenth of it
    else:
        assert loss_shift <= 1e-6


def test_default_weights_hide_some_wrong_readings():
    """Why `loud` exists: at the reference's default weights some seams can be wrong without any tensor leaving the neighbourhood of
    the bar.  Recorded, and asserted only as far as the argument needs it: at least one reading stays within 10 bars."""
    quiet = {}
    for mutant in sorted(sr.MUTANTS):
        d, loss_shift, bar = _shifts("default", mutant)
        worst = max(d, key=d.get)
        beyond = sum(v >= 10 * bar for v in d.values())
        print(f"default / {mutant}: {worst} moves by {d[worst]:.3e} (bar {bar:.3e}), {beyond} tensors beyond 10 bars, loss by {loss_shift:.3e}")
        sr.record(dict(test="cpu_mutant", case="default", mutant=mutant, largest_shift=d[worst], tensor=worst, gpu_bar=bar,
                       tensors_beyond_10_bars=beyond, rel_loss_shift=loss_shift))
        if d[worst] < 10 * bar:
            quiet[mutant] = d[worst]
    sr.record(dict(test="cpu_mutant_summary", case="default", within_10_bars=quiet))
    assert quiet, "every wrong reading is loud at the default weights: the `loud` case has lost its reason"


@pytest.mark.parametrize("name", sr.CASES)
def test_reference_names_are_the_products_trainable_parameters(name):
    from s3gaussian_amd.pipeline import GaussianParams, default_hyper, default_opt
    case, r64, _, _ = chains(name)
    pc = GaussianParams(3, case["hyper"])
    L = case["leaves"]
    pc.init_from_tensors(L["_xyz"], L["_scaling"], L["_rotation"], L["_opacity"], torch.cat([L["_features_dc"], L["_features_rest"]], 1), "cpu")
    pc._deformation.load_state_dict(case["state"])
    params = {n: p for n, p in pc.named_parameters() if p.requires_grad}
    assert set(params) == set(r64["grads"])
    assert set(sr.LEAVES) <= set(params) and sum("grid.grids" in n for n in params) == 24
    for n, g in r64["grads"].items():
        assert g is None or g.shape == tuple(params[n].shape), n
    for n, v in L.items():
        assert torch.equal(params[n].detach(), v), n
    connected = {n for n, g in r64["grads"].items() if g is not None}
    if name == "coarse":
        assert connected == set(sr.LEAVES)
    else:       # the reference's default heads: feature_out, pos_deform, shs_deform, dino_head and the planes; nothing else
        heads = ("feature_out", "pos_deform", "shs_deform", "dino_head", "grid.grids")
        assert connected == set(sr.LEAVES) | {n for n in params if any(h in n for h in heads)}
        assert len(connected) == 46
    # the weights restated in step_ref are the product's defaults
    assert vars(default_hyper(**case["hyper_over"])) == vars(case["hyper"])
    want = dict(vars(default_opt()), **(sr.LOUD_OPT if name == "loud" else {}))
    assert vars(case["opt"]) == want
