"""The checker of tests/test_step_views_gpu.py, checked (no GPU): tests/step_ref_views.py, the float64 reference chain of one
training step over a batch of views.

  one view    a batch of step_ref's own view reproduces step_ref.reference_step to 1e-12: the helper adds batch semantics, nothing else
  yardstick   per case, float32 chain against float64 chain over every gradient tensor, the summed viewspace gradient and
              xyz_gradient_accum: at most step_ref.YARDSTICK_MAX, so the GPU bar (BAR_MARGIN x the case's largest) stays <= 1e-4;
              both chains blend the same instances with the same radii in every view
  mutants     each wrong reading of a batch seam (step_ref_views.MUTANTS: depth normalised per view; dx / dshs / feat terms from the
              first view; the feature image supervised on all views under feat_views="last"; the sum of per-view gradient norms
              instead of the norm of the sum; the plane regulariser applied V times) moves some tensor by 10 x the GPU bar or more,
              on the case named beside it.  Evaluated in float32 against the float32 chain, like step_ref's."""
import numpy as np
import pytest
import torch

from tests import step_ref as sr
from tests import step_ref_views as srv

_cache = {}


def chains(name):
    """(case, float64 result, float32 result, yardstick) of a case, evaluated once per session."""
    if name not in _cache:
        case = srv.build_case(name)
        r64, r32 = srv.reference_step_views(case, torch.float64), srv.reference_step_views(case, torch.float32)
        _cache[name] = (case, r64, r32, max(srv.distances(r32, r64).values()))
    return _cache[name]


def test_a_one_view_batch_is_the_single_view_reference_step():
    case = srv.build_case("one", views=(sr.VIEW,), base="default")
    one = srv.reference_step_views(case, torch.float64)
    ref = sr.reference_step(sr.build_case("default"), torch.float64)
    assert abs(one["loss"] - ref["loss"]) <= 1e-12 * abs(ref["loss"])
    assert set(one["grads"]) == set(ref["grads"])
    for k, g in ref["grads"].items():
        if g is None:
            assert one["grads"][k] is None, k
        else:
            assert sr.rel_l2(one["grads"][k], g) <= 1e-12, k
    assert sr.rel_l2(one["dL_dmeans2D"], ref["dL_dmeans2D"]) <= 1e-12
    assert np.array_equal(one["radii"][0], ref["radii"]) and one["num_rendered"] == [ref["num_rendered"]]
    for a, b in zip(one["stats"], sr.densify_stats(ref["dL_dmeans2D"], ref["radii"])):
        assert sr.rel_l2(a, b) <= 1e-12


@pytest.mark.parametrize("name", sorted(srv.CASES))
def test_float32_chain_is_within_the_yardstick_of_the_float64_chain(name):
    case, r64, r32, yard = chains(name)
    d = srv.distances(r32, r64)
    worst = max(d, key=d.get)
    visible = [int((r > 0).sum()) for r in r64["radii"]]
    print(f"{name}: yardstick {yard:.3e} ({worst}), loss {r64['loss']:.9f} vs {r32['loss']:.9f}, R = {r64['num_rendered']}, visible = {visible}")
    sr.record(dict(test="cpu_yardstick_views", case=name, views=list(case["views"]), yardstick=yard, worst_tensor=worst,
                   gpu_bar=sr.BAR_MARGIN * yard, per_tensor=d, loss_f64=r64["loss"], loss_f32=r32["loss"],
                   num_rendered=r64["num_rendered"], visible=visible))
    assert all(np.array_equal(a, b) for a, b in zip(r64["radii"], r32["radii"])) and r64["num_rendered"] == r32["num_rendered"]
    assert min(visible) > 400 and min(r64["num_rendered"]) > 1000                   # every view sees something
    seen_by = np.sum([r > 0 for r in r64["radii"]], axis=0)
    print(f"  Gaussians seen by exactly one view: {int((seen_by == 1).sum())}, by several: {int((seen_by >= 2).sum())}")
    assert (seen_by == 1).sum() > 50 and (seen_by >= 2).sum() > 50                    # one view only / several: both happen
    assert {k for k, v in r64["grads"].items() if v is None} == {k for k, v in r32["grads"].items() if v is None}
    assert all(np.isfinite(v).all() and np.linalg.norm(v) > 0 for v in r64["grads"].values() if v is not None)
    assert np.array_equal(r64["stats"][1], r32["stats"][1]) and np.array_equal(r64["stats"][2], r32["stats"][2])
    assert yard <= sr.YARDSTICK_MAX, d
    assert sr.BAR_MARGIN * yard <= 1e-4
    assert abs(r32["loss"] - r64["loss"]) <= sr.LOSS_YARDSTICK_MAX * abs(r64["loss"])


# the case on which each wrong reading is shown: `mixed` where "the last view" has to differ from "the first", `rig` elsewhere
MUTANT_CASE = {"depth_per_view": "rig", "last_view_terms_from_first": "mixed", "feat_on_all_views": "rig",
               "sum_of_view_norms": "rig", "plane_reg_per_view": "rig"}


@pytest.mark.parametrize("mutant", sorted(srv.MUTANTS))
def test_every_wrong_reading_of_a_batch_seam_is_loud(mutant):
    assert set(MUTANT_CASE) == set(srv.MUTANTS)
    name = MUTANT_CASE[mutant]
    case, r64, r32, yard = chains(name)
    mut = srv.reference_step_views(case, torch.float32, mutate=mutant)
    d, bar = srv.distances(mut, r32), sr.BAR_MARGIN * yard
    loss_shift = abs(mut["loss"] - r32["loss"]) / abs(r32["loss"])
    worst = max(d, key=d.get)
    print(f"{name} / {mutant}: {worst} moves by {d[worst]:.3e} (bar {bar:.3e}), loss by {loss_shift:.3e}")
    sr.record(dict(test="cpu_mutant_views", case=name, mutant=mutant, largest_shift=d[worst], tensor=worst, gpu_bar=bar,
                   tensors_beyond_10_bars=sum(v >= 10 * bar for v in d.values()), rel_loss_shift=loss_shift))
    assert d[worst] >= 10 * bar, d
    if srv.MUTANTS[mutant]:
        assert loss_shift >= 10 * sr.BAR_MARGIN * sr.LOSS_YARDSTICK_MAX, loss_shift
    else:
        assert loss_shift <= 1e-6


def test_feat_views_all_is_another_step_than_the_reference_batch():
    """The extension supervises every view's feature image: against feat_views="last" it moves tensors by many bars (so the GPU
    test of either variant cannot be passed by the other)."""
    case, r64, r32, yard = chains("rig")
    every = srv.reference_step_views(case, torch.float32, feat_views="all")
    d = srv.distances(every, r32)
    assert max(d.values()) >= 10 * sr.BAR_MARGIN * yard, d
