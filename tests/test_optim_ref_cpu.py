"""The checker of tests/test_optim_trajectory_gpu.py, checked without a GPU: tests/optim_ref.py's float64 Adam against
torch.optim.Adam in float64 over every script, and the bar's power -- a float32 restatement of csrc/adam.hip passes it, the same
restatement with one wrong reading (optim_ref.MUTANTS) lands at least ten times above it."""
import math

import pytest
import torch

from tests import optim_ref as R

SENSITIVITY = 10.0          # a mutant's error / bar on its worst tensor, at least
# the events after which a bias correction that is one step behind must show in that event's own script (at 29 990 steps both
# corrections are 1 to the last bit, and "set_lr" has no event)
STALE_STEP_EVENTS = tuple(e for e in R.EVENTS if e not in ("set_lr", "jump"))


def _script(name):
    return R.full_script() if name == "all" else R.event_script(name)


@pytest.mark.parametrize("name", ("all",) + R.EVENTS + ("repoint_shrink", "repoint_grow", "repoint_restride"))
def test_float64_reference_equals_torch_adam_in_float64(name):
    """Two double evaluations of one recurrence over at most 60 steps: 1e-12 of the tensor's scale, equal step counts."""
    script = R.repoint_script(name[len("repoint_"):]) if name.startswith("repoint_") else _script(name)
    mine = R.run(script, R.PlainAdam(script, R.F64))
    ref = R.run(script, R.TorchSubject(script, "torch64"))
    assert set(mine) == set(script["tensors"]) == set(ref)
    for n in mine:
        assert mine[n][3] == ref[n][3] and mine[n][3] > 0, (n, mine[n][3], ref[n][3])
        for k, q in enumerate(("p", "m", "v")):
            a, b = mine[n][k], ref[n][k]
            assert a.shape == b.shape and a.dtype == b.dtype == torch.float64
            scale = float(b.abs().max())
            assert scale > 0 and float((a - b).abs().max()) <= 1e-12 * scale, (n, q, float((a - b).abs().max()), scale)


def test_full_script_holds_every_event_and_input_the_bar_needs():
    script = R.full_script()
    kinds = [(op[1], op[2]) for op in script["ops"] if op[0] == "event"]
    assert {k for k, _ in kinds} == {"replace", "cat", "prune", "permute", "checkpoint", "step_repr", "jump"}
    assert [p for k, p in kinds if k == "checkpoint"] == ["same", "fresh"]
    assert tuple(p for k, p in kinds if k == "step_repr") == R.STEP_REPRS
    steps = [op[1] for op in script["ops"] if op[0] == "step"]
    assert 40 <= len(steps) <= 60 and len(script["tensors"]) <= 12
    assert all(g.numel() <= 4200 for s in steps for g in s.values() if g is not None)
    assert steps[0]["mlp_b"] is None and steps[23]["mlp_b"] is None and steps[10]["mlp_b"] is not None
    assert bool((steps[5]["f_rest"].reshape(-1)[::5] == 0).all()) and bool((steps[5]["f_rest"].reshape(-1)[1::5] != 0).all())
    scales = sorted(spec["grad"] for spec in script["tensors"].values())
    assert scales[0] == 1e-6 and scales[-1] == 1e2
    assert {R.GROUPS[g]["eps"] for g in script["groups"]} == {1e-15, 1e-8}
    assert len({R.GROUPS[g]["betas"] for g in script["groups"]}) == 2          # more than one launch per step
    # no lr phase so small that an event's effect vanishes: the schedules fall by less than 4x over a script
    lrs = [op[1] for op in script["ops"] if op[0] == "lr"]
    assert all(lrs[-1][g] > 0.25 * lrs[0][g] and lrs[k + 1][g] < lrs[k][g] for g in lrs[0] for k in range(len(lrs) - 1))


@pytest.mark.parametrize("fma", (False, True), ids=("plain", "contracted"))
@pytest.mark.parametrize("name", ("all", "shapes") + R.EVENTS)
def test_float32_restatement_of_the_kernel_is_under_the_bar(name, fma):
    """csrc/adam.hip's operation order in float32 on the CPU, with and without the contractions a compiler may make: what the
    GPU is expected to compute.  If this did not pass, the bar would ask more than float32 can give."""
    script = R.shapes_script() if name == "shapes" else _script(name)
    f64, cpu32 = R.yardsticks(name, script)
    rows = R.compare(R.run(script, R.PlainAdam(script, R.F32, fma=fma)), f64, cpu32)
    assert all(r["ok"] for r in rows), "\n" + R.table(rows, only_failed=True)


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_is_ten_times_over_the_bar_on_the_full_script(mutant):
    script = R.full_script()
    f64, cpu32 = R.yardsticks("all", script)
    rows = R.compare(R.run(script, R.PlainAdam(script, R.F32, mutate=mutant)), f64, cpu32)
    worst = R.worst_over_bar(rows)
    print(f"{mutant}: worst err / bar = {worst:.3g}")
    assert all(r["ok"] for r in rows if r["quantity"] == "step")        # the reported counts are right: only the arithmetic is off
    assert worst >= SENSITIVITY, f"{mutant}: {worst:.3g} x the bar\n" + R.table(rows)


@pytest.mark.parametrize("event,mutant", [(e, "stale_step") for e in STALE_STEP_EVENTS]
                         + [("replace", "no_zero_at_replace"), ("permute", "no_permute_moments"), ("set_lr", "prev_lr"),
                            ("set_lr", "gs_m_only"), ("set_lr", "w2_f32")])
def test_each_event_script_sees_its_own_mutant(event, mutant):
    script = R.event_script(event)
    f64, cpu32 = R.yardsticks(event, script)
    rows = R.compare(R.run(script, R.PlainAdam(script, R.F32, mutate=mutant)), f64, cpu32)
    worst = R.worst_over_bar(rows)
    print(f"{event} / {mutant}: worst err / bar = {worst:.3g}")
    assert worst >= SENSITIVITY, f"{event} / {mutant}: {worst:.3g} x the bar\n" + R.table(rows)


def test_jump_keeps_the_bias_corrections_finite():
    script = R.event_script("jump")
    f64, _ = R.yardsticks("jump", script)
    for n, (p, m, v, step) in f64.items():
        assert step == R.JUMP_TO + 10 and all(bool(torch.isfinite(t).all()) for t in (p, m, v)), n
    assert math.isfinite(1.0 / math.sqrt(1.0 - 0.999 ** R.JUMP_TO))


def test_bar_has_an_ulp_floor_where_the_cpu_is_exact():
    z = torch.zeros(4, dtype=torch.float64)
    one = {"t": (z + 1.0, z, z, 1.0)}
    rows = R.compare({"t": (z + 1.0 + 1e-7, z, z, 1.0)}, one, one)
    assert [r["ok"] for r in rows] == [True, True, True, True]           # 1e-7 < ulp32(1) = 1.19e-7
    rows = R.compare({"t": (z + 1.0 + 2e-7, z, z + 1e-40, 2.0)}, one, one)
    assert [r["ok"] for r in rows] == [False, True, False, False]
