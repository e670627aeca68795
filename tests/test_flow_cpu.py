"""CPU-only: the checker of the scene-flow colours is itself checked, the frame plan is tied to the reference's loops, and the binding
refuses what it must without a device.

tests/flow_ref.py (pure numpy, table form) is what tests/test_flow_gpu.py compares the kernel with.  Here it is tied to the reference's
own scene_flow_to_rgb output recorded in tests/golden/scene_flow.npz.

The colour bar: flow_ref.COLOR_BAR = 4 x 1.78813934e-07 = 7.15e-07, four times the largest |restatement - reference| that
tests/golden/make_golden_flow.py measured over the fixture (numpy's and torch's fp32 atan2 / hypot differ in the last bit).  It is far
below 1e-5, and a wheel index off by one moves the green channel by 0.067 r."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import flow_ref as fr


@pytest.fixture(scope="module")
def fixture():
    return fr.load_fixture()


def test_restatement_matches_the_references_colours(fixture):
    cases, _, max_dev = fixture
    assert fr.COLOR_BAR == 4 * fr.MEASURED_DEV <= 1e-5 and abs(max_dev - fr.MEASURED_DEV) <= 1e-12
    seen = 0.0
    for c in cases:
        got = fr.colors(c["dx_a"], c["dx_b"])
        assert got.dtype == np.float32 and got.shape == c["colors"].shape
        dev = float(np.abs(got - c["colors"]).max())
        print(f"{c['name']}: |restatement - reference| max {dev:.4e}")
        seen = max(seen, dev)
        assert dev <= fr.COLOR_BAR, (c["name"], dev)
        lo, hi = fr.flow_range(c["dx_a"], c["dx_b"])
        assert lo == c["min"] and hi == c["max"]
    assert abs(seen - max_dev) <= 1e-12       # the bar's source is what this machine evaluates, too


def test_fixture_inputs_reach_both_branches_and_both_axes(fixture):
    """For every P >= 63: at least 5 % of the rows with r > 1, at least 5 % with r < 0.05, a row with y == 0 and one with x == 0."""
    cases, _, _ = fixture
    assert [c["dx_a"].shape[0] for c in cases[:len(fr.SIZES)]] == list(fr.SIZES)
    for c in cases:
        if c["dx_a"].shape[0] < 63:
            continue
        f = fr.normalise(c["dx_a"], c["dx_b"])
        r = np.hypot(f[:, 0], f[:, 1])
        assert (r > 1).mean() >= 0.05 and (r < 0.05).mean() >= 0.05, c["name"]
        assert (f[:, 1] == 0).any() and (f[:, 0] == 0).any(), c["name"]
        assert f.min() == 0 and f.max() < 1


def test_zero_flow_is_white_and_one_moving_row_is_the_only_colour(fixture):
    cases, _, _ = fixture
    zero, one = cases[-2], cases[-1]
    assert np.array_equal(zero["dx_a"], zero["dx_b"]) and np.array_equal(zero["colors"], np.ones_like(zero["colors"]))
    assert np.array_equal(fr.colors(zero["dx_a"], zero["dx_b"]), np.ones_like(zero["colors"]))
    assert int((one["dx_a"] != one["dx_b"]).any(axis=1).sum()) == 1


def test_wheel_built_by_the_references_rule_equals_the_recorded_wheel(fixture):
    _, wheel, _ = fixture
    assert wheel.shape == (56, 3) and fr.WHEEL.dtype == wheel.dtype and np.array_equal(fr.WHEEL, wheel)
    assert np.array_equal(fr.WHEEL[:16], np.stack([np.full(16, 255.0), 17.0 * np.arange(16), np.zeros(16)], axis=1))


def test_closed_form_equals_the_table_form_on_the_reachable_domain():
    """Step 1 puts x and y into [0, 1): a dense grid of [0, 1]^2 (corners, both axes and the r = 1 arc's neighbourhood included)."""
    u = np.linspace(0.0, 1.0, 1201, dtype=np.float32)
    x, y = np.meshgrid(u, u)
    dev = float(np.abs(fr.closed_form(x, y) - fr.table_form(x, y)).max())
    print(f"|closed form - table form| max {dev:.4e} over {x.size} points")
    assert dev <= fr.COLOR_BAR
    r = np.hypot(x, y)
    assert (r > 1).any() and (r == 0).any() and (np.arctan2(y, x) * 54 / (2 * np.pi)).max() >= 13.49


def test_wrong_readings_of_the_definition_are_far_outside_the_bar(fixture):
    """The dark background, the radius over all three components, min / max per column and a missing 1e-6 each move a colour by at
    least 10 bars on every fixture case with P >= 63."""
    cases, _, _ = fixture
    for c in cases:
        if c["dx_a"].shape[0] < 63:
            continue
        for v in fr.VARIANTS:
            moved = float(np.abs(fr.colors(c["dx_a"], c["dx_b"], variant=v) - c["colors"]).max())
            assert moved >= 10 * fr.COLOR_BAR, (c["name"], v, moved)


def test_frame_plan_of_nine_frames_is_the_hand_enumerated_one():
    """utils/video_utils.py:252-299 at num_cams = 3 and 9 frames."""
    from s3gaussian_amd.flow import frame_plan
    forward, backward = frame_plan(9, 3)
    assert [tuple(p) for p in forward] == [(0, 3, False), (1, 4, False), (2, 5, False), (3, 6, False), (4, 7, False), (5, 8, False),
                                           (3, 6, True), (4, 7, True), (5, 8, True)]
    assert [tuple(p) for p in backward] == [(0, 3, True), (1, 4, True), (2, 5, True), (0, 3, False), (1, 4, False), (2, 5, False),
                                            (3, 6, False), (4, 7, False), (5, 8, False)]
    assert [p[:2] for p in forward[6:]] == [p[:2] for p in backward[6:]] and [p[:2] for p in backward[:3]] == [p[:2] for p in forward[:3]]


def _reference_lists(N, num_cams=3):
    """Index-level transliteration of utils/video_utils.py:252-299: which (camera, (from, to)) each list ends up holding."""
    forward, backward, bf_first, ff_last = [], [], [], []
    for t in range(N):
        if t < N - num_cams:
            ff = (t, t + num_cams)
            if t == N - num_cams - 1 or t == N - num_cams - 2 or t == N - num_cams - 3:
                ff_last.append(ff)
            forward.append((t, ff))
        if t > num_cams - 1:
            bf = (t - num_cams, t)
            if t == num_cams or t == num_cams + 1 or t == num_cams + 2:
                bf_first.append(bf)
            backward.append((t, bf))
    for i, bf in enumerate(bf_first):
        backward.insert(i, (i, bf))
    for i, ff in enumerate(ff_last):
        forward.append((N - num_cams + i, ff))
    return forward, backward


@pytest.mark.parametrize("N", [6, 9, 12])
def test_frame_plan_agrees_with_the_references_loops(N):
    from s3gaussian_amd.flow import frame_plan
    forward, backward = frame_plan(N, 3)
    ref_f, ref_b = _reference_lists(N, 3)
    assert [(i, (p.from_frame, p.to_frame)) for i, p in enumerate(forward)] == ref_f
    assert [(i, (p.from_frame, p.to_frame)) for i, p in enumerate(backward)] == ref_b


def test_frame_plan_refuses_too_few_frames():
    from s3gaussian_amd.flow import frame_plan
    for N, n in ((5, 3), (0, 1), (1, 1), (7, 4)):
        with pytest.raises(ValueError):
            frame_plan(N, n)
    with pytest.raises(ValueError):
        frame_plan(9, 0)
    forward, backward = frame_plan(2, 1)
    assert [tuple(p) for p in forward] == [(0, 1, False), (0, 1, True)] and [tuple(p) for p in backward] == [(0, 1, True), (0, 1, False)]
    assert len(frame_plan(8, 4)[0]) == 8


def test_scene_flow_colors_has_no_cpu_fallback():
    from s3gaussian_amd.flow import scene_flow_colors
    x = torch.rand(16, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        scene_flow_colors(x, x)


def test_extra_colors_is_refused_outside_no_grad():
    from s3gaussian_amd.pipeline import render
    with pytest.raises(RuntimeError, match="no_grad"):
        render({}, None, None, None, extra_colors=[torch.zeros(1, 3)])


def test_null_and_negative_p_are_refused_before_any_device_call():
    """Return code 1 and a message with NULL pointers and no GPU in the machine; P == 0 succeeds without looking at a pointer."""
    from s3gaussian_amd import flow
    L = flow._bind()
    assert L.s3g_scene_flow_colors(-1, None, None, None, None, None, None) == 1 and b"P = -1" in L.s3g_last_error()
    assert L.s3g_scene_flow_colors(5, None, None, None, None, None, None) == 1 and b"NULL" in L.s3g_last_error()
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    for args in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):     # dx_a, dx_b, colors, workspace
        assert L.s3g_scene_flow_colors(5, args[0], args[1], args[2], None, args[3], None) == 1 and b"NULL" in L.s3g_last_error()
    assert L.s3g_scene_flow_colors(0, None, None, None, None, None, None) == 0


def test_workspace_bytes_are_monotone():
    from s3gaussian_amd import flow
    L = flow._bind()
    sizes = (1, 2, 63, 64, 65, 1365, 1366, 4096, 70_001, 699_050, 699_051, 1_200_000, 10_000_000, 2 ** 31 - 1)
    got = [L.s3g_scene_flow_workspace_bytes(P) for P in sizes]
    assert got == sorted(got) and got[0] > 0 and got[-1] > got[0]
    assert L.s3g_scene_flow_workspace_bytes(0) == 0 and L.s3g_scene_flow_workspace_bytes(-3) == 0
