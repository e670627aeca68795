"""Generate tests/golden/scene_flow.npz: inputs and the reference's own colours for the scene-flow colours (s3gaussian_amd/flow.py).

    python tests/golden/make_golden_flow.py        # rewrites scene_flow.npz next to this file

Runs in the build container only: `*_colors` are recorded from the REFERENCE'S OWN utils/visualization_tools.py::scene_flow_to_rgb
(loaded from the reference tree, never copied; plotly and cv2, which that module imports for other functions and the container lacks,
are replaced by empty stub modules), called the way its flow_visualizer does: background="bright", flow_max_radius=1.0.  Without the
reference tree this script refuses to run.

Cases: p{P} for P in flow_ref.SIZES, `zero` (dx_a == dx_b: every colour is white) and `one_row` (dx_a == dx_b except for one row).
Per case: {name}_dx_a, {name}_dx_b, {name}_colors (the reference's fp32 output), {name}_min / {name}_max (flow.min() / flow.max()).
Also `wheel`, the reference's 56 x 3 WHEEL, and `max_dev`, the largest |tests/flow_ref.py - reference| over all cases -- the
yardstick of the colour bar (flow_ref.COLOR_BAR = 4 x, which this script checks against the constant in flow_ref.py).

Inputs for P >= 63 (shares asserted here and in tests/test_flow_cpu.py): the flow's components lie in [-0.004, 0.006] -- a span at
which the 1e-6 of step 1 moves a colour by 1e-4 -- with the minimum in the x and y columns and the maximum in the z column only: x
reaches 0.95 and y 0.85 of the range, so a per-column normalisation shows.  8 % of the rows have x in [0.80, 0.94] and y in
[0.72, 0.84] of the range (r > 1, the `hue / r` branch), 8 % have both within 3 % of the minimum (r < 0.05), the rest is uniform in
[0.05, 0.80].  Row 0 is (mid, min, mid) and row 1 (min, mid, mid) with dx_a = 0, so that y = 0 and x = 0 exactly; row 2 holds the
maxima.  Everything else has a random dx_a, so the difference is a real fp32 subtraction."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("S3G_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import flow_ref as fr  # noqa: E402

LO, HI = -0.004, 0.006


def reference_module():
    path = os.path.join(REF, "utils", "visualization_tools.py")
    if not os.path.isfile(path):
        raise SystemExit(f"{path} is missing: the fixture records the reference's own colours and cannot be written without it")
    for name in ("plotly", "plotly.graph_objects", "cv2", "tqdm"):
        try:
            __import__(name)
        except Exception:
            sys.modules[name] = types.ModuleType(name)
            if name == "tqdm":
                sys.modules[name].tqdm = lambda x, **k: x
    if not hasattr(sys.modules["plotly"], "graph_objects"):
        sys.modules["plotly"].graph_objects = sys.modules["plotly.graph_objects"]
    spec = importlib.util.spec_from_file_location("_reference_visualization_tools", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_case(P, seed):
    rng = np.random.default_rng(seed)
    span = HI - LO
    at = lambda u: LO + span * np.asarray(u)      # a position in the range, 0 = minimum, 1 = maximum
    flow = at(rng.uniform(0.05, 0.80, size=(P, 3)))
    dx_a = (0.05 * rng.standard_normal((P, 3))).astype(np.float32)
    if P >= 63:
        n = max(4, int(round(0.08 * P)))
        big, small = np.arange(3, 3 + n), np.arange(3 + n, 3 + 2 * n)
        flow[big, 0], flow[big, 1] = at(rng.uniform(0.80, 0.94, size=n)), at(rng.uniform(0.72, 0.84, size=n))
        flow[small, :2] = at(rng.uniform(0.001, 0.03, size=(n, 2)))
        flow[0], flow[1], flow[2] = at((0.5, 0.0, 0.5)), at((0.0, 0.5, 0.5)), at((0.95, 0.85, 1.0))
        dx_a[:3] = 0.0
    dx_b = (dx_a.astype(np.float64) + flow).astype(np.float32)
    return dx_a, dx_b


def shares(dx_a, dx_b):
    f = fr.normalise(dx_a, dx_b)
    r = np.hypot(f[:, 0], f[:, 1])
    return float((r > 1).mean()), float((r < 0.05).mean()), int((f[:, 1] == 0).sum()), int((f[:, 0] == 0).sum())


def main():
    vt = reference_module()
    out, dev = {}, 0.0
    cases = [(f"p{P}", *make_case(P, seed=500 + P)) for P in fr.SIZES]
    a = (0.05 * np.random.default_rng(7).standard_normal((17, 3))).astype(np.float32)
    cases.append(("zero", a, a.copy()))
    b = a.copy()
    b[5] += np.float32(0.01) * np.array([1.0, -2.0, 0.5], np.float32)
    cases.append(("one_row", a, b))
    for name, dx_a, dx_b in cases:
        flow = torch.from_numpy(dx_b) - torch.from_numpy(dx_a)
        ref = vt.scene_flow_to_rgb(flow, background="bright", flow_max_radius=1.0).numpy()
        assert ref.dtype == np.float32 and ref.shape == dx_a.shape
        mine = fr.colors(dx_a, dx_b)
        d = float(np.abs(mine - ref).max())
        dev = max(dev, d)
        out.update({f"{name}_dx_a": dx_a, f"{name}_dx_b": dx_b, f"{name}_colors": ref, f"{name}_min": np.float32(flow.min().item()),
                    f"{name}_max": np.float32(flow.max().item())})
        over, small, y0, x0 = shares(dx_a, dx_b)
        print(f"{name:8s} P {dx_a.shape[0]:5d}: |restatement - reference| max {d:.4e}; r > 1 {over:.3f}, r < 0.05 {small:.3f}, "
              f"y == 0 rows {y0}, x == 0 rows {x0}")
        if dx_a.shape[0] >= 63:
            assert over >= 0.05 and small >= 0.05 and y0 >= 1 and x0 >= 1, name
        for v in fr.VARIANTS:
            moved = float(np.abs(fr.colors(dx_a, dx_b, variant=v) - ref).max())
            print(f"           {v:12s} moves a colour by {moved:.3e}")
    assert np.array_equal(ref_wheel := vt.WHEEL.numpy().astype(np.float32), fr.WHEEL) and vt.N_COLS == fr.N_COLS
    assert np.array_equal(vt.scene_flow_to_rgb(torch.zeros(5, 3), background="bright", flow_max_radius=1.0).numpy(), np.ones((5, 3)))
    out["wheel"], out["max_dev"] = ref_wheel, np.float64(dev)
    print(f"max_dev = {dev:.8e}  ->  colour bar {4 * dev:.4e}")
    path = os.path.join(HERE, "scene_flow.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 400 * 1024
    assert abs(fr.MEASURED_DEV - dev) <= 1e-12, f"update MEASURED_DEV in tests/flow_ref.py to {dev:.8e}"


if __name__ == "__main__":
    main()
