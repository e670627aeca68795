"""Generate tests/golden/depthvis.npz: inputs and the reference's own bytes for the coloured depth frames (s3gaussian_amd/depthvis.py).

    python tests/golden/make_golden_depthvis.py        # rewrites depthvis.npz next to this file

Runs in the build container only: `*_bytes` are recorded from the REFERENCE'S OWN utils/visualization_tools.py (loaded from the
reference tree, never copied; the modules it imports for other functions and the container lacks are replaced by empty stubs, as in
make_golden_flow.py), called the way its depth_visualizer does (utils/video_utils.py:27-33):
    to8b(visualize_depth(depth, acc, lo, hi, depth_curve_fn=lambda x: -np.log(x + 1e-6)))
for (lo, hi) = (4.0, 120) and (None, None).  Without the reference tree this script refuses to run.

Cases: seeded street-like frames (tests/depthvis_ref.py::street) at 37 x 53 and 96 x 144, `{name}_depth`, `{name}_alpha`; per bounds
kind in ("fixed", "auto"): `{name}_{kind}_bytes` (the reference's uint8 [H,W,3]) and `{name}_{kind}_mismatch_pixels`, the number of
pixels where the restatement's bytes differ from the reference's -- each by exactly one table step, asserted here.  `{name}_percentiles`:
the reference's own weighted_percentile(depth, acc, [0.5, 99.5]) (fp32 cumsum); `{name}_percentile_rel`: the largest relative distance
of the restatement's from them.  `table`: the 256 x 3 bytes of matplotlib's turbo table through to8b."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import depthvis_ref as dr  # noqa: E402
from tests.golden.make_golden_flow import reference_module  # noqa: E402

CASES = (("s37x53", 37, 53, 4101), ("s96x144", 96, 144, 4102))
BOUNDS = {"fixed": (4.0, 120), "auto": (None, None)}


def turbo_table():
    import matplotlib
    lut = matplotlib.colormaps["turbo"](np.arange(256))[:, :3]
    return (255 * np.clip(lut, 0, 1)).astype(np.uint8)


def main():
    vt = reference_module()
    table = turbo_table()
    assert len({tuple(r) for r in table.tolist()}) == 256, "steps_apart needs distinct table rows"
    out = {"table": table}
    for name, H, W, seed in CASES:
        depth, alpha = dr.street(H, W, seed)
        assert depth.min() > 0 and alpha.min() >= 0 and alpha.max() <= 1 and alpha[0].mean() < 0.35 and alpha[-1].mean() > 0.95
        out[f"{name}_depth"], out[f"{name}_alpha"] = depth, alpha
        ref_p = np.asarray(vt.weighted_percentile(depth, alpha, [0.5, 99.5]), dtype=np.float64)
        mine_p = dr.weighted_percentiles(depth, alpha)
        rel = float(np.max(np.abs(mine_p - ref_p) / np.abs(ref_p)))
        out[f"{name}_percentiles"], out[f"{name}_percentile_rel"] = ref_p, np.float64(rel)
        print(f"{name}: reference percentiles {ref_p}, restatement {mine_p}, relative distance {rel:.3e}")
        for kind, (lo, hi) in BOUNDS.items():
            ref = vt.to8b(vt.visualize_depth(depth.copy(), alpha.copy(), lo, hi, depth_curve_fn=lambda x: -np.log(x + 1e-6)))
            assert ref.dtype == np.uint8 and ref.shape == (H, W, 3)
            mine = dr.colors(depth, alpha, None if lo is None else float(lo), None if hi is None else float(hi), table)
            differ = np.any(mine != ref, axis=-1)
            steps = dr.steps_apart(mine, ref, table)
            assert steps.min() >= 0 and np.all(steps[differ] == 1), (name, kind, np.unique(steps))
            out[f"{name}_{kind}_bytes"] = ref
            out[f"{name}_{kind}_mismatch_pixels"] = np.int64(differ.sum())
            print(f"  {kind:5s}: {int(differ.sum())} of {H * W} pixels differ, each by one table step; "
                  f"{int(dr.near_step(dr.u256(depth, alpha, lo, hi)).sum())} near a step")
    path = os.path.join(HERE, "depthvis.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 300 * 1024


if __name__ == "__main__":
    main()
