"""Generate tests/golden/sky_frames.npz: what the reference's own save_seperate_videos writes for the keys its render_func never
fills -- "opacities", "sky_masks", "gt_sky_masks" (utils/video_utils.py:461-471, 480, 489) -- from generated opacity images.

    python tests/golden/make_golden_sky_frames.py        # rewrites sky_frames.npz next to this file

Runs in the build container only, like make_golden_frames.py, whose loader of the reference's module (imageio replaced by a
recording stub) it uses.  render_results holds one [H,W] fp32 array per camera under "opacities" and under "gt_sky_masks" -- the
`permute(1, 2, 0).squeeze()` form render_func gives its images, here of a [1,H,W] image -- and the function is called as
train.py::do_evaluation calls it, with keys = the three.  "sky_masks" reads render_results["opacities"]; its list only has to be
non-empty.

Per size s{H}x{W} of frames_ref.SIZES, 2 timestamps x 3 cameras: s.._in_opacities, s.._in_gt_sky_masks [6,1,H,W] fp32,
s.._frames_{key}: every frame the key's writer received -- [2, H, 3 W] uint8 for "opacities" (a strip of [H,W] frames has no
channel axis), [2, H, 3 W, 3] for the two mask keys -- and s.._middle_{key}, the returned frame."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from tests import frames_ref as fr  # noqa: E402
import make_golden_frames as mg  # noqa: E402

f32 = np.float32
KEYS = ("opacities", "sky_masks", "gt_sky_masks")


def unit_images(rng, n, H, W):
    """[n,1,H,W] fp32 in [0,1] with exact 0 and 1 and k / 255 with its fp32 neighbours (for x and for 1 - x) among the values."""
    x = rng.uniform(0.0, 1.0, size=(n, 1, H, W)).astype(f32)
    v = [f32(0.0), f32(1.0)]
    for k in fr.PLANTED_K[:3]:
        q = f32(k) / f32(255)
        v += [np.nextafter(q, f32(-1)), q, np.nextafter(q, f32(2)), f32(1) - q]
    flat = x[0].reshape(-1)
    flat[rng.choice(flat.size, size=len(v), replace=False)] = np.array(v, f32)
    return x


def main():
    log = {}
    vu = mg.reference_module(log)
    out = {}
    n, T = fr.NUM_CAMS, fr.NUM_TIMESTAMPS
    for H, W in fr.SIZES:
        rng = np.random.default_rng(1900 + 10 * H + W)
        inputs = {"opacities": unit_images(rng, n * T, H, W), "gt_sky_masks": unit_images(rng, n * T, H, W)}
        results = {k: [inputs[k][i, 0].copy() for i in range(n * T)] for k in inputs}
        results["sky_masks"] = results["opacities"]
        log.clear()
        path = f"/nonexistent/s{H}x{W}.mp4"
        returned = vu.save_seperate_videos(results, path, num_timestamps=T, keys=list(KEYS), num_cams=n, fps=24)
        tag = f"s{H}x{W}"
        for k in KEYS:
            frames = log[path.replace(".mp4", f"_{k}.mp4")]
            shape = (H, n * W) if k == "opacities" else (H, n * W, 3)
            assert len(frames) == T and all(f.dtype == np.uint8 and f.shape == shape for f in frames), (k, [f.shape for f in frames])
            assert np.array_equal(returned[k], frames[T // 2])
            out[f"{tag}_frames_{k}"] = np.stack(frames)
            out[f"{tag}_middle_{k}"] = np.array(returned[k], copy=True)
        for k in inputs:
            out[f"{tag}_in_{k}"] = inputs[k]
        assert not np.array_equal(out[f"{tag}_frames_sky_masks"][0], out[f"{tag}_frames_sky_masks"][1])
    dst = os.path.join(HERE, "sky_frames.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")
    assert os.path.getsize(dst) < 100 * 1024


if __name__ == "__main__":
    main()
