"""Generate tests/golden/video_frames.npz: inputs and the reference's own video frames for s3gaussian_amd/frames.py.

    python tests/golden/make_golden_frames.py        # rewrites video_frames.npz next to this file

Runs in the build container only: the `frames` and `middle` arrays are what the REFERENCE'S OWN utils/video_utils.py::
save_seperate_videos (loaded from the reference tree, never copied) appended to its video writers and returned, called as
train.py::do_evaluation calls it -- save_seperate_videos(render_results, path, num_timestamps, keys=[all seven], num_cams=3, fps=24)
-- with `imageio` replaced by a stub whose get_writer records every append_data, and with empty stub modules for what that file imports
for other functions (plyfile, skimage, lpipsPyTorch, gaussian_renderer, plotly, cv2, and whatever else of its import list the
container lacks).  render_results is filled the way render_func fills it (utils/video_utils.py:176-201): `permute(1, 2, 0).cpu()
.numpy()` of the [C,H,W] torch images, the depth divided in place by its own max().  Without the reference tree this script refuses
to run.

Per size s{H}x{W} of frames_ref.SIZES, 2 timestamps x 3 cameras: s.._in_{key} [6,C,H,W] fp32 (the device-layout images; the RAW
depths for "depths"), s.._frames_{key} [2, H, 3 W, C] uint8 (every frame the key's writer received), s.._middle_{key} (the returned
frame).  The script asserts that tests/frames_ref.py reproduces every recorded frame exactly, and the input shares below (asserted
again in tests/test_frames_cpu.py: frames_ref.check_inputs):

  * RGB values span [-0.2, 1.2] with at least 5 % of the samples below 0 and 5 % above 1; exact 0, exact 1, -0.0, a denormal, and
    k / 255 with its two fp32 neighbours for k in PLANTED_K are present;
  * on at least 40 % of the in-range samples truncation and round-to-nearest of 255 x give different bytes;
  * every depth image holds at least 3 pixels whose byte under x * (1 / m) differs from the byte under x / m.  Such values are rare
    (a handful in 1e8 uniform draws from [4, m]): they sit where 255 * (x / m) lies within an ulp of an integer, so the search walks
    the fp32 neighbours of m k / 255, k = 1..254, and plants the first few it finds;
  * the three depth images of a strip have different maxima."""
import importlib
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

from tests import frames_ref as fr  # noqa: E402

PLANTED_K = fr.PLANTED_K
f32 = np.float32


class _Stub(types.ModuleType):
    """An empty module: any attribute is a placeholder that is never called here."""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return lambda *a, **k: (_ for _ in ()).throw(RuntimeError(f"stub {self.__name__}.{name} called"))


class _RecordingWriter:
    def __init__(self, log, path):
        self.frames = log.setdefault(path, [])

    def append_data(self, frame):
        self.frames.append(np.array(frame, copy=True))

    def close(self):
        pass


def reference_module(log):
    path = os.path.join(REF, "utils", "video_utils.py")
    if not os.path.isfile(path):
        raise SystemExit(f"{path} is missing: the fixture records the reference's own frames and cannot be written without it")
    for name in ("plyfile", "skimage", "skimage.metrics", "lpipsPyTorch", "gaussian_renderer", "imageio"):
        sys.modules[name] = _Stub(name)
    for name in ("plotly", "plotly.graph_objects", "cv2", "sklearn", "sklearn.cluster", "matplotlib", "matplotlib.cm", "scipy",
                 "scipy.ndimage", "tqdm"):
        try:
            importlib.import_module(name)
        except Exception:
            sys.modules[name] = _Stub(name)
    sys.modules["imageio"].get_writer = lambda p, **kw: _RecordingWriter(log, p)
    if isinstance(sys.modules["tqdm"], _Stub):
        sys.modules["tqdm"].tqdm = lambda x, **k: x
        sys.modules["tqdm"].trange = lambda *a, **k: range(*a)
    sys.path.insert(0, REF)
    try:
        return importlib.import_module("utils.video_utils")
    finally:
        sys.path.remove(REF)


def rgb_images(rng, n, H, W, special):
    x = rng.uniform(-0.2, 1.2, size=(n, 3, H, W)).astype(f32)
    if special:
        v = [f32(0.0), f32(1.0), f32(-0.0), f32(1e-40), f32(-0.2), f32(1.2)]
        for k in PLANTED_K:
            q = f32(k) / f32(255)
            v += [np.nextafter(q, f32(-1)), q, np.nextafter(q, f32(2))]
        flat = x[0].reshape(-1)
        at = rng.choice(flat.size, size=len(v), replace=False)
        flat[at] = np.array(v, f32)
    return x


def reciprocal_candidates(m, spread=256):
    """fp32 values in [4, m) near m k / 255 whose byte differs between x / m and x * (1 / m)."""
    m = f32(m)
    centre = (m * (np.arange(1, 255, dtype=np.float64) / 255.0)).astype(f32).view(np.int32)
    x = (centre[:, None] + np.arange(-spread, spread + 1, dtype=np.int32)[None, :]).reshape(-1).view(f32)
    x = x[(x >= 4) & (x < m)]
    a = (f32(255) * np.clip(x / m, f32(0), f32(1))).astype(np.uint8)
    b = (f32(255) * np.clip(x * (f32(1) / m), f32(0), f32(1))).astype(np.uint8)
    return x[a != b]


def depth_images(rng, n, H, W, size_index):
    out = np.empty((n, 1, H, W), f32)
    for i in range(n):
        m = f32(30.0 + 7.3 * i + 11.9 * size_index + rng.uniform(0, 3))
        cand = reciprocal_candidates(m)
        assert len(cand) >= 3, (m, len(cand))
        d = rng.uniform(4.0, float(m) * 0.999, size=H * W).astype(f32)
        at = rng.choice(d.size, size=6, replace=False)
        d[at[0]] = m
        d[at[1]] = 0.0                                            # a background pixel
        d[at[2:]] = rng.choice(cand, size=4, replace=False)
        assert d.max() == m
        out[i, 0] = d.reshape(H, W)
    return out


def main():
    log = {}
    vu = reference_module(log)
    out = {}
    n, T = fr.NUM_CAMS, fr.NUM_TIMESTAMPS
    for si, (H, W) in enumerate(fr.SIZES):
        rng = np.random.default_rng(900 + 10 * H + W)
        inputs = {k: rgb_images(rng, n * T, H, W, special=True) for k in fr.RGB_KEYS}
        inputs["depths"] = depth_images(rng, n * T, H, W, si)
        below, above, share, planted = fr.check_inputs(inputs)
        # render_results the way render_func fills it (utils/video_utils.py:176-201)
        results = {k: [] for k in fr.KEYS}
        for i in range(n * T):
            for k in fr.RGB_KEYS:
                results[k].append(torch.from_numpy(inputs[k][i].copy()).permute(1, 2, 0).squeeze().cpu().numpy())
            depth_np = torch.from_numpy(inputs["depths"][i].copy()).permute(1, 2, 0).cpu().numpy()
            depth_np /= depth_np.max()
            results["depths"].append(depth_np)
        log.clear()
        path = f"/nonexistent/s{H}x{W}.mp4"
        returned = vu.save_seperate_videos(results, path, num_timestamps=T, keys=list(fr.KEYS), num_cams=n, fps=24)
        tag = f"s{H}x{W}"
        changed = {v: 0 for v in fr.VARIANTS}
        for k in fr.KEYS:
            frames = log[path.replace(".mp4", f"_{k}.mp4")]
            C = 1 if k == "depths" else 3
            assert len(frames) == T and all(f.dtype == np.uint8 and f.shape == (H, n * W, C) for f in frames), (k, len(frames))
            mine = [fr.strip(list(inputs[k][t * n:(t + 1) * n]), normalize=(k == "depths")) for t in range(T)]
            for t in range(T):
                assert np.array_equal(mine[t], frames[t]), (tag, k, t)
            assert np.array_equal(returned[k], frames[T // 2]) and np.array_equal(fr.middle(mine), returned[k])
            for v in fr.VARIANTS:
                changed[v] += sum(int((fr.strip(list(inputs[k][t * n:(t + 1) * n]), normalize=(k == "depths"), variant=v) != frames[t]).sum())
                                  for t in range(T))
            out[f"{tag}_in_{k}"] = inputs[k]
            out[f"{tag}_frames_{k}"] = np.stack(frames)
            out[f"{tag}_middle_{k}"] = np.array(returned[k], copy=True)
        print(f"{tag}: below 0 {below:.3f}, above 1 {above:.3f}, truncation matters on {share:.3f} of the in-range samples, "
              f"reciprocal-sensitive pixels per depth image {planted}; bytes a wrong reading changes: {changed}")
        assert all(c > 0 for c in changed.values()), changed
    dst = os.path.join(HERE, "video_frames.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")
    assert os.path.getsize(dst) < 400 * 1024


if __name__ == "__main__":
    main()
