"""Pure-numpy restatement of the bytes the reference hands to its video writers: the checker of s3gaussian_amd.frames on a machine
that has neither the reference tree nor a GPU.  Images come in the device layout, fp32 [C,H,W].

  to8b(x)             utils/visualization_tools.py:68-71     (255 * np.clip(x, 0, 1)).astype(np.uint8): fp32 multiply, truncation
  hwc(image)          utils/video_utils.py:180-192           get_numpy(image.permute(1, 2, 0))
  normalise_depth(d)  utils/video_utils.py:196-198           depth.permute(1, 2, 0).cpu().numpy(), `/=` its own max(): fp32 division
  strip(images)       utils/video_utils.py:465, 480, 489     to8b(np.concatenate(frames, axis=1)) of one timestamp's num_cams frames
  middle(strips)      utils/video_utils.py:449, 491-492      the strip of timestamp num_timestamps // 2

tests/golden/video_frames.npz records what the reference's own save_seperate_videos appended to its writers for generated inputs
(tests/golden/make_golden_frames.py); tests/test_frames_cpu.py compares this restatement with those recordings byte for byte.
`variant` switches ONE step to a plausible wrong reading; test_frames_cpu.py shows that each changes bytes of the fixture."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "video_frames.npz")
KEYS = ("gt_rgbs", "rgbs", "depths", "dynamic_rgbs", "static_rgbs", "forward_flows", "backward_flows")
RGB_KEYS = tuple(k for k in KEYS if k != "depths")
SIZES = ((5, 7), (6, 8))          # (H, W): W % 4 != 0 takes the kernel's byte path, W % 4 == 0 its packed path
NUM_CAMS, NUM_TIMESTAMPS = 3, 2
VARIANTS = ("round", "reciprocal", "strip_max")
PLANTED_K = (1, 7, 128, 200, 254)     # k / 255 and its two fp32 neighbours are among the RGB inputs

f32 = np.float32


def to8b(x, variant=None):
    x = np.asarray(x, f32)
    with np.errstate(invalid="ignore"):
        y = f32(255) * np.clip(x, f32(0), f32(1))
        if variant == "round":
            y = np.rint(y)
        return y.astype(np.uint8)


def hwc(image):
    return np.array(np.asarray(image, f32).transpose(1, 2, 0), order="C", copy=True)     # never a view: normalise_depth divides in place


def normalise_depth(depth, variant=None, strip_max=None):
    d = hwc(depth)
    m = d.max() if strip_max is None else f32(strip_max)
    with np.errstate(invalid="ignore", divide="ignore"):
        if variant == "reciprocal":
            d *= f32(1) / m
        else:
            d /= m
    return d


def strip(images, normalize=False, variant=None):
    """[H, len(images) * W, C] uint8 of one timestamp: images are the cameras' [C,H,W] fp32 arrays."""
    if normalize:
        smax = max(float(np.asarray(i).max()) for i in images) if variant == "strip_max" else None
        frames = [normalise_depth(i, variant, smax) for i in images]
    else:
        frames = [hwc(i) for i in images]
    return to8b(np.concatenate(frames, axis=1), variant)


def middle(strips):
    return strips[len(strips) // 2]


def tile(image, normalize=False):
    """One camera's [H,W,C] tile."""
    return strip([image], normalize)


def truncation_matters(x):
    """Boolean mask over the in-range (0 < x < 1) samples: truncation and round-to-nearest of 255 x give different bytes."""
    x = np.asarray(x, f32)
    inside = (x > 0) & (x < 1)
    y = f32(255) * x[inside]
    return np.trunc(y) != np.rint(y)


def reciprocal_differs(depth):
    """Boolean [H,W] mask: the byte under x * (1 / m) differs from the byte under x / m."""
    return (to8b(normalise_depth(depth)) != to8b(normalise_depth(depth, "reciprocal")))[..., 0]


def check_inputs(inputs):
    """The shares the docstring promises, for one size's inputs; -> figures for the log."""
    rgb = np.concatenate([inputs[k].reshape(-1) for k in RGB_KEYS])
    below, above = float((rgb < 0).mean()), float((rgb > 1).mean())
    assert rgb.min() == f32(-0.2) and rgb.max() == f32(1.2) and below >= 0.05 and above >= 0.05, (rgb.min(), rgb.max(), below, above)
    bits = set(rgb.view(np.uint32).tolist())
    need = [f32(0.0), f32(1.0), f32(-0.0), f32(1e-40)]
    for k in PLANTED_K:
        q = f32(k) / f32(255)
        need += [np.nextafter(q, f32(-1)), q, np.nextafter(q, f32(2))]
    for v in need:
        assert int(np.array(v, f32).view(np.uint32)) in bits, v
    assert 0 < abs(float(f32(1e-40))) < float(np.finfo(f32).tiny)
    share = float(truncation_matters(rgb).mean())
    assert share >= 0.40, share
    depths = inputs["depths"]
    planted = [int(reciprocal_differs(d).sum()) for d in depths]
    assert min(planted) >= 3, planted
    for t in range(len(depths) // NUM_CAMS):
        maxima = [float(d.max()) for d in depths[t * NUM_CAMS:(t + 1) * NUM_CAMS]]
        assert len(set(maxima)) == NUM_CAMS, maxima
    return below, above, share, planted


def load_fixture(path=FIXTURE):
    """-> {(H, W): {"inputs": {key: [N,C,H,W] fp32}, "frames": {key: [T, H, n W, C] uint8}, "middle": {key: [H, n W, C] uint8}}};
    inputs["depths"] holds the RAW depths."""
    z = np.load(path)
    out = {}
    for H, W in SIZES:
        tag = f"s{H}x{W}"
        out[(H, W)] = {"inputs": {k: z[f"{tag}_in_{k}"] for k in KEYS}, "frames": {k: z[f"{tag}_frames_{k}"] for k in KEYS},
                       "middle": {k: z[f"{tag}_middle_{k}"] for k in KEYS}}
    return out
