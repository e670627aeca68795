"""Pure-numpy fp32 restatement of the reference's scene-flow colours, in TABLE form: the checker of s3gaussian_amd.flow on a machine
that has neither the reference tree nor a GPU.

  colors(dx_a, dx_b) = utils/visualization_tools.py::scene_flow_to_rgb(dx_b - dx_a, background="bright", flow_max_radius=1.0), the
  `flow_visualizer` of utils/video_utils.py:260,277:
    1. f = (flow - min) / (max - min + 1e-6), min / max over all 3P elements
    2. x, y = f[:,0], f[:,1];  r = |x + iy|;  theta = angle(x + iy), + 2 pi where negative
    3. A = theta * (N_COLS - 1) / (2 pi);  hue = WHEEL[trunc(A)] * (1 - fmod(A, 1)) + WHEEL[ceil(A)] * fmod(A, 1)
    4. 255 - r * (255 - hue), and hue * (1 / r) where r > 1;  / 255

The wheel is built here by the reference's rule (six transitions of 15, 6, 4, 11, 13, 6 entries between the primary hues, each a
`linspace(endpoint=False)` truncated to uint8, the first entry appended to close the circle); tests/golden/scene_flow.npz records the
reference's own 56 x 3 wheel and tests/test_flow_cpu.py compares the two exactly.  The kernel (include/s3g_flow.h) uses no table:
`closed_form` below is what it evaluates, and test_flow_cpu.py shows that both forms agree wherever step 1 can put (x, y).
`variant` switches ONE step to a plausible wrong reading; each lands far outside COLOR_BAR on the fixture."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "scene_flow.npz")
SIZES = (1, 2, 63, 64, 65, 257, 1000, 4099)
TRANSITIONS = (15, 6, 4, 11, 13, 6)
VARIANTS = ("dark", "radius3", "per_column", "no_eps")
# 4 x the largest |restatement - reference colours| over the fixture, as tests/golden/make_golden_flow.py measured it (MEASURED_DEV,
# also stored in the fixture as `max_dev`).  One bar for the restatement, the closed form and the kernel; it may never exceed 1e-5:
# a wheel index off by one moves the green channel by 17/255 = 0.067 times r.
MEASURED_DEV = 1.78813934e-07
COLOR_BAR = 4 * MEASURED_DEV
assert COLOR_BAR <= 1e-5

f32 = np.float32


def make_wheel():
    """[56,3] fp32: the 55 wheel entries and the first one again."""
    hues = [np.array(h) for h in ([255, 0, 0], [255, 255, 0], [0, 255, 0], [0, 255, 255], [0, 0, 255], [255, 0, 255], [255, 0, 0])]
    wheel = np.zeros((sum(TRANSITIONS), 3), dtype="uint8")
    start = 0
    for k, length in enumerate(TRANSITIONS):
        wheel[start:start + length] = np.linspace(hues[k], hues[k + 1], length, endpoint=False)    # truncation to uint8
        start += length
    wheel = wheel.astype(f32)
    return np.vstack((wheel, wheel[:1]))


WHEEL = make_wheel()
N_COLS = len(WHEEL) - 1


def normalise(dx_a, dx_b, variant=None):
    flow = np.asarray(dx_b, f32) - np.asarray(dx_a, f32)
    if flow.size == 0:
        return flow
    eps = f32(0.0) if variant == "no_eps" else f32(1e-6)
    if variant == "per_column":
        lo, hi = flow.min(axis=0, keepdims=True), flow.max(axis=0, keepdims=True)
    else:
        lo, hi = flow.min(), flow.max()
    with np.errstate(invalid="ignore", divide="ignore"):
        return ((flow - lo) / (hi - lo + eps)).astype(f32)


def table_form(x, y, r=None, variant=None):
    """Steps 2-4 for normalised components x, y (fp32 arrays of one shape) -> [...,3]."""
    x, y = np.asarray(x, f32), np.asarray(y, f32)
    if r is None:
        r = np.hypot(x, y).astype(f32)
    ang = np.arctan2(y, x).astype(f32)
    ang = np.where(ang < 0, ang + f32(2 * np.pi), ang).astype(f32)
    ang = ang * f32((N_COLS - 1) / (2 * np.pi))
    lo, hi = np.trunc(ang), np.ceil(ang)
    frac = np.fmod(ang, f32(1))[..., None]
    index = lambda k: np.clip(np.nan_to_num(k, nan=0.0), 0, N_COLS).astype(np.int64)     # (NaN only under variant="no_eps" on a zero flow)
    hue = WHEEL[index(lo)] * (f32(1) - frac) + WHEEL[index(hi)] * frac
    rr = r[..., None]
    over = r > 1
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = (f32(1) / r)[..., None]
        if variant == "dark":
            c = hue * rr
            c[over] = (f32(255.0) - inv * (f32(255.0) - hue))[over]
        else:
            c = f32(255.0) - rr * (f32(255.0) - hue)
            c[over] = (hue * inv)[over]
    return (c / f32(255.0)).astype(f32)


def closed_form(x, y):
    """What the kernel evaluates: the red -> yellow transition's entries are (255, 17 k, 0), so no table is read; radius and angle
    are evaluated in double and rounded to fp32 once, everything else is fp32 in the reference's order."""
    x, y = np.asarray(x, f32), np.asarray(y, f32)
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    r = np.sqrt(xd * xd + yd * yd).astype(f32)
    A = np.arctan2(yd, xd).astype(f32) * f32((N_COLS - 1) / (2 * np.pi))
    lo, hi = np.trunc(A), np.ceil(A)
    frac = A - lo
    g = (f32(17) * lo) * (f32(1) - frac) + (f32(17) * hi) * frac
    zero = np.zeros_like(r)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = f32(1) / r
        bright = np.stack([f32(255) - r * zero, f32(255) - r * (f32(255) - g), f32(255) - r * f32(255)], axis=-1)
        dim = np.stack([f32(255) * inv, g * inv, zero * inv], axis=-1)
    return (np.where((r > 1)[..., None], dim, bright) / f32(255)).astype(f32)


def colors(dx_a, dx_b, variant=None):
    """[P,3] fp32 colours of the flow dx_b - dx_a."""
    f = normalise(dx_a, dx_b, variant)
    if f.size == 0:
        return np.zeros((0, 3), f32)
    r = np.sqrt((f * f).sum(axis=1)).astype(f32) if variant == "radius3" else None
    return table_form(f[:, 0], f[:, 1], r, variant)


def flow_range(dx_a, dx_b):
    flow = np.asarray(dx_b, f32) - np.asarray(dx_a, f32)
    return flow.min(), flow.max()


def load_fixture():
    """-> (cases, wheel, max_dev); a case is a dict name, dx_a, dx_b, colors (the reference's), min, max."""
    z = np.load(FIXTURE)
    names = [f"p{P}" for P in SIZES] + ["zero", "one_row"]
    cases = [dict(name=n, dx_a=z[f"{n}_dx_a"], dx_b=z[f"{n}_dx_b"], colors=z[f"{n}_colors"], min=z[f"{n}_min"], max=z[f"{n}_max"])
             for n in names]
    return cases, z["wheel"], float(z["max_dev"])
