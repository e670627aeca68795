"""numpy restatement of the coloured depth frames (include/s3g_depthvis.h, s3gaussian_amd/depthvis.py): the contract of the kernels.

The reference: utils/visualization_tools.py:106-194 -- weighted_percentile, visualize_cmap, visualize_depth -- called as its
depth_visualizer does (utils/video_utils.py:27-33), then to8b.  What differs, on purpose:
  * the weights are integers, llrint(clip(A, 0, 1) * 2^30), and their prefix sums exact; the order is (depth, row-major index): the
    reference's fp32 cumsum depends on the order of equal depths and carries about 1e-5 of relative noise into its own bounds;
  * the curve is evaluated in float64 (the reference takes the log of the fp32 image in fp32);
  * only None is a missing bound (the reference's `lo or ...` also replaces a given 0.0);
  * NaN depths take no part in the percentiles.
tests/golden/depthvis.npz records how far the reference's own bytes are from these."""
import numpy as np

EPS = float(np.finfo(np.float32).eps)        # 2^-23
PERCENTILES = (0.5, 99.5)                    # 50 -+ 99.0 / 2: visualize_cmap's percentile=99.0
SCALE = 1 << 30
MAX_PIXELS = 1 << 23


def _plane(a):
    a = np.asarray(a, dtype=np.float32)
    if a.ndim == 3 and a.shape[0] == 1:
        a = a[0]
    assert a.ndim == 2, a.shape
    return a


def weights(alpha):
    """int64 weights of the flattened opacity image; NaN -> 0."""
    a = _plane(alpha).reshape(-1).astype(np.float64)
    with np.errstate(invalid="ignore"):
        c = np.where(np.isnan(a), 0.0, np.minimum(np.maximum(a, 0.0), 1.0))
    return np.rint(c * SCALE).astype(np.int64)


def interp(q, S, x):
    """np.interp(q, S, x) for one q over non-decreasing S (float64, exact integers) in the stated evaluation order."""
    if q < S[0]:
        return float(x[0])
    if q >= S[-1]:
        return float(x[-1])
    j = int(np.searchsorted(S, q, side="right")) - 1        # the last index with S_j <= q
    if q == S[j] or x[j + 1] == x[j]:
        return float(x[j])
    slope = (x[j + 1] - x[j]) / (S[j + 1] - S[j])
    return float(slope * (q - S[j]) + x[j])


def weighted_percentiles(depth, alpha, ps=PERCENTILES):
    """float64 [len(ps)]: the weighted percentiles of the depth image; NaN when no pixel takes part."""
    d = _plane(depth).reshape(-1)
    if d.size > MAX_PIXELS:
        raise ValueError(f"weighted_percentiles: {d.size} pixels (at most 2^23)")
    w = weights(alpha)
    assert w.size == d.size
    keep = ~np.isnan(d)
    if not keep.any():
        return np.full(len(ps), np.nan)
    x = d[keep].astype(np.float64) + 0.0                    # -0.0 + 0.0 = +0.0
    order = np.argsort(x, kind="stable")
    x = x[order]
    S = np.cumsum(w[keep][order], dtype=np.int64)
    total = int(S[-1])
    Sd = S.astype(np.float64)                               # exact: total <= 2^53
    with np.errstate(all="ignore"):
        return np.array([interp(p * (float(total) / 100.0), Sd, x) for p in ps], dtype=np.float64)


def bounds(depth, alpha, lo, hi):
    """(lo, hi) as float64: a given bound as given, a None one from the weighted percentiles."""
    if lo is None or hi is None:
        if alpha is None:
            raise ValueError("an automatic bound needs alpha")
        lo_auto, hi_auto = weighted_percentiles(depth, alpha)
        lo = lo_auto - EPS if lo is None else float(lo)
        hi = hi_auto + EPS if hi is None else float(hi)
    return np.float64(lo), np.float64(hi)


def u256(depth, alpha, lo, hi):
    """u * 256 per pixel, float64 [H,W]: the number the table index is truncated from."""
    d = _plane(depth).astype(np.float64)
    lo, hi = bounds(depth, alpha, lo, hi)
    with np.errstate(all="ignore"):
        v = -np.log(d + 1e-6)
        c_lo, c_hi = -np.log(lo + 1e-6), -np.log(hi + 1e-6)
        t = np.nan_to_num(np.clip((v - np.minimum(c_lo, c_hi)) / np.abs(c_hi - c_lo), 0, 1))
        u = t if alpha is None else t * _plane(alpha).astype(np.float64)
        return u * 256.0


def near_step(x):
    """Pixels whose u * 256 lies within 1e-9 of a table step: a last-bit difference of the logarithm may move them by one entry."""
    with np.errstate(invalid="ignore"):
        return (x > 0) & (x < 256) & (np.abs(x - np.rint(x)) < 1e-9)


def index(x):
    """Table index of u * 256 (NaN: 0; the caller blanks those pixels)."""
    with np.errstate(invalid="ignore"):
        return np.clip(np.trunc(np.nan_to_num(x, nan=0.0, posinf=256.0, neginf=-1.0)), 0, 255).astype(np.int64)


def colors(depth, alpha, lo, hi, table):
    """uint8 [H,W,3]: to8b(visualize_depth(depth, alpha, lo, hi, -log(x + 1e-6))) in the arithmetic above."""
    x = u256(depth, alpha, lo, hi)
    out = np.asarray(table, dtype=np.uint8)[index(x)]
    out[np.isnan(x)] = 0
    return out


def steps_apart(a, b, table):
    """Per pixel, the smallest |i - j| over table entries i, j with table[i] == a and table[j] == b (the table's rows are distinct, so
    this is the index distance); -1 where a colour is not in the table."""
    table = np.asarray(table, dtype=np.int64)
    code = {int(r[0]) << 16 | int(r[1]) << 8 | int(r[2]): k for k, r in enumerate(table)}
    def idx(img):
        c = img.astype(np.int64)
        c = c[..., 0] << 16 | c[..., 1] << 8 | c[..., 2]
        return np.vectorize(lambda v: code.get(int(v), -10_000))(c)
    ia, ib = idx(a), idx(b)
    return np.where((ia < 0) | (ib < 0), -1, np.abs(ia - ib))


def street(H, W, seed):
    """A seeded street-like frame: positive depths that fall with the image row (far at the top, near at the bottom), opacity rising
    from about 0.2 at the top to 1."""
    rng = np.random.default_rng(seed)
    row = np.linspace(0.0, 1.0, H)[:, None]
    depth = (3.0 + 150.0 * (1.0 - row) ** 2) * np.exp(0.15 * rng.standard_normal((H, W)))
    alpha = np.clip(0.2 + 0.9 * row + 0.05 * rng.standard_normal((H, W)), 0.0, 1.0)
    return depth.astype(np.float32), alpha.astype(np.float32)


def check_against_reference(mine, golden, name, kind):
    """The bars of the issue: no pixel more than one table step from the reference's byte, and at most 4 x the recorded share of
    differing pixels (at least one pixel is allowed)."""
    ref, table = golden[f"{name}_{kind}_bytes"], golden["table"]
    assert mine.shape == ref.shape and mine.dtype == np.uint8
    steps = steps_apart(mine, ref, table)
    differ = np.any(mine != ref, axis=-1)
    allowed = max(4 * int(golden[f"{name}_{kind}_mismatch_pixels"]), 1)
    print(f"{name} {kind}: {int(differ.sum())} pixels differ (allowed {allowed}), largest step {int(steps.max())}")
    assert steps.min() >= 0 and steps.max() <= 1, (name, kind, np.unique(steps))
    assert int(differ.sum()) <= allowed, (name, kind, int(differ.sum()), allowed)
