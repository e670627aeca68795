"""CPU-only: the restatement of the coloured depth frames (tests/depthvis_ref.py) against the reference's recorded bytes
(tests/golden/depthvis.npz, written by tests/golden/make_golden_depthvis.py from the reference's own visualization_tools.py), against a
plain np.interp on float64 prefix sums, and the refusals of s3gaussian_amd.depthvis and its entry points that need no GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import depthvis_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("s37x53", "s96x144")
BOUNDS = {"fixed": (4.0, 120.0), "auto": (None, None)}


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "depthvis.npz")))


@pytest.mark.parametrize("kind", sorted(BOUNDS))
@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_the_reference_bytes(golden, name, kind):
    lo, hi = BOUNDS[kind]
    mine = dr.colors(golden[f"{name}_depth"], golden[f"{name}_alpha"], lo, hi, golden["table"])
    dr.check_against_reference(mine, golden, name, kind)


@pytest.mark.parametrize("name", CASES)
def test_restatement_percentiles_match_the_reference(golden, name):
    ref = golden[f"{name}_percentiles"]
    mine = dr.weighted_percentiles(golden[f"{name}_depth"], golden[f"{name}_alpha"])
    rel = np.abs(mine - ref) / np.abs(ref)
    bar = 4 * float(golden[f"{name}_percentile_rel"])        # the recorded distance is the reference's own fp32 cumsum noise
    print(f"{name}: relative distances {rel}, bar {bar:.3e}")
    assert np.all(rel <= bar), (rel, bar)


def test_table_is_matplotlibs_turbo_and_the_librarys(golden):
    import matplotlib
    from s3gaussian_amd import depthvis
    lut = matplotlib.colormaps["turbo"](np.arange(256))[:, :3]
    table = (255 * np.clip(lut, 0, 1)).astype(np.uint8)
    assert np.array_equal(golden["table"], table)
    assert depthvis.TABLE.shape == (256, 3) and depthvis.TABLE.dtype == np.uint8 and np.array_equal(depthvis.TABLE, table)
    # what the colormap call does to a float: entry trunc(u * 256), under -> 0, over -> 255
    u = np.array([-0.5, 0.0, 0.2, 0.999, 1.0, 1.5])
    assert np.array_equal((255 * np.clip(matplotlib.colormaps["turbo"](u)[:, :3], 0, 1)).astype(np.uint8), table[dr.index(u * 256)])


def plain_interp(depth, alpha):
    """weighted_percentile of the reference on float64 sums of the integer weights, stable order, NaN depths dropped."""
    d = np.asarray(depth, np.float32).reshape(-1)
    w = dr.weights(np.asarray(alpha, np.float32).reshape(1, -1)).astype(np.float64)
    keep = ~np.isnan(d)
    x, w = d[keep].astype(np.float64), w[keep]
    order = np.argsort(x, kind="stable")
    x, w = x[order], w[order]
    acc = np.cumsum(w)
    return np.interp(np.array(dr.PERCENTILES) * (acc[-1] / 100), acc, x)


@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (3, 5), (37, 53), (64, 64)])
@pytest.mark.parametrize("kind", ["tie_free", "eight_values", "two_values", "zero_weights_between"])
def test_restatement_equals_np_interp_exactly(shape, kind):
    rng = np.random.default_rng(1000 * shape[0] + shape[1] + 100_000 * len(kind))
    n = shape[0] * shape[1]
    if kind == "tie_free":
        depth = rng.permutation(np.linspace(0.5, 150.0, n)).astype(np.float32)
        assert len(np.unique(depth)) == n
    elif kind == "eight_values":
        depth = rng.choice(np.linspace(2.0, 90.0, 8), size=n).astype(np.float32)
    elif kind == "two_values":
        depth = rng.choice([3.5, 77.25], size=n).astype(np.float32)
    else:
        depth = rng.choice(np.linspace(2.0, 90.0, 8), size=n).astype(np.float32)
    alpha = rng.uniform(0.0, 1.0, size=n).astype(np.float32)
    if kind == "zero_weights_between":
        alpha[rng.uniform(size=n) < 0.6] = 0.0
        alpha[0] = 0.7
    mine = dr.weighted_percentiles(depth.reshape(shape), alpha.reshape(shape))
    assert np.array_equal(mine, plain_interp(depth, alpha)), (mine, plain_interp(depth, alpha))


def test_restatement_edge_rules():
    one = np.ones((2, 3), np.float32)
    d = np.array([[5.0, np.nan, 1.0], [3.0, 2.0, 4.0]], np.float32)
    assert np.all(np.isnan(dr.weighted_percentiles(np.full((2, 3), np.nan, np.float32), one)))
    assert np.array_equal(dr.weighted_percentiles(d, 0 * one), [5.0, 5.0])                 # total = 0: x_last
    w = np.zeros((2, 3), np.float32)
    w[1, 0] = 1.0                                                                        # the only weight sits on depth 3
    # q < total everywhere; the crossing pixel is 3.0 and its predecessor 2.0, S_j = 0: slope * q + 2
    q = np.array(dr.PERCENTILES) * (float(1 << 30) / 100.0)
    assert np.array_equal(dr.weighted_percentiles(d, w), (1.0 / float(1 << 30)) * q + 2.0)
    z = np.array([[-0.0, 0.0, 1.0]], np.float32)
    r = dr.weighted_percentiles(z, np.array([[1.0, 1.0, 0.0]], np.float32))
    assert np.array_equal(r, [0.0, 0.0]) and not np.signbit(r).any()
    assert np.array_equal(dr.weights(np.array([[np.nan, -1.0, 2.0, 2.0 ** -31, 1.5 * 2.0 ** -30, 1.0]], np.float32)),
                          [0, 0, 1 << 30, 0, 2, 1 << 30])
    # only None is a missing bound: a given 0.0 stays
    lo, hi = dr.bounds(d, one, 0.0, None)
    assert lo == 0.0 and hi == dr.weighted_percentiles(d, one)[1] + dr.EPS
    with pytest.raises(ValueError):
        dr.bounds(d, None, None, 1.0)


def test_python_refusals_without_a_gpu():
    from s3gaussian_amd import depthvis
    d, a = torch.rand(4, 6), torch.rand(4, 6)
    with pytest.raises(RuntimeError, match="GPU"):
        depthvis.depth_colors(d, a)
    with pytest.raises(RuntimeError, match="GPU"):
        depthvis.weighted_percentiles(d, a)
    with pytest.raises(RuntimeError, match="GPU"):
        depthvis.depth_colors(None)


def test_entry_points_refuse_before_any_device_call():
    """include/s3g_depthvis.h: everything invalid is S3G_ERR_INVALID_ARG before a device call, so none of this needs a GPU."""
    from s3gaussian_amd import _lib, depthvis
    L = depthvis._bind()
    for name in ("s3g_depthvis_workspace_bytes", "s3g_depth_percentiles", "s3g_depth_colors", "s3g_depth_turbo_table"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name)
    INVALID = 1
    word = (C.c_double * 4)()
    some = C.cast(word, C.c_void_p)
    nan = float("nan")
    err = lambda: L.s3g_last_error().decode()
    assert L.s3g_depthvis_workspace_bytes(0, 4) == 0 and L.s3g_depthvis_workspace_bytes(4, -1) == 0
    assert L.s3g_depthvis_workspace_bytes(2048, 4096) > 0 and L.s3g_depthvis_workspace_bytes(2048, 4097) == 0      # 2^23 and beyond
    small, full = L.s3g_depthvis_workspace_bytes(1, 1), L.s3g_depthvis_workspace_bytes(1066, 1600)
    assert 0 < small < full and small % 128 == 0 and full % 128 == 0
    # percentiles
    assert L.s3g_depth_percentiles(0, 4, some, some, some, some, None) == INVALID and "H = 0" in err()
    assert L.s3g_depth_percentiles(2048, 4097, some, some, some, some, None) == INVALID and "2^23" in err()
    for k in range(4):
        args = [some] * 4
        args[k] = None
        assert L.s3g_depth_percentiles(4, 4, *args, None) == INVALID and "NULL" in err()
    # colours
    assert L.s3g_depth_colors(4, 0, some, some, 4.0, 120.0, None, some, 12, 0, None) == INVALID and "W = 0" in err()
    assert L.s3g_depth_colors(4, 4, None, some, 4.0, 120.0, None, some, 12, 0, None) == INVALID and "NULL depth" in err()
    assert L.s3g_depth_colors(4, 4, some, some, 4.0, 120.0, None, None, 12, 0, None) == INVALID and "NULL depth or dst" in err()
    assert L.s3g_depth_colors(4, 4, some, some, nan, 120.0, None, some, 12, 0, None) == INVALID and "bounds is NULL" in err()
    assert L.s3g_depth_colors(4, 4, some, some, 4.0, nan, None, some, 12, 0, None) == INVALID and "bounds is NULL" in err()
    assert L.s3g_depth_colors(4, 4, some, None, nan, 120.0, some, some, 12, 0, None) == INVALID and "alpha may be NULL only" in err()
    assert L.s3g_depth_colors(4, 4, some, some, 4.0, 120.0, None, some, 12, -1, None) == INVALID and "do not fit" in err()
    assert L.s3g_depth_colors(4, 4, some, some, 4.0, 120.0, None, some, 11, 0, None) == INVALID and "do not fit" in err()
    assert L.s3g_depth_colors(4, 4, some, some, 4.0, 120.0, None, some, 36, 9, None) == INVALID and "do not fit" in err()


def test_evaluate_video_refuses_depth_keys_by_name():
    """The key check comes before anything touches a device."""
    from s3gaussian_amd import pipeline
    assert pipeline.DEPTH_VIDEO_KEYS == ("depth_colors",)
    with pytest.raises(RuntimeError, match="depth_colours_please"):
        pipeline.evaluate_video(None, [], [], None, None, keys=("rgbs",), depth_keys=("depth_colours_please",))
    with pytest.raises(RuntimeError, match="depth_keys="):
        pipeline.evaluate_video(None, [], [], None, None, keys=("rgbs", "depth_colors"))
    with pytest.raises(RuntimeError, match="depth_bounds"):
        pipeline.evaluate_video(None, [], [], None, None, keys=("rgbs",), depth_keys=("depth_colors",), depth_bounds=(4.0,))
