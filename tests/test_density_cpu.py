"""CPU-only checks of adaptive density control (s3gaussian_amd/density.py, include/s3g_density.h): the fixture recorded from the
reference's own densify / prune / reset_opacity is what its generator says it is, the ctypes mirrors follow the header, CPU tensors
are refused, and `density_control` restates the schedule of train.py:494-516."""
import ctypes
import importlib.util
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "density_control.npz")


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_density", os.path.join(ROOT, "tests", "golden", "make_golden_density.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _inputs(f):
    return {k: torch.from_numpy(f[k]) for k in ("xyz", "scaling", "rotation", "opacity", "accum", "denom", "max_radii2D", "table")}


def test_fixture_loads_and_is_self_consistent():
    f = np.load(GOLDEN)
    P = int(f["P"])
    assert os.path.getsize(GOLDEN) < 1 << 20
    assert f["xyz"].shape == (P, 3) and f["scaling"].shape == (P, 3) and f["rotation"].shape == (P, 4) and f["opacity"].shape == (P, 1)
    assert f["accum"].shape == (P, 1) and f["denom"].shape == (P, 1) and f["max_radii2D"].shape == (P,) and f["table"].dtype == np.bool_
    assert int((f["denom"] == 0).sum()) > 0                               # rows that were never visible are part of the input
    src, kind = f["densify_src"], f["densify_kind"]
    n_clone, n_split = int((kind == 1).sum()), int((kind == 2).sum())
    assert src.shape == kind.shape == (P + n_clone + n_split,) and int((kind == 3).sum()) == n_split
    # the order contract: [kept originals | clones | children copy 1 | copy 2], each run ascending in its source row
    assert np.all(np.diff(kind.astype(np.int64)) >= 0)
    for k in range(4):
        assert np.all(np.diff(src[kind == k]) > 0)
    assert np.array_equal(src[kind == 2], src[kind == 3])
    assert not np.intersect1d(src[kind == 0], src[kind == 2]).size       # a split row does not survive
    assert np.all(np.isin(src[kind == 1], src[kind == 0]))               # a cloned row does
    assert f["z"].shape == (2 * n_split, 3) and f["child_xyz"].shape == f["child_xyz_f64"].shape == (2 * n_split, 3)
    assert f["child_xyz_f64"].dtype == np.float64 and f["reset_opacity_f64"].dtype == np.float64
    for name in ("xyz", "scaling", "reset"):
        assert 0 < float(f[f"ref_err_{name}"]) < 1e-5
    for tag in ("screen", "none"):
        kept = f[f"prune_kept_{tag}"]
        assert np.all(np.diff(kept) > 0) and 0 <= kept.min() and kept.max() < P
    assert np.all(np.isin(f["prune_kept_screen"], f["prune_kept_none"]))  # the size tests only ever drop more


def test_no_near_ties_flag_and_class_shares_hold_when_recomputed():
    f = np.load(GOLDEN)
    gen = _generator()
    inp = _inputs(f)
    P = int(f["P"])
    assert bool(f["no_near_ties"]) and int(f["ulp_gap"]) == 4 and gen.no_near_ties(inp)
    for name, q, t in gen.decision_quantities(inp):                      # and, independently of the generator's helper:
        qf = q.numpy().astype(np.float32)
        qf = qf[np.isfinite(qf)]
        t32 = np.float32(t)
        lo, hi = t32, t32
        for _ in range(4):
            lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
        assert not np.any((qf >= lo) & (qf <= hi)), name
    shares = gen.class_shares(inp)
    kind = f["densify_kind"]
    assert shares["clone"] == pytest.approx((kind == 1).sum() / P) == pytest.approx(float(f["share_clone"]))
    assert shares["split"] == pytest.approx((kind == 2).sum() / P) == pytest.approx(float(f["share_split"]))
    assert shares["prune_screen"] == pytest.approx(1 - f["prune_kept_screen"].shape[0] / P) == pytest.approx(float(f["share_prune_screen"]))
    assert shares["prune_none"] == pytest.approx(1 - f["prune_kept_none"].shape[0] / P) == pytest.approx(float(f["share_prune_none"]))
    assert all(0.01 <= v <= 0.30 for v in shares.values()), shares


def test_rerunning_the_generator_reproduces_the_fixture():
    gen = _generator()
    if not gen.reference_present():
        pytest.skip("the reference is not on this machine: the fixture cannot be regenerated here")
    import sys
    before = set(sys.modules)
    fresh = gen.generate()
    assert not [m for m in set(sys.modules) - before if m.split(".")[0] in ("scene", "utils", "arguments")]
    f = np.load(GOLDEN)
    assert set(f.files) == set(fresh)
    for k in f.files:
        assert np.array_equal(np.asarray(fresh[k]), f[k]), k


def _struct_fields(name):
    txt = open(os.path.join(ROOT, "include", "s3g_density.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields.append(re.findall(r"[A-Za-z_][A-Za-z0-9_]*", decl)[-1])
    return fields


def test_ctypes_mirrors_follow_the_header_and_symbols_are_exported():
    from s3gaussian_amd import _lib, density
    assert _struct_fields("s3g_density_tensor") == [f[0] for f in density._Tensor._fields_]
    assert _struct_fields("s3g_density_plan") == [f[0] for f in density._Plan._fields_]
    assert ctypes.sizeof(density._Tensor) == 6 * 8 + 2 * 4 and ctypes.sizeof(density._Plan) == 4 * 4 + 13 * 8
    L = density._lib_bound()
    for sym in ("s3g_density_count_words", "s3g_density_classify_densify", "s3g_density_classify_prune", "s3g_density_scan",
                "s3g_density_apply", "s3g_density_reset_opacity"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(L, sym)
    assert L.s3g_density_count_words(0) == 3 and L.s3g_density_count_words(256) == 3 and L.s3g_density_count_words(257) == 6
    # argument validation happens before anything is launched (no GPU needed), with the library's error convention
    assert L.s3g_density_scan(-1, None, None, None) == 1 and b"s3g_density_scan" in L.s3g_last_error()
    plan = density._Plan(P=10, n_clone=8, n_split=8, n_drop=0)
    assert L.s3g_density_apply(ctypes.byref(plan), 0, None, None) == 1 and b"do not fit" in L.s3g_last_error()
    assert L.s3g_density_apply(None, 0, None, None) == 1


def _cpu_model(P=32):
    from s3gaussian_amd.pipeline import GaussianParams, default_hyper, default_opt
    g = torch.Generator().manual_seed(0)
    pc = GaussianParams(3, default_hyper())
    pc.init_from_tensors(torch.randn(P, 3, generator=g), torch.randn(P, 3, generator=g) - 3, torch.randn(P, 4, generator=g),
                         torch.randn(P, 1, generator=g), torch.randn(P, 16, 3, generator=g), "cpu")
    pc.training_setup(default_opt())
    return pc


def test_cpu_tensors_are_refused_not_routed_to_a_slow_path():
    pc = _cpu_model()
    before = pc._xyz
    with pytest.raises(RuntimeError, match="GPU"):
        pc.densify(0.0002, 0.005, 5.0, None, 5, 5, None, 600, "fine")
    with pytest.raises(RuntimeError, match="GPU"):
        pc.prune(0.0002, 0.005, 5.0, 20)
    with pytest.raises(RuntimeError, match="GPU"):
        pc.reset_opacity()
    assert pc._xyz is before and pc._xyz.shape[0] == 32


def test_percent_dense_is_a_class_default_that_training_setup_overrides():
    from s3gaussian_amd.density import default_density_opt
    from s3gaussian_amd.pipeline import GaussianParams, default_opt
    assert GaussianParams.percent_dense == 0.01
    pc = _cpu_model()
    assert pc.percent_dense == 0.01                        # default_opt carries no percent_dense: the class default stands
    o = default_opt()
    o.percent_dense = 0.02
    pc.training_setup(o)
    assert pc.percent_dense == 0.02 and GaussianParams.percent_dense == 0.01
    d = default_density_opt(pruning_interval=200)
    assert (d.percent_dense, d.densification_interval, d.opacity_reset_interval, d.pruning_interval, d.pruning_from_iter,
            d.densify_from_iter, d.densify_until_iter) == (0.01, 100, 3000, 200, 500, 500, 25_000)
    assert (d.densify_grad_threshold_coarse, d.densify_grad_threshold_fine_init, d.densify_grad_threshold_after,
            d.opacity_threshold_coarse, d.opacity_threshold_fine_init, d.opacity_threshold_fine_after) == (0.0002,) * 3 + (0.005,) * 3
    assert not hasattr(default_opt(), "densify_until_iter")             # default_opt stays as it was


class _Recorder:
    """Stands where the model stands: records what density_control asks of it."""

    def __init__(self, P=100_000):
        self.get_xyz = SimpleNamespace(shape=(P, 3))
        self.calls = []

    def densify(self, *a):
        self.calls.append(("densify",) + a)

    def prune(self, *a):
        self.calls.append(("prune",) + a)

    def reset_opacity(self):
        self.calls.append(("reset",))


# worked out by hand from train.py:494-516 for: densify_grad_threshold_fine_init 0.0004 -> after 0.0002, opacity_threshold_fine_init
# 0.01 -> after 0.005 over densify_until_iter = 25 000 (the coarse pair 0.0002 / 0.005), from_iter 500 for both, reset every 3000.
#   iteration, stage, P, pruning_interval -> densify?, prune?, reset?, densify threshold, opacity threshold, size threshold
SCHEDULE = [
    (100, "fine", 100_000, 100, False, False, False, 0.0004 - 100 * 8e-9, 0.01 - 100 * 2e-7, None),       # before from_iter
    (500, "fine", 100_000, 100, False, False, False, 0.000396, 0.0099, None),                             # `>` from_iter, not `>=`
    (600, "fine", 100_000, 100, True, True, False, 0.0003952, 0.00988, None),
    (650, "fine", 100_000, 100, False, False, False, 0.0003948, 0.00987, None),                           # off the interval
    (3000, "fine", 100_000, 100, True, True, True, 0.000376, 0.0094, None),                               # size test only AFTER 3000
    (3100, "fine", 100_000, 100, True, True, False, 0.0003752, 0.00938, 20),
    (6000, "coarse", 100_000, 100, True, True, True, 0.0002, 0.005, 20),                                  # coarse: fixed thresholds
    (24000, "fine", 100_000, 100, True, True, True, 0.000208, 0.0052, 20),
    (25000, "fine", 100_000, 100, False, False, False, None, None, None),                                 # densify_until_iter: nothing
    (27000, "fine", 100_000, 100, False, False, False, None, None, None),                                 # ... not even the reset
    (600, "fine", 2_000_000, 100, False, True, False, 0.0003952, 0.00988, None),                          # the `< 2 000 000` cap
    (600, "fine", 1_999_999, 100, True, True, False, 0.0003952, 0.00988, None),
    (700, "fine", 100_000, 200, True, False, False, 0.0003944, 0.00986, None),                            # separate intervals
    (800, "fine", 100_000, 200, True, True, False, 0.0003936, 0.00984, None),
]


@pytest.mark.parametrize("row", SCHEDULE, ids=lambda r: f"it{r[0]}-{r[1]}-P{r[2]}-pi{r[3]}")
def test_density_control_restates_the_reference_schedule(row):
    from s3gaussian_amd.density import default_density_opt, density_control
    it, stage, P, prune_every, want_d, want_p, want_r, d_th, o_th, size = row
    opt = default_density_opt(densify_grad_threshold_fine_init=0.0004, opacity_threshold_fine_init=0.01, pruning_interval=prune_every)
    rec = _Recorder(P)
    out = density_control(rec, it, opt, stage, 7.5)
    kinds = [c[0] for c in rec.calls]
    assert kinds == [k for k, w in (("densify", want_d), ("prune", want_p), ("reset", want_r)) if w]       # and in that order
    assert bool(out["densify"]) == want_d and bool(out["prune"]) == want_p and out["reset"] == want_r
    for c in rec.calls:
        if c[0] == "densify":     # gaussians.densify(densify_threshold, opacity_threshold, extent, size_threshold, 5, 5, model_path, iteration, stage)
            assert c[1] == pytest.approx(d_th, rel=1e-12) and c[2] == pytest.approx(o_th, rel=1e-12)
            assert c[3:] == (7.5, size, 5, 5, None, it, stage)
        if c[0] == "prune":       # gaussians.prune(densify_threshold, opacity_threshold, extent, size_threshold)
            assert c[1] == pytest.approx(d_th, rel=1e-12) and c[2] == pytest.approx(o_th, rel=1e-12) and c[3:] == (7.5, size)
    if d_th is not None:
        assert out["densify_threshold"] == pytest.approx(d_th, rel=1e-12) and out["opacity_threshold"] == pytest.approx(o_th, rel=1e-12)
        assert out["size_threshold"] == size
