"""Adaptive density control on the GPU (s3gaussian_amd/density.py, include/s3g_density.h) against the fixture recorded from the
reference's own `GaussianModel.densify / prune / reset_opacity` (tests/golden/make_golden_density.py), plus the Philox path, the
edges, the operation inside the training loops and a full-size run.

Bounds.  Classes, row order and every copied value are EXACT (the fixture's generator asserts that no decision quantity lies within
4 fp32 ulp of its threshold).  The three computed quantities -- children xyz, children scaling, reset opacities -- are compared with
the float64 evaluation stored in the fixture and may differ from it by at most  2 * ref_err + 1 ulp of the value,  ref_err being the
reference's own fp32 rounding error against the same float64 values: our kernel rounds in another order and uses the device's
exp / log / sqrt, which twice the reference's own error bounds without admitting a wrong formula.  The measured worst cases are
printed by the tests."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "density_control.npz")
ATTRS = {"xyz": "_xyz", "f_dc": "_features_dc", "f_rest": "_features_rest", "opacity": "_opacity", "scaling": "_scaling",
         "rotation": "_rotation"}
STEP = 3.0


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_density", os.path.join(ROOT, "tests", "golden", "make_golden_density.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _row_coded(shape, offset, dev):
    """value = 64 * row + column + offset: exact in fp32 for the sizes used here, so a misplaced row OR column shows."""
    P = shape[0]
    w = int(np.prod(shape[1:])) if len(shape) > 1 else 1
    v = torch.arange(P, dtype=torch.float32)[:, None] * 64.0 + torch.arange(w, dtype=torch.float32)[None, :] + offset
    return v.reshape(shape).to(dev)


def _fixture_model(dev, stepped=True):
    """The fixture's decision inputs in a GaussianParams; features and Adam moments row-coded; `step` = 3 for every parameter."""
    from s3gaussian_amd.pipeline import GaussianParams, default_hyper, default_opt
    f = np.load(GOLDEN)
    P = int(f["P"])
    t = lambda k: torch.from_numpy(f[k])
    pc = GaussianParams(3, default_hyper())
    pc.init_from_tensors(t("xyz"), t("scaling"), t("rotation"), t("opacity"), _row_coded((P, 16, 3), 0.0, "cpu"), dev)
    pc._deformation_table = t("table").to(dev)
    pc.training_setup(default_opt())
    pc.xyz_gradient_accum, pc.denom, pc.max_radii2D = t("accum").to(dev), t("denom").to(dev), t("max_radii2D").to(dev)
    if stepped:
        for attr in ATTRS.values():
            p = getattr(pc, attr)
            pc.optimizer.state[p] = {"step": torch.tensor(STEP), "exp_avg": _row_coded(tuple(p.shape), 0.25, dev),
                                     "exp_avg_sq": _row_coded(tuple(p.shape), 0.5, dev)}
    return pc, f


def _snapshot(pc):
    snap = {}
    for name, attr in ATTRS.items():
        p = getattr(pc, attr)
        st = pc.optimizer.state.get(p, None)
        snap[name] = (p, p.detach().clone(), st["exp_avg"].clone() if st else None, st["exp_avg_sq"].clone() if st else None)
    snap["accum"], snap["denom"], snap["radii"] = pc.xyz_gradient_accum.clone(), pc.denom.clone(), pc.max_radii2D.clone()
    snap["table"] = pc._deformation_table.clone()
    return snap


def _check_surgery(pc, snap):
    """The reference's optimizer surgery: fresh Parameters in the single-parameter groups, state re-keyed, `step` untouched."""
    groups = {g["name"]: g for g in pc.optimizer.param_groups}
    for name, attr in ATTRS.items():
        p = getattr(pc, attr)
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.grad is None and p.is_contiguous()
        assert groups[name]["params"][0] is p and p is not snap[name][0]
        assert snap[name][0] not in pc.optimizer.state
        if snap[name][2] is not None:
            assert float(pc.optimizer.state[p]["step"]) == STEP
    assert len(groups["deformation"]["params"]) > 1 and len(groups["grid"]["params"]) > 1       # left alone


def _within(got, f64, ref_err, what):
    """|got - float64| <= 2 * ref_err + 1 ulp(value); prints the measured worst case."""
    got64 = got.detach().cpu().double().numpy()
    err = np.abs(got64 - f64)
    ulp = np.spacing(np.abs(f64).astype(np.float32)).astype(np.float64)
    bound = 2.0 * float(ref_err) + ulp
    print(f"{what}: worst |ours - float64| = {err.max():.3e} (reference's own: {float(ref_err):.3e}; bound 2 * ref_err + 1 ulp, "
          f"worst ratio to the bound {float((err / bound).max()):.3f})")
    assert np.all(err <= bound), (what, float(err.max()), float((err / bound).max()))


def test_densify_matches_the_reference_fixture(gpu_device):
    dev = gpu_device
    pc, f = _fixture_model(dev)
    snap = _snapshot(pc)
    P = int(f["P"])
    src = torch.from_numpy(f["densify_src"].astype(np.int64)).to(dev)
    kind = torch.from_numpy(f["densify_kind"].astype(np.int64)).to(dev)
    n_clone, n_split = int((kind == 1).sum()), int((kind == 2).sum())
    out = pc.densify(float(f["max_grad"]), float(f["min_opacity"]), float(f["extent"]), None, 5, 5, None, 1000, "fine",
                     noise=torch.from_numpy(f["z"]).to(dev))
    assert out == {"clone": n_clone, "split": n_split, "P": P + n_clone + n_split} and pc._xyz.shape[0] == src.shape[0]
    _check_surgery(pc, snap)
    child = kind >= 2
    for name, attr in ATTRS.items():
        new = getattr(pc, attr).detach()
        _, old, m, v = snap[name]
        rows = ~child if name in ("xyz", "scaling") else torch.ones_like(child)
        assert new.shape[1:] == old.shape[1:]
        assert torch.equal(new[rows], old[src[rows]]), name                              # bit-equal to the gathered input
        st = pc.optimizer.state[getattr(pc, attr)]
        for key, before in (("exp_avg", m), ("exp_avg_sq", v)):
            assert torch.equal(st[key][kind == 0], before[src[kind == 0]]), (name, key)  # survivors keep their moments
            assert float(st[key][kind > 0].abs().max()) == 0.0, (name, key)              # clones and children start from zero
    Pn = src.shape[0]
    assert pc.xyz_gradient_accum.shape == (Pn, 1) and pc.denom.shape == (Pn, 1) and pc.max_radii2D.shape == (Pn,)
    assert float(pc.xyz_gradient_accum.abs().max()) == 0 and float(pc.denom.abs().max()) == 0 and float(pc.max_radii2D.abs().max()) == 0
    assert pc._deformation_table.dtype == torch.bool and torch.equal(pc._deformation_table, snap["table"][src])
    _within(pc._xyz.detach()[child], f["child_xyz_f64"], f["ref_err_xyz"], "children xyz")
    _within(pc._scaling.detach()[child], f["child_scaling_f64"], f["ref_err_scaling"], "children scaling")


@pytest.mark.parametrize("screen", [20, None])
def test_prune_matches_the_reference_fixture(gpu_device, screen):
    dev = gpu_device
    pc, f = _fixture_model(dev)
    snap = _snapshot(pc)
    kept = torch.from_numpy(f["prune_kept_screen" if screen else "prune_kept_none"].astype(np.int64)).to(dev)
    out = pc.prune(float(f["max_grad"]), float(f["min_opacity"]), float(f["extent"]), screen)
    assert out == {"drop": int(f["P"]) - kept.shape[0], "P": kept.shape[0]} and pc._xyz.shape[0] == kept.shape[0]
    _check_surgery(pc, snap)
    for name, attr in ATTRS.items():
        _, old, m, v = snap[name]
        assert torch.equal(getattr(pc, attr).detach(), old[kept]), name
        st = pc.optimizer.state[getattr(pc, attr)]
        assert torch.equal(st["exp_avg"], m[kept]) and torch.equal(st["exp_avg_sq"], v[kept]), name
    # the accumulators are gathered, not zeroed
    assert torch.equal(pc.xyz_gradient_accum, snap["accum"][kept]) and torch.equal(pc.denom, snap["denom"][kept])
    assert torch.equal(pc.max_radii2D, snap["radii"][kept]) and torch.equal(pc._deformation_table, snap["table"][kept])
    assert float(pc.denom.sum()) > 0


def test_reset_opacity_matches_the_reference_fixture(gpu_device):
    dev = gpu_device
    pc, f = _fixture_model(dev)
    snap = _snapshot(pc)
    pc.reset_opacity()
    p = pc._opacity
    assert p is not snap["opacity"][0] and pc.optimizer.param_groups[5]["params"][0] is p and snap["opacity"][0] not in pc.optimizer.state
    st = pc.optimizer.state[p]
    assert float(st["step"]) == STEP and float(st["exp_avg"].abs().max()) == 0 and float(st["exp_avg_sq"].abs().max()) == 0
    assert st["exp_avg"].shape == p.shape
    _within(p.detach(), f["reset_opacity_f64"], f["ref_err_reset"], "reset opacity")
    for name in ("xyz", "f_dc", "f_rest", "scaling", "rotation"):       # nothing else moves
        assert getattr(pc, ATTRS[name]) is snap[name][0] and torch.equal(getattr(pc, ATTRS[name]).detach(), snap[name][1])


def test_philox_noise_is_reproducible_and_standard_normal(gpu_device):
    dev = gpu_device
    gen = _generator()
    runs = []
    for seed in (1234, 1234, 99):
        pc, f = _fixture_model(dev)
        out = pc.densify(float(f["max_grad"]), float(f["min_opacity"]), float(f["extent"]), None, 5, 5, None, 1000, "fine",
                         seed=seed, return_noise=True)
        runs.append((out, {n: getattr(pc, a).detach().clone() for n, a in ATTRS.items()}))
    (o1, a), (o2, b), (o3, c) = runs
    for n in ATTRS:
        assert torch.equal(a[n], b[n]), n                                  # same seed: bit-identical
    assert torch.equal(o1["noise"], o2["noise"])
    kind = torch.from_numpy(f["densify_kind"].astype(np.int64)).to(dev)
    src = torch.from_numpy(f["densify_src"].astype(np.int64))
    child = kind >= 2
    n_split = int((kind == 2).sum())
    assert not torch.equal(a["xyz"][child], c["xyz"][child]) and not torch.equal(o1["noise"], o3["noise"])      # another seed
    assert torch.equal(a["xyz"][~child], c["xyz"][~child]) and torch.equal(a["scaling"], c["scaling"])
    # the returned deviates reproduce the children through the formula, to the bound of the fixture test
    z = o1["noise"].cpu()
    assert z.shape == (2 * n_split, 3)
    inp = {k: torch.from_numpy(f[k]) for k in ("xyz", "scaling", "rotation")}
    xyz64, scaling64 = gen.children_float64(inp, src[child.cpu()], z)
    _within(a["xyz"][child], xyz64.numpy(), f["ref_err_xyz"], "children xyz from noise_out")
    _within(a["scaling"][child], scaling64.numpy(), f["ref_err_scaling"], "children scaling (Philox run)")
    # 5-sigma bounds of the estimators over the n = 6 * n_split values; the seed is fixed, so this is deterministic
    zz = z.double()
    n = zz.numel()
    assert n == 6 * n_split
    mean, var = float(zz.mean()), float(zz.var(unbiased=True))
    first, second = zz[:n_split].reshape(-1), zz[n_split:].reshape(-1)       # a parent's two children: rows j and n_split + j
    corr = float(((first - first.mean()) * (second - second.mean())).mean() / (first.std(unbiased=False) * second.std(unbiased=False)))
    print(f"Philox deviates: n = {n}, mean {mean:+.4f}, var {var:.4f}, max |z| {float(zz.abs().max()):.3f}, sibling correlation {corr:+.4f}")
    assert abs(mean) <= 5 / np.sqrt(n) and abs(var - 1) <= 5 * np.sqrt(2 / n) and float(zz.abs().max()) <= 6.5
    assert abs(corr) <= 5 / np.sqrt(3 * n_split)


def test_edges_nothing_selected_short_noise_pending_grad(gpu_device):
    dev = gpu_device
    pc, f = _fixture_model(dev)
    args = (float(f["min_opacity"]), float(f["extent"]), None, 5, 5, None, 1000, "fine")
    # noise too short: RuntimeError BEFORE anything is mutated, compared tensor by tensor
    snap = _snapshot(pc)
    with pytest.raises(RuntimeError, match="noise"):
        pc.densify(float(f["max_grad"]), *args, noise=torch.zeros((10, 3), device=dev))
    for name, attr in ATTRS.items():
        p, old, m, v = snap[name]
        assert getattr(pc, attr) is p and torch.equal(p.detach(), old)
        st = pc.optimizer.state[p]
        assert torch.equal(st["exp_avg"], m) and torch.equal(st["exp_avg_sq"], v) and float(st["step"]) == STEP
    assert torch.equal(pc.xyz_gradient_accum, snap["accum"]) and torch.equal(pc.denom, snap["denom"])
    assert torch.equal(pc.max_radii2D, snap["radii"]) and torch.equal(pc._deformation_table, snap["table"])
    # nothing selected: the same Parameter objects remain and the counts say so
    out = pc.densify(1e9, *args)
    assert out == {"clone": 0, "split": 0, "P": int(f["P"])}
    for name, attr in ATTRS.items():
        assert getattr(pc, attr) is snap[name][0] and torch.equal(getattr(pc, attr).detach(), snap[name][1])
    out = pc.prune(float(f["max_grad"]), 0.0, float(f["extent"]), None)        # sigmoid(o) < 0 never holds
    assert out == {"drop": 0, "P": int(f["P"])} and pc._xyz is snap["xyz"][0]
    # a pending .grad is gone afterwards
    pc, f = _fixture_model(dev)
    old = pc._xyz
    for attr in ATTRS.values():
        getattr(pc, attr).grad = torch.ones_like(getattr(pc, attr))
    pc.densify(float(f["max_grad"]), *args, seed=5)
    assert old.grad is None and all(getattr(pc, attr).grad is None for attr in ATTRS.values())
    getattr(pc, "_opacity").grad = torch.ones_like(pc._opacity)
    old = pc._opacity
    pc.reset_opacity()
    assert old.grad is None and pc._opacity.grad is None


def test_edges_never_stepped_optimizer_and_everything_pruned(gpu_device):
    """A model whose optimizer has never stepped (no state yet: it stays without one), then the same surgery down to nothing followed
    by one training_step, as tests/test_cfg5_flow_gpu.py does with its stand-in helpers."""
    from s3gaussian_amd.pipeline import training_step
    from tests.test_cfg5_flow_gpu import _setup
    dev = gpu_device
    pc, cams, targets, hyper, opt, bg = _setup(dev, P=8000, W=160, H=112, seed=5)
    assert len(pc.optimizer.state) == 0
    P0 = pc._xyz.shape[0]
    pc.xyz_gradient_accum.fill_(1.0)
    pc.denom.fill_(1.0)                                             # every mean gradient is 1: everything clones or splits
    out = pc.densify(0.5, 0.005, 5.0, None, 5, 5, None, 600, "fine", seed=1)
    assert out["clone"] + out["split"] == P0 and pc._xyz.shape[0] == P0 + out["clone"] + out["split"]
    assert len(pc.optimizer.state) == 0                             # no state yet: stays without one
    pc.reset_opacity()
    assert len(pc.optimizer.state) == 0
    loss, pkg = training_step(pc, cams[0], *targets[0], hyper, opt, bg, stage="fine", densify_stats=True)
    assert torch.isfinite(loss) and pkg["radii"].numel() == pc._xyz.shape[0]
    assert float(pc.optimizer.state[pc._xyz]["step"]) == 1.0 and pc.optimizer.state[pc._xyz]["exp_avg"].shape == pc._xyz.shape
    out = pc.prune(0.0002, 2.0, 5.0, None)                          # sigmoid(o) < 2 always holds: everything goes
    assert out["P"] == 0 and pc._xyz.shape == (0, 3) and pc._features_rest.shape == (0, 15, 3) and pc.denom.shape == (0, 1)
    assert pc.optimizer.state[pc._xyz]["exp_avg"].shape == (0, 3) and float(pc.optimizer.state[pc._xyz]["step"]) == 1.0
    loss, pkg = training_step(pc, cams[0], *targets[0], hyper, opt, bg, stage="fine", densify_stats=True)
    assert torch.isfinite(loss) and pkg["radii"].numel() == 0 and not pkg["densify_stats_fused"]
    assert float(pkg["render"].detach().abs().max()) == 0.0
    assert pc.densify(0.0002, 0.005, 5.0, None, 5, 5, None, 700, "fine") == {"clone": 0, "split": 0, "P": 0}


# ---- in the loop -------------------------------------------------------------------------------------------------------------------
ITERS = 40


def _loop(dev, mode, events, dopt, extent):
    """ITERS iterations on the 60 k-point scene; mode "sync": a plain loop on the synchronous rasterizer forward, "replay": through
    run_training_steps on the host-asynchronous one.  events: density_control after every iteration's statistics."""
    from s3gaussian_amd import raster_C
    from s3gaussian_amd.density import density_control
    from s3gaussian_amd.hexplane import sort_state_words
    from s3gaussian_amd.pipeline import run_training_steps, training_step
    from tests.test_cfg5_flow_gpu import _setup
    prev_async = raster_C.set_async(mode == "replay")
    raster_C._async_states.pop(dev.index or 0, None)
    raster_C.invalidate_geometry_cache()
    try:
        torch.manual_seed(11)                   # the Philox seeds of the split events are drawn from torch's CPU generator
        pc, cams, targets, hyper, opt, bg = _setup(dev)
        grid = pc._deformation.deformation_net.grid
        losses, sizes, checks = {}, {}, []

        def issue(i):
            v = i % len(cams)
            if checks and checks[-1][0] == i - 1 and checks[-1][2] and mode == "sync":        # first step after an event that changed P
                hits = raster_C._geom_cache_hits
            else:
                hits = None
            loss, _ = training_step(pc, cams[v], *targets[v], hyper, opt, bg, stage="fine", densify_stats=True)
            losses[i] = loss
            if hits is not None:
                assert raster_C._geom_cache_hits == hits                                         # the geometry cache missed
                assert grid._order_cache["sort_state"].numel() == sort_state_words(4) * pc._xyz.shape[0]   # re-sorted at the new P
                assert grid._order_cache["sort_age"] == 0
            if events:
                before = pc._xyz.shape[0]
                out = density_control(pc, i, dopt, "fine", extent)
                if out["densify"] or out["prune"] or out["reset"]:
                    sizes[i] = pc._xyz.shape[0]
                    resized = bool((out["densify"] and out["densify"]["clone"] + out["densify"]["split"]) or (out["prune"] and out["prune"]["drop"]))
                    assert resized or pc._xyz.shape[0] == before
                    checks.append((i, out, resized))

        if mode == "sync":
            for i in range(1, ITERS + 1):
                issue(i)
        else:
            log = []
            res = run_training_steps(issue, 1, ITERS, optimizer=pc.optimizer, device=dev, log=log)
            assert log[-1] == ITERS and res["issued"] == len(log)
        torch.cuda.synchronize()
        assert pc.xyz_gradient_accum.shape == (pc._xyz.shape[0], 1) and pc.max_radii2D.shape == (pc._xyz.shape[0],)
        steps = sorted({float(s["step"]) for s in pc.optimizer.state.values() if "step" in s})
        assert steps == [float(ITERS)], steps                      # Adam `step` advanced by one per iteration, events or not
        lv = [float(losses[i]) for i in range(1, ITERS + 1)]
        assert all(np.isfinite(lv)), lv
        return dict(params={n: p.detach().clone() for n, p in pc.named_parameters()}, sizes=sizes, losses=lv,
                    events=[(i, o["densify"], o["prune"], o["reset"]) for i, o, _ in checks])
    finally:
        raster_C.set_async(prev_async)
        raster_C._async_states.pop(dev.index or 0, None)
        raster_C.invalidate_geometry_cache()


def _calibrate(dev):
    """Thresholds for the shortened schedule from the scene itself (setup, not a bound): the gradient threshold is the 0.85 quantile
    of the mean viewspace gradient after nine iterations and the extent puts percent_dense * extent at the median scale, so that both
    clone and split are exercised whatever the synthetic scene's units are."""
    from s3gaussian_amd.pipeline import training_step
    from tests.test_cfg5_flow_gpu import _setup
    pc, cams, targets, hyper, opt, bg = _setup(dev)
    for i in range(1, 10):
        v = i % len(cams)
        training_step(pc, cams[v], *targets[v], hyper, opt, bg, stage="fine", densify_stats=True)
    g = (pc.xyz_gradient_accum / pc.denom).nan_to_num(0.0).squeeze(1)
    th = float(torch.quantile(g[g > 0], 0.85))
    extent = float(torch.exp(pc._scaling.detach()).max(dim=1).values.median()) / 0.01
    return th, extent


def _distance(a, b):
    if a["params"].keys() != b["params"].keys() or any(a["params"][n].shape != b["params"][n].shape for n in a["params"]):
        return float("inf")
    return max(float((a["params"][n] - b["params"][n]).abs().max()) if a["params"][n].numel() else 0.0 for n in a["params"])


def test_density_control_in_the_training_loops(gpu_device):
    """40 iterations with densify + prune every 10 and one opacity reset (iteration 25; the size tests are on from then), in the
    deterministic HexPlane mode: once as a plain synchronous loop, once through run_training_steps.  Same P after every event and all
    parameters bit-identical at the end.  The yardstick for that bar is the same pair of loops WITHOUT density events: were that pair
    not bit-identical in this mode, the bar would be "no further apart than that pair" (the test prints both distances)."""
    from s3gaussian_amd import hexplane
    from s3gaussian_amd.density import default_density_opt
    dev = gpu_device
    prev = hexplane.set_deterministic(True)
    try:
        th, extent = _calibrate(dev)
        dopt = default_density_opt(densify_from_iter=5, pruning_from_iter=5, densification_interval=10, pruning_interval=10,
                                   opacity_reset_interval=25, densify_until_iter=1000, densify_grad_threshold_fine_init=th,
                                   densify_grad_threshold_after=th)
        base = [_loop(dev, m, False, dopt, extent) for m in ("sync", "replay")]
        runs = [_loop(dev, m, True, dopt, extent) for m in ("sync", "replay")]
    finally:
        hexplane.set_deterministic(prev)
    floor, got = _distance(*base), _distance(*runs)
    print(f"threshold {th:.3e}, extent {extent:.3f}; P after each event: {runs[0]['sizes']}; events {runs[0]['events']}")
    print(f"max |parameter difference| sync vs run_training_steps: without events {floor:.3e}, with events {got:.3e}")
    assert [e[0] for e in runs[0]["events"]] == [10, 20, 25, 30, 40]
    assert runs[0]["sizes"] == runs[1]["sizes"], (runs[0]["sizes"], runs[1]["sizes"])         # same P after every event
    assert len(set(runs[0]["sizes"].values()) | {60_000}) > 1                                 # and the events did change it
    assert any(e[1] and (e[1]["clone"] > 0 and e[1]["split"] > 0) for e in runs[0]["events"])
    if floor == 0.0:
        for n in runs[0]["params"]:
            assert torch.equal(runs[0]["params"][n], runs[1]["params"][n]), n                 # bit-identical
    else:
        assert got <= floor, (got, floor)


# ---- full size ---------------------------------------------------------------------------------------------------------------------
def _near(q, t, ulps=4):
    """rows whose fp32 quantity lies within `ulps` of the fp32 threshold"""
    t32 = torch.tensor(t, dtype=torch.float32, device=q.device)
    d = (q.contiguous().view(torch.int32).long() - t32.view(torch.int32).long()).abs()
    return (d <= ulps) & torch.isfinite(q)


def test_full_size_classes_and_gather(gpu_device):
    """P = 1.2 M, seeded decision inputs (uniform gradients, log-uniform scales, normal opacity logits) built on the CPU.  Classes and
    kept indices against the same masks evaluated by torch ops on the GPU; rows within 4 ulp of a threshold may be left out, at most
    1e-5 * P of them; then a gather spot-check on 1000 random rows per tensor."""
    from s3gaussian_amd import density
    from s3gaussian_amd.pipeline import GaussianParams, default_hyper, default_opt
    dev = gpu_device
    P = 1_200_000
    g = torch.Generator().manual_seed(2025)
    u = lambda *s: torch.rand(*s, generator=g)
    base = torch.exp(np.log(0.005) + u(P, 1) * (np.log(1.0) - np.log(0.005)))
    scaling = torch.log(base * torch.exp(0.25 * (u(P, 3) - 0.5)))
    denom = torch.floor(u(P, 1) * 12.0)
    accum = u(P, 1) * 0.00031 * denom
    radii = torch.floor(u(P) * 22.0)
    radii = torch.where(radii == 20.0, radii + 1.0, radii)
    pc = GaussianParams(3, default_hyper())
    pc.init_from_tensors((u(P, 3) - 0.5) * 40.0, scaling, torch.randn(P, 4, generator=g), -2.0 + 2.0 * torch.randn(P, 1, generator=g),
                         torch.randn(P, 16, 3, generator=g), dev)
    pc._deformation_table = (u(P) < 0.7).to(dev)
    pc.training_setup(default_opt())
    pc.xyz_gradient_accum, pc.denom, pc.max_radii2D = accum.to(dev), denom.to(dev), radii.to(dev)
    for attr in ATTRS.values():
        p = getattr(pc, attr)
        pc.optimizer.state[p] = {"step": torch.tensor(STEP), "exp_avg": torch.randn(p.shape, generator=g).to(dev),
                                 "exp_avg_sq": torch.rand(p.shape, generator=g).to(dev)}
    extent, th, min_op = 5.0, 0.0002, 0.005
    budget = int(1e-5 * P)

    # ---- densify: classes
    gq = (pc.xyz_gradient_accum / pc.denom).squeeze(1)
    gq[gq.isnan()] = 0.0
    ms = torch.exp(pc._scaling.detach()).max(dim=1).values
    sel, small = gq >= np.float32(th), ms <= np.float32(0.01 * extent)
    want = torch.where(sel & small, density.CLONE, torch.where(sel & ~small, density.SPLIT, density.KEEP)).to(torch.uint8)
    cls, counts = density.classify(pc, "densify", extent, max_grad=th, percent_dense=0.01)
    left_out = _near(gq, th) | _near(ms, 0.01 * extent)
    print(f"densify classes: {int(left_out.sum())} rows within 4 ulp of a threshold left out (at most {budget} allowed); counts {counts}")
    assert int(left_out.sum()) <= budget
    assert torch.equal(cls[~left_out], want[~left_out])
    assert counts["clone"] == int((cls == density.CLONE).sum()) and counts["split"] == int((cls == density.SPLIT).sum()) and counts["drop"] == 0
    assert 0.03 * P < counts["clone"] < 0.3 * P and 0.03 * P < counts["split"] < 0.3 * P
    # the order contract, from the kernel's own class bytes by torch ops
    idx = torch.arange(P, device=dev)
    split_rows = idx[cls == density.SPLIT]
    src = torch.cat([idx[cls != density.SPLIT], idx[cls == density.CLONE], split_rows, split_rows])
    n_keep = P - counts["split"]
    snap = _snapshot(pc)
    out = pc.densify(th, min_op, extent, None, 5, 5, None, 1000, "fine", seed=7)
    assert out == {"clone": counts["clone"], "split": counts["split"], "P": src.shape[0]} and pc._xyz.shape[0] == src.shape[0]
    pick = torch.from_numpy(np.random.default_rng(0).choice(src.shape[0], 1000, replace=False)).to(dev)
    pick = torch.cat([pick, torch.tensor([0, n_keep - 1, n_keep, n_keep + counts["clone"] - 1, n_keep + counts["clone"],
                                          src.shape[0] - 1], device=dev)])          # and the seams of the four runs
    is_child = pick >= n_keep + counts["clone"]
    for name, attr in ATTRS.items():
        new = getattr(pc, attr).detach()
        _, old, m, v = snap[name]
        rows = pick[~is_child] if name in ("xyz", "scaling") else pick
        assert torch.equal(new[rows], old[src[rows]]), name
        st = pc.optimizer.state[getattr(pc, attr)]
        surv = pick[pick < n_keep]
        assert torch.equal(st["exp_avg"][surv], m[src[surv]]) and torch.equal(st["exp_avg_sq"][surv], v[src[surv]]), name
        assert float(st["exp_avg"][pick[pick >= n_keep]].abs().max()) == 0 and float(st["exp_avg_sq"][pick[pick >= n_keep]].abs().max()) == 0
        assert float(st["exp_avg"][n_keep:].abs().max()) == 0                                     # (all of the new rows, cheaply)
    assert torch.equal(pc._deformation_table[pick], snap["table"][src[pick]])
    kids = pc._xyz.detach()[n_keep + counts["clone"]:]
    assert bool(torch.isfinite(kids).all()) and not torch.equal(kids[:counts["split"]], kids[counts["split"]:])

    # ---- prune with the size tests on, on the densified model (its radii were zeroed: put seeded ones back)
    P2 = pc._xyz.shape[0]
    pc.max_radii2D = torch.floor(torch.rand(P2, generator=g) * 22.0).to(dev)
    pc.max_radii2D[pc.max_radii2D == 20.0] = 21.0
    op = torch.sigmoid(pc._opacity.detach()).squeeze(1)
    ms = torch.exp(pc._scaling.detach()).max(dim=1).values
    drop = (op < np.float32(min_op)) | (pc.max_radii2D > 20.0) | (ms > np.float32(0.1 * extent))
    cls, counts = density.classify(pc, "prune", extent, min_opacity=min_op, max_screen_size=20)
    left_out = _near(op, min_op) | _near(ms, 0.1 * extent)
    print(f"prune classes: {int(left_out.sum())} rows within 4 ulp of a threshold left out (at most {int(1e-5 * P2)} allowed); counts {counts}")
    assert int(left_out.sum()) <= int(1e-5 * P2)
    assert torch.equal((cls == density.DROP)[~left_out], drop[~left_out]) and counts["drop"] == int((cls == density.DROP).sum())
    kept = torch.arange(P2, device=dev)[cls == density.KEEP]
    snap = _snapshot(pc)
    out = pc.prune(th, min_op, extent, 20)
    assert out == {"drop": counts["drop"], "P": kept.shape[0]} and 0.03 * P2 < counts["drop"] < 0.5 * P2
    pick = torch.from_numpy(np.random.default_rng(1).choice(kept.shape[0], 1000, replace=False)).to(dev)
    pick = torch.cat([pick, torch.tensor([0, kept.shape[0] - 1], device=dev)])
    for name, attr in ATTRS.items():
        _, old, m, v = snap[name]
        assert torch.equal(getattr(pc, attr).detach()[pick], old[kept[pick]]), name
        st = pc.optimizer.state[getattr(pc, attr)]
        assert torch.equal(st["exp_avg"][pick], m[kept[pick]]) and torch.equal(st["exp_avg_sq"][pick], v[kept[pick]]), name
    assert torch.equal(pc.max_radii2D, snap["radii"][kept]) and torch.equal(pc._deformation_table, snap["table"][kept])
