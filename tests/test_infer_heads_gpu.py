"""One-kernel deformation inference for the head sets beyond dx + dshs (mlp.deform_infer_heads, include/s3g_mlp.h::s3g_deform_infer_heads)
against the route it replaces under torch.no_grad(): HexPlane sampler -> deform_mlp(need_feat=False) -> geometry_heads.  Both are the
same fma chains in the same order, so every output must be BIT-IDENTICAL -- no tolerance appears below -- and through pipeline.render(),
evaluate_video() and save_split_point_clouds() nothing may change.  (The replaced route itself is checked against the reference
restatement in test_static_route_gpu.py, test_geometry_route_gpu.py and test_head_subsets_route_gpu.py.)"""
import itertools
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL = dict(grid_dimensions=2, input_coordinate_dim=4, output_coordinate_dim=32, resolution=[8, 8, 8, 5])
PIPE = dict(convert_SHs_python=True, compute_cov3D_python=False, debug=False)
NAMES = ("dx", "dshs", "ds", "dr", "do")          # the order of deform_infer_heads' result
EVERY_P = [frozenset(s) for s in (["dshs"], ["dx"], ["dx", "ds", "dr"], ["ds", "dr", "do"], ["dshs", "dr"], ["do"])]
SERVED = ([frozenset(c) for n in (1, 2, 3) for c in itertools.combinations(("dx", "ds", "dr", "do"), n)]
          + [frozenset(["dshs"])] + [frozenset(["dshs", g]) for g in ("ds", "dr", "do")])


@pytest.fixture(autouse=True)
def exact_chain():
    """The new kernel is the exact fp32 chain.  Without the SH head so is the route it replaces, in every arithmetic mode; with it that
    route follows mlp.set_mlp_arithmetic (default "bf16x3"), and the bit-identity below -- like `Deformation._infer_heads_ok` -- is a
    statement about the "f32" mode (tests/test_infer_gpu.py::exact_chain)."""
    from s3gaussian_amd import mlp
    mlp.set_mlp_arithmetic("f32")
    yield
    mlp.set_mlp_arithmetic(mlp.DEFAULT_ARITHMETIC)


@pytest.fixture(scope="module")
def net(gpu_device):
    """Four levels x 32 channels at resolution [8, 8, 8, 5]; all five head modules, planes and head weights perturbed."""
    from s3gaussian_amd.deformation import deform_network
    from s3gaussian_amd.pipeline import default_hyper
    torch.manual_seed(0)
    n = deform_network(default_hyper(kplanes_config=SMALL, no_ds=False, no_dr=False, no_do=False))
    n.deformation_net.set_aabb([40.0, 12.0, 6.0], [-40.0, -12.0, -6.0])
    d = n.deformation_net
    assert len(d.grid.resolutions) == 4
    with torch.no_grad():
        for p in d.grid.grids.parameters():
            p.add_(0.2 * torch.randn_like(p))
        for m in d.modules():
            if isinstance(m, torch.nn.Linear):
                torch.nn.init.normal_(m.bias, std=0.1)
        for head in (d.pos_deform, d.scales_deform, d.rotations_deform, d.opacity_deform, d.shs_deform):
            head[3].weight.copy_(0.3 * torch.randn_like(head[3].weight))
    return n.to(gpu_device).deformation_net


def _inputs(dev, P, tmode, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + P)
    xyz = ((torch.rand(P, 3, generator=g) - 0.5) * torch.tensor([100.0, 30.0, 15.0])).to(dev)     # a fifth of them outside the aabb
    time = (torch.rand(P, 1, generator=g) * 1.2 - 0.1).to(dev) if tmode == "per_point" else torch.full((P, 1), 0.41, device=dev)
    return xyz, time, tmode == "uniform"


def _modules(d, s):
    return (d.pos_deform if "dx" in s else None, d.shs_deform if "dshs" in s else None,
            (d.scales_deform if "ds" in s else None, d.rotations_deform if "dr" in s else None, d.opacity_deform if "do" in s else None))


def _today(d, feats, s):
    """The route the new call replaces, on the sampler's features: (dx, dshs, ds, dr, do) with None for absent heads."""
    from s3gaussian_amd.mlp import deform_mlp
    from s3gaussian_amd.mlp_geom import geometry_heads
    dx, dshs, feat = deform_mlp(feats, d.feature_out, d.pos_deform, d.shs_deform, d.dino_head, need_feat=False, need_dx="dx" in s,
                                need_dshs="dshs" in s)
    assert feat is None
    geo = _modules(d, s)[2]
    ds, dr, do = geometry_heads(feats, d.feature_out, *geo) if any(m is not None for m in geo) else (None, None, None)
    return dx, dshs, ds, dr, do


def _new(d, xyz, time, ut, s):
    from s3gaussian_amd.mlp import deform_infer_heads
    pos, shs, geo = _modules(d, s)
    return deform_infer_heads(d.grid, xyz, time, d.feature_out, pos, shs, geo, uniform_time=ut)


def _assert_equal(got, want, s, what):
    for name, a, b in zip(NAMES, got, want):
        assert (a is None) == (b is None) == (name not in s), (what, sorted(s), name)
        if a is not None:
            assert a.shape == b.shape and torch.equal(a, b), (what, sorted(s), name, int((a != b).any(-1).sum()))


def _fill_order_cache(d, xyz, time, ut):
    """The blocked processing order a backward leaves behind (tests/test_infer_gpu.py)."""
    with torch.enable_grad():
        x = xyz.clone().requires_grad_(True)
        d.grid(x, time, uniform_time=ut).sum().backward()
    for p in d.grid.grids.parameters():
        p.grad = None


def _check_sets(d, dev, P, tmode, sets, need_order):
    xyz, time, ut = _inputs(dev, P, tmode)
    d.grid._order_cache.clear()
    with torch.no_grad():
        feats = d.grid(xyz, time, uniform_time=ut)
        want = {s: _today(d, feats, s) for s in sets}
        for s in sets:
            assert d.grid._order_cache.get("order") is None
            got = _new(d, xyz, time, ut, s)
            _assert_equal(got, want[s], s, (P, tmode, "no cached order"))
        _fill_order_cache(d, xyz, time, ut)
        if need_order:
            assert d.grid._order_cache.get("order") is not None
        for s in sets:
            _assert_equal(_new(d, xyz, time, ut, s), want[s], s, (P, tmode, "cached order"))
    d.grid._order_cache.clear()


@pytest.mark.parametrize("tmode", ["uniform", "per_point"])
@pytest.mark.parametrize("P", [1, 31, 32, 33, 255, 257, 5000])
def test_operator_is_bit_identical_at_the_tile_and_workgroup_edges(gpu_device, net, P, tmode):
    _check_sets(net, gpu_device, P, tmode, EVERY_P, need_order=P >= 5000)


@pytest.mark.parametrize("tmode", ["uniform", "per_point"])
def test_operator_is_bit_identical_in_the_grid_stride_loop(gpu_device, net, tmode):
    """70 001 points: more than 256 workgroups x 8 waves x 32 points = 65 536, the smallest round size with a second sweep."""
    _check_sets(net, gpu_device, 70_001, tmode, [frozenset(["dx", "ds", "dr"]), frozenset(["dshs", "dr"])], need_order=True)


@pytest.mark.parametrize("tmode", ["uniform", "per_point"])
def test_all_eighteen_served_sets_at_257_points(gpu_device, net, tmode):
    from s3gaussian_amd import mlp
    assert len(set(SERVED)) == 18 and all(mlp.infer_heads_served("dx" in s, "dshs" in s, "ds" in s, "dr" in s, "do" in s) for s in SERVED)
    _check_sets(net, gpu_device, 257, tmode, SERVED, need_order=False)


def test_three_launches_of_one_call_are_equal(gpu_device, net):
    xyz, time, ut = _inputs(gpu_device, 5000, "uniform", seed=1)
    for s in (frozenset(["dx", "ds", "dr"]), frozenset(["dshs", "do"])):
        with torch.no_grad():
            runs = [_new(net, xyz, time, ut, s) for _ in range(3)]
        _assert_equal(runs[1], runs[0], s, "second launch")
        _assert_equal(runs[2], runs[0], s, "third launch")


@pytest.mark.parametrize("tmode", ["uniform", "per_point"])
def test_a_head_does_not_depend_on_which_others_are_present(gpu_device, net, tmode):
    xyz, time, ut = _inputs(gpu_device, 5000, tmode, seed=2)
    with torch.no_grad():
        only_dx = _new(net, xyz, time, ut, frozenset(["dx"]))
        dx_ds_dr = _new(net, xyz, time, ut, frozenset(["dx", "ds", "dr"]))
        ds_dr_do = _new(net, xyz, time, ut, frozenset(["ds", "dr", "do"]))
    assert torch.equal(only_dx[0], dx_ds_dr[0])
    assert torch.equal(ds_dr_do[2], dx_ds_dr[2]) and torch.equal(ds_dr_do[3], dx_ds_dr[3])
    assert float(dx_ds_dr[0].abs().max()) > 1e-3 and float(dx_ds_dr[2].abs().max()) > 1e-3 and float(ds_dr_do[4].abs().max()) > 1e-3


def test_an_unserved_set_is_an_error_in_c_and_todays_route_in_deform_heads(gpu_device, net, monkeypatch):
    import s3gaussian_amd.deformation as dm
    xyz, time, ut = _inputs(gpu_device, 257, "uniform", seed=3)
    every = frozenset(NAMES)
    with torch.no_grad(), pytest.raises(Exception, match=r"s3g_deform_infer_heads: the head set dx \+ ds \+ dr \+ do \+ dshs is not served"):
        _new(net, xyz, time, ut, every)
    with torch.no_grad(), pytest.raises(Exception, match=r"the head set dx \+ dshs is not served"):
        _new(net, xyz, time, ut, frozenset(["dx", "dshs"]))
    # the module with all five heads on: deform_heads goes the way it went, and returns what it returned
    assert net._fused_geometry_ok() and not net._infer_heads_ok()
    monkeypatch.setattr(dm, "deform_infer_heads", lambda *a, **k: pytest.fail("deform_infer_heads called for a set it does not serve"))
    monkeypatch.setattr(dm, "INFER_CACHE", False)
    with torch.no_grad():
        a = net.deform_heads(xyz, time, uniform_time=ut, need_feat=False, with_geometry=True)
        monkeypatch.setattr(dm, "FUSED_INFERENCE", False)
        b = net.deform_heads(xyz, time, uniform_time=ut, need_feat=False, with_geometry=True)
        want = _today(net, net.grid(xyz, time, uniform_time=ut), every)
    for x, y in zip(a[:2] + a[3], b[:2] + b[3]):
        assert torch.equal(x, y)
    assert torch.equal(a[0], want[0]) and torch.equal(a[1].reshape(-1, 48), want[1]) and all(torch.equal(x, y) for x, y in zip(a[3], want[2:]))


# ---- through the pipeline ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene():
    from s3gaussian_amd import synth
    return synth.street_scene(P=5000, width=160, height=112, n_frames=2)


def _model(scn, dev, **over):
    from s3gaussian_amd.pipeline import GaussianParams, default_hyper
    torch.manual_seed(0)
    pc = GaussianParams(3, default_hyper(**over))
    gs = scn["gaussians"]
    pc.init_from_tensors(gs["xyz"], gs["log_scales"], gs["rotations_raw"], gs["opacity_logit"], gs["shs"], dev)
    d = pc._deformation.deformation_net
    d.set_aabb(*scn["aabb"])
    with torch.no_grad():
        for p in d.grid.grids.parameters():
            p.add_(0.2 * torch.randn_like(p))
        for head, std in ((d.pos_deform, 0.05), (d.shs_deform, 0.02), (d.scales_deform, 0.02), (d.rotations_deform, 0.02), (d.opacity_deform, 0.02)):
            for p in head.parameters():
                p.add_(std * torch.randn_like(p))
    return pc


def _cam(scn, i, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in scn["cameras"][i].items()}


NETWORKS = {
    "static": (dict(no_dx=True), True),
    "no_dshs": (dict(no_dshs=True), True),
    "4dgs_default": (dict(no_dshs=True, feat_head=False, no_ds=False, no_dr=False), True),
    # dx + dshs + dr: three first layers beside S2 -- 125 440 B of weights, more than the 108 544 B the staging tiles leave.  Not one of
    # the served sets: its renders keep the three separate kernels, and must not change either
    "default_and_dr": (dict(no_dr=False), False),
}


@pytest.mark.parametrize("name", list(NETWORKS))
def test_render_takes_the_one_kernel_route_and_is_unchanged(gpu_device, scene, name, monkeypatch):
    import s3gaussian_amd.deformation as dm
    from s3gaussian_amd import raster_C
    from s3gaussian_amd.pipeline import render
    dev = gpu_device
    over, served = NETWORKS[name]
    pc = _model(scene, dev, **over)
    d = pc._deformation.deformation_net
    assert d._infer_heads_ok() == served
    cams = [_cam(scene, i, dev) for i in range(2)]
    assert cams[0]["time"] == cams[1]["time"]
    pipe, bg = SimpleNamespace(**PIPE), scene["bg"].to(dev)
    calls, samples = [], []
    real, real_grid = dm.deform_infer_heads, d.grid.forward
    monkeypatch.setattr(dm, "deform_infer_heads", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setattr(d.grid, "forward", lambda *a, **k: (samples.append(1), real_grid(*a, **k))[1])
    assert dm.FUSED_INFERENCE and dm.INFER_CACHE
    raster_C.invalidate_geometry_cache()
    hits = dm.infer_cache_hits
    with torch.no_grad():
        a = [render(c, pc, pipe, bg, stage="fine", return_dx=True) for c in cams]
    assert dm.infer_cache_hits == hits + 1                      # the second camera of the timestamp shares the evaluation
    if served:
        assert len(calls) == 1 and not samples                  # one launch for the two cameras; no [P,128] array was ever made
    else:
        assert not calls and len(samples) == 1
    monkeypatch.setattr(dm, "FUSED_INFERENCE", False)
    with torch.no_grad():
        b = [render(c, pc, pipe, bg, stage="fine", return_dx=True) for c in cams]
    assert len(calls) == (1 if served else 0) and len(samples) == (1 if served else 2)      # (the key tells the two routes apart)
    for x, y in zip(a, b):
        for k in ("render", "depth", "radii", "dx", "dshs"):
            assert (x.get(k) is None) == (y.get(k) is None), k
            if x.get(k) is not None:
                assert torch.equal(x[k], y[k]), k
    assert not torch.equal(a[0]["render"], a[1]["render"])
    # with autograd on (training), or with the feature image asked for, the one-kernel route is not taken
    monkeypatch.setattr(dm, "FUSED_INFERENCE", True)
    n = len(calls)
    render(cams[0], pc, pipe, bg, stage="fine")
    if hasattr(d, "dino_head"):
        with torch.no_grad():
            assert render(cams[0], pc, pipe, bg, stage="fine", render_feat=True)["feat"] is not None
    assert len(calls) == n


def test_evaluate_video_and_the_split_export_are_unchanged(gpu_device, scene, monkeypatch, tmp_path):
    """4D-Gaussian-Splatting's default network (dx + ds + dr): the strips of evaluate_video and the files of save_split_point_clouds
    with the one-kernel route on and off."""
    import s3gaussian_amd.deformation as dm
    from s3gaussian_amd import raster_C
    from s3gaussian_amd.pipeline import evaluate_video, save_split_point_clouds
    dev = gpu_device
    pc = _model(scene, dev, **NETWORKS["4dgs_default"][0])
    cams = [_cam(scene, i, dev) for i in range(len(scene["cameras"]))]
    g = torch.Generator().manual_seed(5)
    gts = [torch.rand(3, 112, 160, generator=g).to(dev) for _ in cams]
    pipe, bg = SimpleNamespace(**PIPE), scene["bg"].to(dev)
    calls = []
    real = dm.deform_infer_heads
    monkeypatch.setattr(dm, "deform_infer_heads", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    res, files = {}, {}
    for on in (True, False):
        monkeypatch.setattr(dm, "FUSED_INFERENCE", on)
        raster_C.invalidate_geometry_cache()
        n = len(calls)
        res[on] = evaluate_video(pc, cams, gts, pipe, bg, num_cams=3, keys=("rgbs", "depths"))
        paths = str(tmp_path / f"dynamic_{on}.ply"), str(tmp_path / f"static_{on}.ply")
        info = save_split_point_clouds(pc, cams[0]["time"], *paths)
        assert info["n_dynamic"] + info["n_static"] == 5000
        files[on] = [open(p, "rb").read() for p in paths]
        assert (len(calls) - n >= 2) if on else (len(calls) == n)         # one evaluation per timestamp, at least
    assert res[True]["num_timestamps"] == res[False]["num_timestamps"] == 2
    for k in ("rgbs", "depths"):
        for x, y in zip(res[True]["frames"][k], res[False]["frames"][k]):
            assert torch.equal(x, y), k
    assert torch.equal(res[True]["per_frame"][:, :2], res[False]["per_frame"][:, :2])
    assert files[True] == files[False] and len(files[True][0]) > 0


def test_render_flows_is_unchanged(gpu_device, scene, monkeypatch):
    import s3gaussian_amd.deformation as dm
    from s3gaussian_amd import raster_C
    from s3gaussian_amd.pipeline import render_flows
    dev = gpu_device
    pc = _model(scene, dev, **NETWORKS["no_dshs"][0])
    cams = [_cam(scene, i, dev) for i in range(len(scene["cameras"]))]
    pipe, bg = SimpleNamespace(**PIPE), scene["bg"].to(dev)
    calls = []
    real = dm.deform_infer_heads
    monkeypatch.setattr(dm, "deform_infer_heads", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    out = {}
    for on in (True, False):
        monkeypatch.setattr(dm, "FUSED_INFERENCE", on)
        raster_C.invalidate_geometry_cache()
        n = len(calls)
        out[on] = render_flows(pc, cams, pipe, bg, num_cams=3)
        assert (len(calls) > n) == on
    assert set(out[True]) == set(out[False])

    def same(x, y):
        if torch.is_tensor(x):
            return torch.equal(x, y)
        if isinstance(x, (list, tuple)):
            return len(x) == len(y) and all(same(p, q) for p, q in zip(x, y))
        if isinstance(x, dict):
            return set(x) == set(y) and all(same(x[k], y[k]) for k in x)
        return x == y
    for k in out[True]:
        assert same(out[True][k], out[False][k]), k
