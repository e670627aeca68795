"""The accumulated-opacity image of the rasterizer and its gradient, against the float64 oracle.

Forward: alpha = 1 - final_T, held to the bar and the flipped-pixel allowance tests/test_raster_gpu.py applies to the colour image
(the opacity IS the colour image of unit colours on black).  Backward: losses sum(c color) + sum(d depth) + sum(g_A alpha)
[+ sum(c2 color2)], truth = oracle backward of the RGB + depth part plus oracle backward of the unit-colour render seeded with g_A
(linearity), bar = GRAD_TOL of test_raster_gpu.py -- or, where the route the parent commit offers for the same loss (a third
rasterizer call with unit colours on black through autograd) does not meet that bar against the same truth either, four times
that route's own error: the two routes round differently, neither is wrong.  profiles/alpha_errors.json records both errors."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from tests import alpha_ref as R
from tests.util import oracle_forward, rel_l2, settings_from

pytestmark = pytest.mark.gpu

COLOR_TOL = 1e-4       # tests/test_raster_gpu.py
GRAD_TOL = 1e-4
OUTLIER_FRAC = 5e-4
BGS = {"black": R.BLACK, "colour": R.COLOUR}
NAMES = ("means3D", "means2D", "opacities", "scales", "rotations", "colors_a", "colors_b")
ORACLE = dict(means3D="dL_dmeans3D", means2D="dL_dmeans2D", opacities="dL_dopacity", scales="dL_dscales",
              rotations="dL_drotations", colors_a="dL_dcolors")


RECORD = os.environ.get("S3G_ALPHA_RECORD")     # _record() appends JSON lines to the file this names (profiles/alpha_errors.json
                                                # is the reduced copy of a run); unset: nothing is written


def _record(row):
    if RECORD:
        os.makedirs(os.path.dirname(os.path.abspath(RECORD)), exist_ok=True)
        with open(RECORD, "a") as f:
            f.write(json.dumps(row) + "\n")


def _set_wave_bounds(on) -> bool:
    from s3gaussian_amd import _lib
    L = _lib.lib()
    L.s3g_raster_set_backward_wave_bounds.restype = ctypes.c_int
    L.s3g_raster_set_backward_wave_bounds.argtypes = [ctypes.c_int]
    return bool(L.s3g_raster_set_backward_wave_bounds(int(on)))


def _colors_b(P):
    return torch.rand(P, 3, generator=torch.Generator().manual_seed(41))


def _leaves(s, dev):
    t = lambda x: x.to(dev).clone().requires_grad_(True)
    L = dict(means3D=t(s["means3D"]), opacities=t(s["opacities"]), scales=t(s["scales"]), rotations=t(s["rotations"]),
             colors_a=t(s["colors_precomp"]), colors_b=t(_colors_b(s["means3D"].shape[0])))
    L["means2D"] = torch.zeros_like(L["means3D"], requires_grad=True)
    return L


def _render(s, dev, pair, route, densify_accum=None):
    """route: "alpha" (the new nodes), "existing" (no opacity image), "third" (the parent's way: one more render, unit colours on
    black).  -> (dict of outputs, leaves)"""
    from diff_gaussian_rasterization import GaussianRasterizer
    rs = settings_from(s, dev)
    rast = GaussianRasterizer(raster_settings=rs)
    L = _leaves(s, dev)
    geo = dict(means3D=L["means3D"], means2D=L["means2D"], opacities=L["opacities"], scales=L["scales"], rotations=L["rotations"])
    out = {}
    if pair:
        kw = dict(with_alpha=True) if route == "alpha" else {}
        res = rast.forward_pair(colors_a=L["colors_a"], colors_b=L["colors_b"], densify_accum=densify_accum, **geo, **kw)
        out.update(color=res[0], radii=res[1], depth=res[2], color2=res[3])
        if route == "alpha":
            out["alpha"] = res[4]
    elif route == "alpha":
        out["color"], out["radii"], out["depth"], out["alpha"] = rast.forward_alpha(colors_precomp=L["colors_a"], **geo)
    else:
        out["color"], out["radii"], out["depth"] = rast(colors_precomp=L["colors_a"], **geo)
    if route == "third":
        black = GaussianRasterizer(raster_settings=rs._replace(bg=torch.zeros(3, device=dev)))
        out["alpha"] = black(colors_precomp=torch.ones_like(L["colors_a"]), **geo)[0][0:1]
    return out, L


def _backprop(out, ups, dev, keep):
    c, d, gA, c2 = (u.to(dev) * keep.to(dev) for u in ups)
    loss = (out["color"] * c).sum() + (out["depth"] * d).sum()
    if "alpha" in out:
        loss = loss + (out["alpha"] * gA).sum()
    if "color2" in out:
        loss = loss + (out["color2"] * c2).sum()
    loss.backward()


def _ups(H, W, kind):
    c, d, gA = R.upstream(H, W)
    c2 = torch.randn(3, H, W, generator=torch.Generator().manual_seed(43))
    if kind == "zero":
        gA = torch.zeros_like(gA)
    elif kind == "alpha_only":
        c, d, c2 = torch.zeros_like(c), torch.zeros_like(d), torch.zeros_like(c2)
    return c, d, gA, c2


def _flipped(name, alpha_gpu):
    """[H,W] bool: pixels where the GPU's alpha tests fell the other way than the float64 oracle's."""
    return np.abs(alpha_gpu.detach().cpu().numpy()[0].astype(np.float64) - R.alpha64(name)) > COLOR_TOL


_truth_cache = {}


def _truth(name, bgname, pair, kind, keep):
    """Float64 gradients of the loss of _backprop with the upstream gradients masked by `keep`."""
    key = (name, bgname, pair, kind, keep.numpy().tobytes())
    if key in _truth_cache:
        return _truth_cache[key]
    f = R.forward64(name, BGS[bgname])
    H, W = f["_cfg"]["H"], f["_cfg"]["W"]
    c, d, gA, c2 = (u.double().numpy() * keep.numpy() for u in _ups(H, W, kind))
    o = R.oracle64()
    t = {k: v.copy() for k, v in o.backward(f, c, d).items()}
    a = R.alpha_backward64(name, gA)
    for k in t:
        if k != "dL_dcolors":          # the unit colours of the opacity render are not the scene's colours
            t[k] = t[k] + a[k]
    res = {n: t[k] for n, k in ORACLE.items()}
    if pair:
        s = R.SCENES[name](BGS[bgname])
        s["colors_precomp"] = _colors_b(s["means3D"].shape[0])
        f2 = oracle_forward(o, s)
        t2 = o.backward(f2, c2, np.zeros((1, H, W)))
        for n, k in ORACLE.items():
            if n != "colors_a":
                res[n] = res[n] + t2[k]
        res["colors_b"] = t2["dL_dcolors"]
    _truth_cache[key] = res
    return res


def _errors(L, truth):
    return {n: rel_l2(L[n].grad.cpu().numpy(), truth[n]) for n in truth}


# ---------------------------------------------------------------- forward ----------------------------------------------------------
@pytest.mark.parametrize("bgname", ["black", "colour"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_alpha_matches_the_float64_oracle(gpu_device, name, bgname):
    s = R.SCENES[name](BGS[bgname])
    out, _ = _render(s, gpu_device, False, "alpha")
    a = out["alpha"].detach()
    H, W = R.alpha64(name).shape
    assert a.shape == (1, H, W) and a.dtype == torch.float32
    assert float(a.min()) >= 0.0 and float(a.max()) <= 1.0
    bad = _flipped(name, a)
    assert bad.mean() <= OUTLIER_FRAC, f"{bad.sum()} of {bad.size} pixels outside tolerance"
    n64 = R.forward64(name)["state"]["n_contrib"].reshape(H, W)
    empty = (n64 == 0) & ~bad
    assert empty.any() and (a.detach().cpu().numpy()[0][empty] == 0.0).all()      # no contributor: exactly 0
    if name == "A":
        assert float(a[0, :16, :16].abs().max()) == 0.0                               # the tile with the empty list
    else:
        assert float(a.max()) > 0.999                                                 # pixels that stopped early


@pytest.mark.parametrize("name", ["A", "B"])
def test_alpha_is_reproducible_and_the_other_outputs_are_untouched(gpu_device, name):
    from s3gaussian_amd import raster_C
    s = R.SCENES[name]()
    ref, _ = _render(s, gpu_device, False, "existing")
    ref2, _ = _render(s, gpu_device, True, "existing")
    runs = []
    prev = raster_C.set_async(True)
    try:
        for asynchronous in (True, True, False):
            raster_C.set_async(asynchronous)
            for pair in (False, True):
                out, _ = _render(s, gpu_device, pair, "alpha")
                want = ref2 if pair else ref
                for k in want:
                    assert torch.equal(out[k], want[k]), (asynchronous, pair, k)
                runs.append(out["alpha"])
    finally:
        raster_C.set_async(prev)
    for a in runs[1:]:
        assert torch.equal(a, runs[0])


@pytest.mark.parametrize("name", ["A", "B"])
def test_background_difference_is_the_transmittance(gpu_device, name):
    dev = gpu_device
    b = torch.tensor(R.COLOUR)
    with_bg, _ = _render(R.SCENES[name](R.COLOUR), dev, False, "alpha")
    black, _ = _render(R.SCENES[name](R.BLACK), dev, False, "alpha")
    assert torch.equal(with_bg["alpha"], black["alpha"])
    diff = (with_bg["color"] - black["color"]).detach().cpu()
    want = (1.0 - black["alpha"].detach().cpu()) * b.view(3, 1, 1)
    assert float((diff - want).abs().max()) <= COLOR_TOL


def test_opacity_image_reads_any_forwards_arena(gpu_device):
    """sky.opacity_image on the image arena of the synchronous forward, of the two-image forward and after a reuse blend."""
    from diff_gaussian_rasterization import _C
    from s3gaussian_amd import sky
    dev = gpu_device
    s = R.scene_a()
    cam = s["cam"]
    H, W = cam["image_height"], cam["image_width"]
    want, _ = _render(s, dev, False, "alpha")
    e = torch.Tensor([])
    d = lambda k: s[k].to(dev)
    args = (s["bg"].to(dev), d("means3D"), d("colors_precomp"), d("opacities"), d("scales"), d("rotations"), 1.0, e,
            cam["viewmatrix"].to(dev), cam["projmatrix"].to(dev), cam["tanfovx"], cam["tanfovy"], H, W, e, 0, cam["campos"].to(dev),
            False, False)
    img = _C.rasterize_gaussians(*args)[6]
    assert torch.equal(sky.opacity_image(img, H, W), want["alpha"])
    img2 = _C.rasterize_gaussians(*args, colors2=_colors_b(300).to(dev))[6]
    assert torch.equal(sky.opacity_image(img2, H, W), want["alpha"])
    img3 = _C.rasterize_gaussians(*args[:2], torch.ones(300, 3, device=dev), *args[3:])[6]     # same geometry: the reuse blend
    assert torch.equal(sky.opacity_image(img3, H, W), want["alpha"])
    with pytest.raises(RuntimeError, match="GPU"):
        sky.opacity_image(torch.zeros(16, dtype=torch.uint8), 2, 2)
    with pytest.raises(RuntimeError, match="smaller"):
        sky.opacity_image(torch.zeros(16, dtype=torch.uint8, device=dev), 4, 4)


def test_no_gaussians_gives_zero_opacity(gpu_device):
    from diff_gaussian_rasterization import GaussianRasterizer
    dev = gpu_device
    rast = GaussianRasterizer(raster_settings=settings_from(R.scene_a(), dev))
    z = torch.zeros(0, 3, device=dev)
    kw = dict(means3D=z, means2D=z.clone(), opacities=torch.zeros(0, 1, device=dev), scales=z.clone(),
              rotations=torch.zeros(0, 4, device=dev))
    color, radii, depth, alpha = rast.forward_alpha(colors_precomp=z.clone(), **kw)
    assert alpha.shape == (1, 29, 37) and float(alpha.abs().max()) == 0.0 and float(color.abs().max()) == 0.0
    res = rast.forward_pair(colors_a=z.clone(), colors_b=z.clone(), with_alpha=True, **kw)
    assert len(res) == 5 and float(res[4].abs().max()) == 0.0


# ---------------------------------------------------------------- backward ---------------------------------------------------------
@pytest.mark.parametrize("pair", [False, True], ids=["NX0", "NX3"])
@pytest.mark.parametrize("bgname", ["black", "colour"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_gradients_against_float64_truth(gpu_device, name, bgname, pair):
    dev = gpu_device
    s = R.SCENES[name](BGS[bgname])
    H, W = R.alpha64(name).shape
    prev = _set_wave_bounds(True)
    try:
        for bounds in (True, False):
            _set_wave_bounds(bounds)
            for kind in ("random", "alpha_only"):
                ups = _ups(H, W, kind)
                out, L = _render(s, dev, pair, "alpha")
                keep = torch.from_numpy(~_flipped(name, out["alpha"])).float()
                _backprop(out, ups, dev, keep)
                truth = _truth(name, bgname, pair, kind, keep)
                got = _errors(L, truth)
                out3, L3 = _render(s, dev, pair, "third")
                _backprop(out3, ups, dev, keep)
                parent = _errors(L3, truth)
                print(f"alpha_errors scene={name} bg={bgname} pair={pair} wave_bounds={bounds} loss={kind} new={got} parent={parent}")
                _record(dict(scene=name, bg=bgname, NX=3 if pair else 0, wave_bounds=bounds, loss=kind, masked_pixels=int((keep == 0).sum()),
                             new=got, third_call=parent))
                for n in truth:
                    if kind == "alpha_only" and n.startswith("colors"):
                        assert float(L[n].grad.abs().max()) == 0.0, n          # the opacity does not depend on the colours
                        continue
                    assert got[n] <= max(GRAD_TOL, 4.0 * parent[n]), (bounds, kind, n, got[n], parent[n])
    finally:
        _set_wave_bounds(prev)


@pytest.mark.parametrize("pair", [False, True], ids=["NX0", "NX3"])
@pytest.mark.parametrize("name", ["A", "B"])
def test_zero_opacity_gradient_equals_the_existing_nodes(gpu_device, name, pair):
    dev = gpu_device
    s = R.SCENES[name]()
    H, W = R.alpha64(name).shape
    ups = _ups(H, W, "zero")
    keep = torch.ones(H, W)
    prev = _set_wave_bounds(True)
    try:
        for bounds in (True, False):
            _set_wave_bounds(bounds)
            out, L = _render(s, dev, pair, "alpha")
            _backprop(out, ups, dev, keep)                       # a zero TENSOR on alpha: the new entry point runs
            ref, Lr = _render(s, dev, pair, "existing")
            _backprop(ref, ups, dev, keep)
            out_n, Ln = _render(s, dev, pair, "alpha")
            out_n.pop("alpha")                                   # alpha unused: the existing entry points run (counted in
                                                                 # test_unused_alpha_takes_the_existing_entry_points)
            _backprop(out_n, ups, dev, keep)
            for n in NAMES:
                if n == "colors_b" and not pair:
                    continue
                assert torch.equal(L[n].grad, Lr[n].grad), (bounds, n)
                assert torch.equal(Ln[n].grad, Lr[n].grad), (bounds, n)
    finally:
        _set_wave_bounds(prev)


@pytest.mark.parametrize("pair", [False, True], ids=["NX0", "NX3"])
def test_unused_alpha_takes_the_existing_entry_points(gpu_device, monkeypatch, pair):
    """An alpha output that feeds no loss reaches the node's backward as None (the nodes do not materialise unused gradients): the
    existing entry points run and s3g_raster_backward_alpha is not called.  A zero TENSOR on alpha is a gradient: the new one runs."""
    from s3gaussian_amd import raster_C
    calls = {"alpha": 0, "old": 0}

    def counted(key, fn):
        def wrapper(*a, **k):
            calls[key] += 1
            return fn(*a, **k)
        return wrapper

    monkeypatch.setattr(raster_C, "rasterize_gaussians_backward_alpha", counted("alpha", raster_C.rasterize_gaussians_backward_alpha))
    old = "rasterize_gaussians_backward2" if pair else "rasterize_gaussians_backward"
    monkeypatch.setattr(raster_C, old, counted("old", getattr(raster_C, old)))
    dev = gpu_device
    s = R.scene_a()
    H, W = R.alpha64("A").shape
    keep = torch.ones(H, W)
    out, L = _render(s, dev, pair, "alpha")
    out.pop("alpha")
    _backprop(out, _ups(H, W, "random"), dev, keep)
    assert calls == {"alpha": 0, "old": 1}, calls
    out, L = _render(s, dev, pair, "alpha")
    (out["depth"] * 2.0).sum().backward()                    # colour unused as well: still the existing entry point
    assert calls == {"alpha": 0, "old": 2} and L["means3D"].grad is not None, calls
    out, L = _render(s, dev, pair, "alpha")
    _backprop(out, _ups(H, W, "zero"), dev, keep)
    assert calls == {"alpha": 1, "old": 2}, calls
    out, L = _render(s, dev, pair, "alpha")
    out["alpha"].sum().backward()                            # alpha alone
    assert calls == {"alpha": 2, "old": 2} and L["opacities"].grad is not None, calls


@pytest.mark.parametrize("name", ["A", "B"])
def test_pair_node_keeps_the_fused_densify_statistics(gpu_device, name):
    dev = gpu_device
    s = R.SCENES[name]()
    P = s["means3D"].shape[0]
    H, W = R.alpha64(name).shape
    keep = torch.ones(H, W)

    def acc():
        g = torch.Generator().manual_seed(3)
        return tuple(torch.rand(P, generator=g).to(dev) for _ in range(3))

    a0, a1 = acc(), acc()
    out, L = _render(s, dev, True, "alpha", densify_accum=a0)
    _backprop(out, _ups(H, W, "zero"), dev, keep)
    ref, Lr = _render(s, dev, True, "existing", densify_accum=a1)
    _backprop(ref, _ups(H, W, "zero"), dev, keep)
    for x, y in zip(a0, a1):
        assert torch.equal(x, y)
    # with an opacity gradient the statistics follow the gradient this node really produced
    a2, start = acc(), acc()
    out, L = _render(s, dev, True, "alpha", densify_accum=a2)
    _backprop(out, _ups(H, W, "random"), dev, keep)
    vis = out["radii"] > 0
    norm = L["means2D"].grad[:, :2].norm(dim=1)
    assert torch.allclose(a2[0], start[0] + torch.where(vis, norm, torch.zeros_like(norm)), rtol=1e-5, atol=1e-7)
    assert torch.equal(a2[1], start[1] + vis.float())
    assert torch.equal(a2[2], torch.where(vis, torch.maximum(start[2], out["radii"].float()), start[2]))
    assert not torch.equal(a2[0], a0[0])


@pytest.mark.parametrize("name", ["A", "B"])
def test_single_image_entry_with_accumulators_internals_and_sh(gpu_device, name):
    """The one-image shape of s3g_raster_backward_alpha through the binding: with the accumulators (s3g_raster_backward_accum's shape),
    the internal gradients (dL_dconic, dL_ddepths, dL_dcov3D) and SH colours (dL_dsh)."""
    from s3gaussian_amd import raster_C as _C
    dev = gpu_device
    s = R.SCENES[name]()
    cam = s["cam"]
    P = s["means3D"].shape[0]
    H, W = cam["image_height"], cam["image_width"]
    e = torch.Tensor([])
    d = lambda k: s[k].to(dev)
    c, dd, gA, _ = (u.to(dev) for u in _ups(H, W, "random"))
    view, proj, campos = cam["viewmatrix"].to(dev), cam["projmatrix"].to(dev), cam["campos"].to(dev)
    for mode in ("precomp", "sh"):
        col, sh, deg = (d("colors_precomp"), e, 0) if mode == "precomp" else (e, d("shs"), 3)
        R_, color, depth, radii, geom, binning, img = _C.rasterize_gaussians(
            s["bg"].to(dev), d("means3D"), col, d("opacities"), d("scales"), d("rotations"), 1.0, e, view, proj, cam["tanfovx"],
            cam["tanfovy"], H, W, sh, deg, campos, False, False)
        common = (s["bg"].to(dev), d("means3D"), radii, col)
        tail = (d("scales"), d("rotations"), 1.0, e, view, proj, cam["tanfovx"], cam["tanfovy"])
        g = torch.Generator().manual_seed(3)
        acc0 = tuple(torch.rand(P, generator=g).to(dev) for _ in range(3))
        acc1 = tuple(x.clone() for x in acc0)
        zero = torch.zeros_like(gA)
        new = _C.rasterize_gaussians_backward_alpha(*common, None, *tail, c, dd, None, zero, sh, deg, campos, geom, R_, binning, img,
                                                    False, densify_accum=acc0, return_internals=True)
        old = _C.rasterize_gaussians_backward(*common, *tail, c, dd, sh, deg, campos, geom, R_, binning, img, False,
                                              return_internals=True, densify_accum=acc1)
        new = [x for x in new if x is not None]
        assert len(new) == len(old) == 10
        for i, (x, y) in enumerate(zip(new, old)):
            assert torch.equal(x, y), (mode, i)
        for x, y in zip(acc0, acc1):
            assert torch.equal(x, y)
        if mode == "sh":
            continue
        # the internals and dL_dcov3D against float64 (flipped pixels masked out of all three upstream gradients, as elsewhere)
        keep = torch.from_numpy(~_flipped(name, _C.raster_alpha(img, H, W))).float().to(dev)
        start = tuple(torch.rand(P, generator=g).to(dev) for _ in range(3))
        acc2 = tuple(x.clone() for x in start)
        got = _C.rasterize_gaussians_backward_alpha(*common, None, *tail, c * keep, dd * keep, None, gA * keep, sh, deg, campos, geom,
                                                    R_, binning, img, False, densify_accum=acc2, return_internals=True)
        o = R.oracle64()
        f = R.forward64(name)
        k = keep.cpu().double().numpy()
        t = o.backward(f, c.cpu().double().numpy() * k, dd.cpu().double().numpy() * k)
        a = R.alpha_backward64(name, gA.cpu().double().numpy() * k)
        # NX = 0 WITH the accumulators and a non-zero g_A: every gradient against float64, the statistics against this call's own
        # dL_dmeans2D (as test_pair_node_keeps_the_fused_densify_statistics holds the two-image shape)
        for idx, key in ((0, "dL_dmeans2D"), (1, "dL_dcolors"), (3, "dL_dopacity"), (4, "dL_dmeans3D"), (7, "dL_dscales"),
                         (8, "dL_drotations")):
            want = t[key] + (a[key] if key != "dL_dcolors" else 0.0)
            err = rel_l2(got[idx].cpu().numpy(), want)
            print(f"alpha_errors scene={name} NX=0 with accumulators {key} new={err}")
            assert err <= GRAD_TOL, (key, err)
        vis = radii > 0
        norm = got[0][:, :2].norm(dim=1)
        assert torch.allclose(acc2[0], start[0] + torch.where(vis, norm, torch.zeros_like(norm)), rtol=1e-5, atol=1e-7)
        assert torch.equal(acc2[1], start[1] + vis.float())
        assert torch.equal(acc2[2], torch.where(vis, torch.maximum(start[2], radii.float()), start[2]))
        assert not torch.equal(acc2[0], acc0[0])                 # the opacity gradient moved the statistics
        for idx, key in ((5, "dL_dcov3D"), (9, "dL_dconic"), (10, "dL_ddepths")):
            want = t[key] + (a[key] if key != "dL_ddepths" else 0.0)
            err = rel_l2(got[idx].cpu().numpy(), want)
            print(f"alpha_errors scene={name} internal={key} new={err}")
            assert err <= GRAD_TOL, (key, err)


def test_the_two_nodes_with_and_without_the_opacity_output(gpu_device):
    """_RasterizeGaussians / _RasterizeGaussiansPair called directly: 3 / 4 outputs, one more with the trailing with_alpha=True; that
    output is raster_alpha of a plain forward bit for bit, and with it left unused every input gradient is the plain node's."""
    from s3gaussian_amd import raster_C as _C
    from s3gaussian_amd.rasterizer import _RasterizeGaussians, _RasterizeGaussiansPair
    dev = gpu_device
    s = R.scene_a()
    rs = settings_from(s, dev)
    H, W = rs.image_height, rs.image_width
    assert s["colors_precomp"].shape[1] == _C.NUM_CHANNELS
    c, d, _, c2 = (u.to(dev) for u in _ups(H, W, "random"))
    e = torch.Tensor([])

    def run(pair, *trailing):
        L = _leaves(s, dev)
        if pair:
            tensors = (L["means3D"], L["means2D"], L["colors_a"], L["colors_b"], L["opacities"], L["scales"], L["rotations"], e)
            out = _RasterizeGaussiansPair.apply(*tensors, rs, *trailing)
        else:
            tensors = (L["means3D"], L["means2D"], e, L["colors_a"], L["opacities"], L["scales"], L["rotations"], e)
            out = _RasterizeGaussians.apply(*tensors, rs, *trailing)
        loss = (out[0] * c).sum() + (out[2] * d).sum()
        if pair:
            loss = loss + (out[3] * c2).sum()
        loss.backward()                      # the opacity output, where there is one, feeds nothing
        return out, L

    img = _C.rasterize_gaussians(rs.bg, s["means3D"].to(dev), s["colors_precomp"].to(dev), s["opacities"].to(dev), s["scales"].to(dev),
                                 s["rotations"].to(dev), 1.0, e, rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, H, W, e, 0,
                                 rs.campos, False, False)[6]
    alpha = _C.raster_alpha(img, H, W)
    assert 0.01 < float(alpha.mean()) < 0.999
    for pair, n in ((False, 3), (True, 4)):
        plain, Lp = run(pair)
        assert len(plain) == n
        with_alpha, La = run(pair, *((None,) if pair else ()), False, True)      # (densify_accum,) forward_only, with_alpha
        assert len(with_alpha) == n + 1
        assert torch.equal(with_alpha[-1], alpha)
        for k in range(n):
            assert torch.equal(with_alpha[k], plain[k]), k
        for name in NAMES:
            if name == "colors_b" and not pair:
                continue
            assert Lp[name].grad is not None and torch.equal(La[name].grad, Lp[name].grad), (pair, name)
