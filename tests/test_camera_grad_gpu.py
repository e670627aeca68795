"""GPU: the camera-gradient kernel and the pose kernels against their float64 restatements (tests/pose_ref.py), and the camera
gradients through GaussianRasterizer against float64 autograd of oracle/torch_ref.

  * s3g_camera_backward against camera_terms_ref on the same fp32 inputs -- the library's own backward outputs and the forward's
    own cov3D / clamped, read out of the geometry arena.  Both sides form the same per-Gaussian terms in IEEE double and differ
    in the order of the sum over P only: the bar is 1e-12 x sum|term| per output ((P + a few hundred operations) x 1.1e-16 is
    1.5e-13 at P = 1000).  Two runs are bit-identical, the entries that enter no product are exactly 0.
  * through the single, alpha and pair nodes (the pair with fused densify statistics): the error relative to sum|term| per block
    is at most 4 x the relative error of the same call's means3D gradient against the same autograd (the bar of
    tests/test_camera_grad_cpu.py); every other .grad is bit-identical to the call without requires_grad on the camera.
  * after an overflowed asynchronous forward: zeros, no NaN.
  * s3g_pose_apply / _backward against pose_map_ref and its autograd Jacobian at 1e-12.
"""
import math
import warnings

import numpy as np
import pytest
import torch

from tests.pose_ref import BLOCKS, UNUSED, camera_terms_ref, pose_map_ref
from tests.test_camera_grad_cpu import POSE_CASES, block_errors, camera_scene, upstream
from tests.util import rel_l2, settings_from

pytestmark = pytest.mark.gpu

W, H = 40, 24
EMPTY = torch.Tensor([])


def _arena_arrays(geom, P):
    """cov3D [P,6] and clamped [P,3] of the forward that filled `geom` (GeomState::carve, csrc/raster_dev.hpp: depths, means2D,
    conic_opacity, cov3D, rgb, clamped, ... each 128-byte aligned)."""
    off = 0
    spans = {}
    for name, nbytes in (("depths", 4 * P), ("means2D", 8 * P), ("conic_opacity", 16 * P), ("cov3D", 24 * P), ("rgb", 12 * P),
                         ("clamped", 3 * P)):
        off = (off + 127) & ~127
        spans[name] = (off, off + nbytes)
        off += nbytes
    raw = geom.cpu().numpy()
    cov = raw[spans["cov3D"][0]:spans["cov3D"][1]].view(np.float32).reshape(P, 6)
    clamped = raw[spans["clamped"][0]:spans["clamped"][1]].reshape(P, 3)
    return cov, clamped


def _library_backward(s, mode, dev, gc, gd, colors2=None, gc2=None, galpha=None, cov_precomp=False):
    """One forward + backward through raster_C on the scene -> every array s3g_camera_backward and its restatement read."""
    from s3gaussian_amd import raster_C as _C
    cam = s["cam"]
    H, W = cam["image_height"], cam["image_width"]
    t = lambda k: s[k].to(dev).contiguous()
    m3, op, sc, rot = t("means3D"), t("opacities"), t("scales"), t("rotations")
    sh = t("shs") if mode == "sh" else EMPTY
    col = t("colors_precomp") if mode != "sh" else EMPTY
    cov = EMPTY
    if cov_precomp:
        from s3gaussian_amd.pipeline import covariance_from_scaling_rotation
        cov, sc, rot = covariance_from_scaling_rotation(sc, 1.0, rot).contiguous(), EMPTY, EMPTY
    view, proj, campos, bg = cam["viewmatrix"].to(dev), cam["projmatrix"].to(dev), cam["campos"].to(dev), s["bg"].to(dev)
    deg = 3 if mode == "sh" else 0
    _C.invalidate_geometry_cache()
    out = _C.rasterize_gaussians(bg, m3, col, op, sc, rot, 1.0, cov, view, proj, cam["tanfovx"], cam["tanfovy"], H, W, sh, deg, campos,
                                 False, False, colors2=colors2)
    R, color, depth, radii, geom, binning, img = out[:7]
    grads = _C.rasterize_gaussians_backward_alpha(
        bg, m3, radii, col, colors2, sc, rot, 1.0, cov, view, proj, cam["tanfovx"], cam["tanfovy"], gc.float().to(dev), gd.float().to(dev),
        None if gc2 is None else gc2.float().to(dev), torch.zeros(1, H, W, device=dev) if galpha is None else galpha.float().to(dev),
        sh, deg, campos, geom, R, binning, img, False, return_internals=True)
    g_m2, g_col, _, _, g_m3, *_rest, g_conic, g_dep = grads
    P = m3.shape[0]
    cov3D, clamped = _arena_arrays(geom, P)
    if cov_precomp:
        cov3D = cov.cpu().numpy()
    return dict(P=P, m3=m3, radii=radii, geom=geom, view=view, proj=proj, campos=campos, sh=sh if mode == "sh" else None, deg=deg,
                cov=cov if cov_precomp else None, g_m2=g_m2, g_col=g_col, g_conic=g_conic, g_dep=g_dep, g_m3=g_m3,
                cov3D=cov3D, clamped=clamped, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], H=H, W=W)


def _kernel(b, dev, pieces=("m2", "conic", "dep", "col"), g_dir=None):
    from s3gaussian_amd import raster_C as _C
    pick = lambda name, t_: t_ if name in pieces else None
    return _C.camera_backward(b["P"], dev, means3D=b["m3"], radii=b["radii"], geomBuffer=b["geom"], viewmatrix=b["view"],
                              projmatrix=b["proj"], campos=b["campos"], tan_fovx=b["tanfovx"], tan_fovy=b["tanfovy"], image_height=b["H"],
                              image_width=b["W"], dL_dmeans2D=pick("m2", b["g_m2"]), dL_dconic=pick("conic", b["g_conic"]),
                              dL_ddepths=pick("dep", b["g_dep"]), dL_dcolors=pick("col", b["g_col"]), sh=b["sh"], degree=b["deg"],
                              cov3D_precomp=b["cov"], g_dir=g_dir)


def _restatement(b, pieces=("m2", "conic", "dep", "col"), g_dir=None):
    n = lambda t_: t_.cpu().numpy()
    pick = lambda name, t_: n(t_) if name in pieces else None
    return camera_terms_ref(P=b["P"], means3D=n(b["m3"]), radii=n(b["radii"]), cov3D=b["cov3D"], clamped=b["clamped"],
                            viewmatrix=n(b["view"]), projmatrix=n(b["proj"]), campos=n(b["campos"]), tanfovx=b["tanfovx"],
                            tanfovy=b["tanfovy"], image_height=b["H"], image_width=b["W"], dL_dmeans2D=pick("m2", b["g_m2"]),
                            dL_dconic=pick("conic", b["g_conic"]), dL_ddepths=pick("dep", b["g_dep"]), dL_dcolors=pick("col", b["g_col"]),
                            shs=None if b["sh"] is None else n(b["sh"]), sh_degree=b["deg"], g_dir=None if g_dir is None else n(g_dir))


def _assert_matches(got, sums, abs_sums, what):
    got = got.cpu().numpy()
    assert np.isfinite(got).all(), what
    excess = np.abs(got - sums) - 1e-12 * abs_sums
    print(what, "max |kernel - restatement| / sum|term| =", float((np.abs(got - sums) / np.maximum(abs_sums, 1e-300)).max()))
    assert (excess <= 0).all(), (what, got, sums, abs_sums)
    for j in UNUSED:
        assert got[j] == 0.0, (what, j)


@pytest.mark.parametrize("mode", ["sh", "precomp"])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_kernel_matches_the_restatement(gpu_device, P, mode):
    dev = gpu_device
    s = camera_scene(P, P=P, W=W, H=H) if P > 1 else camera_scene(2, P=1, W=W, H=H, spread=0.3, zmin=3.0, zmax=4.0)
    gc, gd = upstream(P, H, W)
    b = _library_backward(s, mode, dev, gc, gd, cov_precomp=(P == 257))
    assert int((b["radii"] > 0).sum()) >= (1 if P == 1 else P // 8)
    g_dir = torch.randn(P, 3, generator=torch.Generator().manual_seed(P)).to(dev)
    full = ("m2", "conic", "dep", "col")
    variants = [(full, None), (full, g_dir), ((), g_dir)] + [(tuple(p for p in full if p != drop), None) for drop in full]
    for pieces, gd_ in variants:
        got = _kernel(b, dev, pieces, gd_)
        again = _kernel(b, dev, pieces, gd_)
        assert torch.equal(got, again), (pieces, "two runs differ")
        sums, abs_sums = _restatement(b, pieces, gd_)
        _assert_matches(got, sums, abs_sums, (P, mode, pieces, gd_ is not None))
    # the pieces are there to be dropped: each one moves the result of this scene
    sums, _ = _restatement(b)
    assert np.abs(sums[BLOCKS["view"]]).max() > 0 and np.abs(sums[BLOCKS["proj"]]).max() > 0
    assert (np.abs(sums[BLOCKS["campos"]]).max() > 0) == (mode == "sh")


def test_all_culled_scene_and_no_gaussians_give_exact_zeros(gpu_device):
    from s3gaussian_amd import raster_C as _C
    dev = gpu_device
    s = camera_scene(4, P=200, W=W, H=H, zmin=-6.0, zmax=-1.0)         # everything behind the camera
    gc, gd = upstream(4, H, W)
    b = _library_backward(s, "sh", dev, gc, gd)
    assert int((b["radii"] > 0).sum()) == 0
    got = _kernel(b, dev)
    assert torch.equal(got, torch.zeros(35, dtype=torch.float64, device=dev))
    g_dir = torch.randn(200, 3, generator=torch.Generator().manual_seed(0)).to(dev)
    got = _kernel(b, dev, g_dir=g_dir)          # g_dir counts every Gaussian, whatever its radius
    sums, abs_sums = _restatement(b, g_dir=g_dir)
    _assert_matches(got, sums, abs_sums, "culled + g_dir")
    assert float(got[32:].abs().max()) > 0 and not got[:32].any()
    out = _C.camera_backward(0, dev, g_dir=torch.empty(0, 3, device=dev))      # P == 0: zeros without a launch
    assert out.shape == (35,) and out.dtype == torch.float64 and not out.any()


# ---- through the autograd nodes ---------------------------------------------------------------------------------------------------
def _truth(s, kind, mode, gc, gd, gc2, ga):
    """float64 autograd of torch_ref for the node's loss: <color, gc> + <depth, gd> [+ <color2, gc2>] [+ <alpha, ga>]."""
    from oracle import torch_ref
    d = lambda t_: t_.detach().to(torch.float64)
    cam = s["cam"]
    view, proj, campos, m3 = (d(cam["viewmatrix"]).requires_grad_(True), d(cam["projmatrix"]).requires_grad_(True),
                              d(cam["campos"]).requires_grad_(True), d(s["means3D"]).requires_grad_(True))
    kw = dict(bg=d(s["bg"]), means3D=m3, opacities=d(s["opacities"]), viewmatrix=view, projmatrix=proj, campos=campos,
              tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], image_height=H, image_width=W, scales=d(s["scales"]), rotations=d(s["rotations"]))
    colour = dict(shs=d(s["shs"]), sh_degree=3) if mode == "sh" else dict(colors_precomp=d(s["colors_precomp"]))
    color, _, depth = torch_ref.rasterize(**kw, **colour)
    loss = (color * gc).sum() + (depth * gd).sum()
    if kind.startswith("pair"):
        color2, _, _ = torch_ref.rasterize(**kw, colors_precomp=d(s["colors_precomp"]).flip(0))
        loss = loss + (color2 * gc2).sum()
    if ga is not None:      # accumulated opacity = what unit colours on a black background render
        ones, _, _ = torch_ref.rasterize(**{**kw, "bg": torch.zeros(3, dtype=torch.float64)}, colors_precomp=torch.ones_like(d(s["means3D"])))
        loss = loss + (ones[0:1] * ga).sum()
    gv, gp, gcam, gm = torch.autograd.grad(loss, (view, proj, campos, m3), allow_unused=True)
    z = lambda g, like: torch.zeros_like(like) if g is None else g
    return torch.cat([z(gv, view).reshape(-1), z(gp, proj).reshape(-1), z(gcam, campos).reshape(-1)]).numpy(), gm.numpy()


def _through_node(s, kind, mode, dev, gc, gd, gc2, ga, camera_grad, acc=None):
    from diff_gaussian_rasterization import GaussianRasterizer
    from s3gaussian_amd import raster_C
    rs = settings_from(s, dev, sh_degree=3 if mode == "sh" else 0)
    if camera_grad:
        rs = rs._replace(viewmatrix=rs.viewmatrix.clone().requires_grad_(True), projmatrix=rs.projmatrix.clone().requires_grad_(True),
                         campos=rs.campos.clone().requires_grad_(True))
    rast = GaussianRasterizer(raster_settings=rs)
    leaf = lambda k: s[k].to(dev).clone().requires_grad_(True)
    m3, op, sc, rot = leaf("means3D"), leaf("opacities"), leaf("scales"), leaf("rotations")
    m2 = torch.zeros_like(m3, requires_grad=True)
    col = leaf("shs") if mode == "sh" else leaf("colors_precomp")
    leaves = [m3, m2, op, sc, rot, col]
    raster_C.invalidate_geometry_cache()
    f = lambda t_: t_.float().to(dev)
    if kind == "single":
        color, radii, depth = rast(means3D=m3, means2D=m2, opacities=op, scales=sc, rotations=rot,
                                   **({"shs": col} if mode == "sh" else {"colors_precomp": col}))
        loss = (color * f(gc)).sum() + (depth * f(gd)).sum()
    elif kind == "alpha":
        color, radii, depth, alpha = rast.forward_alpha(means3D=m3, means2D=m2, opacities=op, scales=sc, rotations=rot,
                                                        **({"shs": col} if mode == "sh" else {"colors_precomp": col}))
        loss = (color * f(gc)).sum() + (depth * f(gd)).sum() + (alpha * f(ga)).sum()
    else:
        col2 = s["colors_precomp"].flip(0).to(dev).clone().requires_grad_(True)
        leaves.append(col2)
        color, radii, depth, color2 = rast.forward_pair(means3D=m3, means2D=m2, opacities=op, colors_a=col, colors_b=col2, scales=sc,
                                                        rotations=rot, densify_accum=acc)
        loss = (color * f(gc)).sum() + (depth * f(gd)).sum() + (color2 * f(gc2)).sum()
    loss.backward()
    cam_grads = (rs.viewmatrix.grad, rs.projmatrix.grad, rs.campos.grad) if camera_grad else None
    return [t_.grad for t_ in leaves], cam_grads


@pytest.mark.parametrize("kind,mode", [("single", "sh"), ("single", "precomp"), ("alpha", "sh"), ("pair", "precomp"), ("pair_densify", "precomp")])
def test_camera_gradients_through_the_rasterizer_nodes(gpu_device, kind, mode):
    dev = gpu_device
    P = 300
    s = camera_scene(11, P=P, W=W, H=H)
    gc, gd = upstream(11, H, W)
    gc2, ga = upstream(12, H, W)
    ga = ga if kind == "alpha" else None
    accs = [tuple(torch.zeros(n, device=dev) for n in ((P, 1), (P, 1), (P,))) for _ in range(2)] if kind == "pair_densify" else [None, None]
    plain, _ = _through_node(s, kind, mode, dev, gc, gd, gc2, ga, False, accs[0])
    grads, cam_grads = _through_node(s, kind, mode, dev, gc, gd, gc2, ga, True, accs[1])
    for a, b_ in zip(plain, grads):          # nothing else moves, bit for bit
        assert (a is None and b_ is None) or torch.equal(a, b_)
    if accs[0] is not None:
        assert all(torch.equal(a, b_) for a, b_ in zip(*accs)) and float(accs[0][1].sum()) > 0
    gview, gproj, gcam = cam_grads
    assert gview.shape == (4, 4) and gproj.shape == (4, 4) and gcam.shape == (3,) and gview.dtype == torch.float32
    got = torch.cat([gview.reshape(-1), gproj.reshape(-1), gcam.reshape(-1)]).double().cpu().numpy()
    truth, truth_m3 = _truth(s, kind, mode, gc, gd, gc2, ga)
    # sum|term| of this node's loss: the restatement on the library's own per-Gaussian outputs for the same upstream gradients
    pair = kind.startswith("pair")
    b = _library_backward(s, mode, dev, gc, gd, colors2=s["colors_precomp"].flip(0).to(dev).contiguous() if pair else None,
                          gc2=gc2 if pair else None, galpha=ga)
    _, abs_sums = _restatement(b)
    means3D_rel = rel_l2(grads[0].cpu().numpy(), truth_m3)
    errs = block_errors(got, truth, abs_sums)
    print(kind, mode, "means3D_rel", means3D_rel, errs)
    assert math.isfinite(means3D_rel) and means3D_rel > 0
    for name, err in errs.items():
        if name == "campos" and mode != "sh":
            assert not got[BLOCKS[name]].any() and not truth[BLOCKS[name]].any()
            continue
        assert err <= 4 * means3D_rel, (name, err, means3D_rel)
        assert np.abs(got[BLOCKS[name]]).max() > 0
    for j in UNUSED:
        assert got[j] == 0.0


def test_only_the_cameras_that_ask_get_a_gradient(gpu_device):
    from diff_gaussian_rasterization import GaussianRasterizer
    dev = gpu_device
    s = camera_scene(11, P=300, W=W, H=H)
    rs = settings_from(s, dev)
    rs = rs._replace(viewmatrix=rs.viewmatrix.clone().requires_grad_(True))
    m3 = s["means3D"].to(dev)           # no per-Gaussian input requires a gradient: the camera alone keeps the backward alive
    color, _, depth = GaussianRasterizer(raster_settings=rs)(means3D=m3, means2D=torch.zeros_like(m3), opacities=s["opacities"].to(dev),
                                                              colors_precomp=s["colors_precomp"].to(dev), scales=s["scales"].to(dev),
                                                              rotations=s["rotations"].to(dev))
    (color.sum() + depth.sum()).backward()
    assert rs.viewmatrix.grad is not None and float(rs.viewmatrix.grad.abs().max()) > 0
    assert rs.projmatrix.grad is None and rs.campos.grad is None


def test_zeros_after_an_overflowed_asynchronous_forward(gpu_device, monkeypatch):
    """tests/test_async_gpu.py's arrangement: the speculative policy with a capacity the scene does not fit.  The backward's
    gradients are zeros then and the arena holds nothing defined: the camera gradients are zeros, not NaN."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from s3gaussian_amd import raster_C
    from tests.util import tiny_scene
    dev = gpu_device
    s = tiny_scene(P=4000, W=160, H=112, seed=8)
    prev, prev_policy = raster_C.set_async(True), raster_C.set_async_policy("speculative")
    try:
        def run(camera_grad):
            rs = settings_from(s, dev)
            if camera_grad:
                rs = rs._replace(viewmatrix=rs.viewmatrix.clone().requires_grad_(True), projmatrix=rs.projmatrix.clone().requires_grad_(True),
                                 campos=rs.campos.clone().requires_grad_(True))
            leaf = lambda k: s[k].to(dev).clone().requires_grad_(True)
            m3, op, sc, rot, col = leaf("means3D"), leaf("opacities"), leaf("scales"), leaf("rotations"), leaf("colors_precomp")
            col2 = s["colors_precomp"].flip(0).to(dev).clone().requires_grad_(True)
            raster_C.invalidate_geometry_cache()
            color, radii, depth, color2 = GaussianRasterizer(raster_settings=rs).forward_pair(
                means3D=m3, means2D=torch.zeros_like(m3, requires_grad=True), opacities=op, colors_a=col, colors_b=col2, scales=sc, rotations=rot)
            (color.sum() + depth.sum() + color2.sum()).backward()
            return rs, color, op.grad
        run(False)                                                         # learns the true counts of this image size
        torch.cuda.synchronize()
        st = raster_C._async_state(dev)
        st.drain(block=True)
        key = (160, 112)
        true_R = st.hist[key][0]
        assert true_R > 200
        rs, _, _ = run(True)                                               # in capacity: the camera gradients are there
        assert float(rs.viewmatrix.grad.abs().max()) > 0
        st.drain(block=True)
        monkeypatch.setattr(raster_C, "_ASYNC_MIN_INSTANCES", 1)
        st.hist[key] = [true_R // 16, true_R // 16, 4]
        assert st.caps(key)[0] < true_R
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            rs, color, g_op = run(True)
            torch.cuda.synchronize()
            assert int(raster_C.async_skip_flag(dev).item()) == 1         # it did overflow
            bg = s["bg"].to(dev)
            assert torch.equal(color, bg[:, None, None].expand_as(color)) and float(g_op.abs().max()) == 0.0
            for g in (rs.viewmatrix.grad, rs.projmatrix.grad, rs.campos.grad):
                assert torch.equal(g, torch.zeros_like(g))
            raster_C.async_status(block=True)
    finally:
        raster_C.set_async(prev)
        raster_C.set_async_policy(prev_policy)
        raster_C._async_states.pop(dev.index or 0, None)
        raster_C.invalidate_geometry_cache()


# ---- pose kernels -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(POSE_CASES)))
def test_pose_kernels_match_the_restatement(gpu_device, case):
    from s3gaussian_amd import pose
    dev = gpu_device
    cam = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in camera_scene(0)["cam"].items()}
    delta = torch.tensor(POSE_CASES[case], dtype=torch.float64, device=dev, requires_grad=True)
    out = pose.apply_pose_delta(delta, cam)
    assert out["image_width"] == cam["image_width"] and out["time"] == cam["time"]          # the other fields are shared
    d_ref = torch.tensor(POSE_CASES[case], dtype=torch.float64, requires_grad=True)
    ref = pose_map_ref(d_ref, cam["viewmatrix"].cpu(), cam["projmatrix"].cpu())
    # forward: everything in double, rounded once -- the fp32 output is the rounding of a value within 1e-12 of the restatement's
    for name, r in zip(("viewmatrix", "projmatrix", "campos"), ref):
        got, want = out[name].detach().double().cpu(), r.detach()
        assert out[name].dtype == torch.float32 and got.shape == want.shape
        half_ulp = torch.abs(want) * 2.0 ** -24          # at least half an fp32 ulp of the entry
        # 1e-12 of the block's magnitude: an entry is a sum of products of the block's size (exact zeros come out as 1e-17)
        assert bool((torch.abs(got - want) <= half_ulp + 1e-12 * float(want.abs().max())).all()), name
    # backward: six tangents dotted with an arbitrary g35, against the autograd Jacobian of the restatement
    g = torch.Generator().manual_seed(case)
    g35 = torch.randn(35, generator=g, dtype=torch.float32).double()     # fp32 values: the outputs are fp32 tensors, so are their gradients
    flat_ref = torch.cat([r.reshape(-1) for r in ref])
    (want,) = torch.autograd.grad((flat_ref * g35).sum(), d_ref, retain_graph=True)
    J = torch.stack([torch.autograd.grad(flat_ref[j], d_ref, retain_graph=True)[0] for j in range(35)])
    scale = (g35.abs()[:, None] * J.abs()).sum(0)
    flat = torch.cat([out[k].reshape(-1).double() for k in ("viewmatrix", "projmatrix", "campos")])
    (got,) = torch.autograd.grad((flat * g35.to(dev)).sum(), delta)
    assert got.dtype == torch.float64 and bool(torch.isfinite(got).all())
    print("pose case", case, "max |kernel - restatement| / sum|g J| =", float(((got.cpu() - want).abs() / scale).max()))
    assert bool(((got.cpu() - want).abs() <= 1e-12 * scale).all()), (got.cpu(), want)


def test_corrected_camera_at_zero_delta_reproduces_the_camera(gpu_device):
    """view' is exact, campos' and proj' to fp32 rounding: proj' = view0 (view0^-1 proj0) carries the rounding of the rigid inverse
    of an fp32 rotation (2.2e-8 before the final rounding on this camera, tests/test_camera_grad_cpu.py)."""
    from s3gaussian_amd import pose
    dev = gpu_device
    cam = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in camera_scene(0)["cam"].items()}
    r = pose.PoseRefiner(2, dev, lr=1e-3)
    with torch.no_grad():
        out = r.corrected(cam, 1)
    assert torch.equal(out["viewmatrix"], cam["viewmatrix"])
    ulp = lambda t_: 2.0 ** -23 * float(t_.abs().max())
    d_proj = float((out["projmatrix"] - cam["projmatrix"]).abs().max())
    d_cam = float((out["campos"] - cam["campos"]).abs().max())
    print("corrected(cam) at delta = 0: max |proj' - proj| =", d_proj, " max |campos' - campos| =", d_cam)
    assert d_proj <= 2 * ulp(cam["projmatrix"]) and d_cam <= 2 * ulp(cam["campos"])
    poses = r.poses([cam, cam])
    assert poses.shape == (2, 4, 4) and torch.equal(poses[0], cam["viewmatrix"].t())
