"""Rasterizer parity PINNED BY THE REFERENCE ITSELF.

oracle/_ref/libref_raster.so is the reference's own forward.cu / backward.cu / rasterizer_impl.cu (hipify-perl + hipcc for
gfx950, recipe oracle/build_ref.sh, host-pointer shim oracle/ref_shim.cpp).  Three-way comparison on the same seeded inputs:

  reference build  <->  CPU oracle (oracle/raster_oracle.c)      pins the restatement every other raster test relies on
  reference build  <->  libs3g.so through the `_C` signatures     the product against the real thing
  CPU oracle       <->  libs3g.so at BASELINE cfg2 / cfg3 size    (the oracle needs ~5 s per view on 8 cores)

Bars, written where they are asserted:
  * integer / index state -- radii, tiles_touched, point_offsets, num_rendered, tile ranges, sorted keys, point_list:
    EXACT (libs3g with the reference's bounding-square binning, `set_exact_cull(False)`);
  * per-Gaussian fp32 state (depths, means2D, cov3D, conic_opacity, rgb, clamped): bit-exact against the
    -ffp-contract=off build of the reference;
  * n_contrib: exact, final_T <= 2e-5 abs, colour <= 1e-4 abs, depth <= 1e-4 rel -- outside at most 0.05 % of pixels, where
    a borderline skip test (alpha ~ 1/255, T ~ 1e-4) flips between exp implementations (libm / ocml / v_exp_f32);
  * gradients (all 10 arrays of RAST/rasterize_points.cu:154-163): rel-L2 <= 1e-4, compared with the flipped pixels
    masked out of the upstream gradient on BOTH sides (so no seed can skip the comparison).  The reference backward sums
    with float atomics; its own run-to-run spread is measured and recorded.

Every comparison appends its numbers to gpurun_out/parity_stats.jsonl (copied to profiles/ for the record).
"""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests.util import oracle_forward, rel_l2, tiny_scene

pytestmark = pytest.mark.gpu

COLOR_TOL = 1e-4
DEPTH_RTOL = 1e-4
FINAL_T_TOL = 2e-5
GRAD_TOL = 1e-4
OUTLIER_FRAC = 5e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_NAMES = ("dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dcolors", "dL_ddepths", "dL_dmeans3D", "dL_dcov3D", "dL_dsh",
              "dL_dscales", "dL_drotations")


def _record(**kw):
    try:
        os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
        with open(os.path.join(ROOT, "gpurun_out", "parity_stats.jsonl"), "a") as f:
            f.write(json.dumps(kw) + "\n")
    except OSError:
        pass


@pytest.fixture(scope="module")
def oracle():
    from oracle.oracle import RasterOracle
    return RasterOracle(np.float32)


@pytest.fixture(scope="module")
def ref(gpu_device):
    from oracle import ref_raster
    if not ref_raster.available():
        pytest.fail("oracle/_ref/libref_raster.so missing: run oracle/build_ref.sh (needs /root/reference) before gpurun")
    return ref_raster.RefRaster()


# ---- scenes ------------------------------------------------------------------------------------------------------------
def _street(P, scale_mult=1.0, cam=4):
    from s3gaussian_amd import synth
    sc = synth.street_scene(P=P, seed=0, n_frames=4)
    gs = sc["gaussians"]
    g = torch.Generator().manual_seed(1)
    return dict(means3D=gs["xyz"], scales=torch.exp(gs["log_scales"]) * scale_mult,
                rotations=torch.nn.functional.normalize(gs["rotations_raw"]), opacities=torch.sigmoid(gs["opacity_logit"]),
                shs=gs["shs"], colors_precomp=torch.rand(P, 3, generator=g), cam=sc["cameras"][cam], bg=sc["bg"])


def _cfg1():
    from s3gaussian_amd import synth
    sc = synth.cfg1_scene()
    gs = sc["gaussians"]
    return dict(means3D=gs["xyz"], scales=torch.exp(gs["log_scales"]), rotations=gs["rotations_raw"],
                opacities=torch.sigmoid(gs["opacity_logit"]), shs=gs["shs"], colors_precomp=torch.rand(10_000, 3),
                cam=sc["cameras"][0], bg=sc["bg"])


def _ties():
    s = tiny_scene(P=500, W=32, H=32, seed=7, scale=0.2)
    s["means3D"][:, 2] = 4.0
    return s


def _long_lists():
    s = tiny_scene(P=18000, W=32, H=16, seed=11, scale=0.02, spread=0.25)
    s["opacities"] = s["opacities"] * 0.05
    return s


def _bucket_lists(P, seed):
    """Round 6: lists of (1024, 4096] keys take the bucket pass of the per-tile sort in a launch of their own, lists of (4096, 7424]
    keys in the long-list launch (csrc/raster_sort.hip::bucket_sort_lds); two tiles share P Gaussians here."""
    s = tiny_scene(P=P, W=32, H=16, seed=seed, scale=0.02, spread=0.25)
    s["opacities"] = s["opacities"] * 0.05
    return s


def _bucket_ties():
    """Thousands of instances at ONE depth: the bucket pass finds a single bucket and the index decides the order."""
    s = tiny_scene(P=3000, W=32, H=16, seed=17, scale=0.02, spread=0.25)
    s["means3D"][:, 2] = 4.0
    s["means3D"][::3, 2] = 4.5
    s["opacities"] = s["opacities"] * 0.05
    return s


def _huge():
    s = tiny_scene(P=3, W=80, H=48)
    s["means3D"][:] = torch.tensor([[0.0, 0.0, 2.0], [0.3, -0.2, 2.5], [-0.4, 0.1, 3.0]])
    s["scales"][:] = torch.tensor([5.0, 2.0, 0.5])[:, None]
    s["opacities"][:] = 0.6
    return s


def _near_plane():
    """Gaussians straddling the 0.2 near cull and far outside the frustum sides (clamped t.xy in computeCov2D)."""
    s = tiny_scene(P=1500, W=64, H=64, seed=13, scale=0.1, spread=6.0, zmin=0.05, zmax=1.5)
    return s


SCENES = {
    "tiny_precomp": (lambda: tiny_scene(P=400, W=48, H=40, seed=1), "precomp"),
    "tiny_sh": (lambda: tiny_scene(P=400, W=33, H=17, seed=1), "sh"),
    "state_2000": (lambda: tiny_scene(P=2000, W=96, H=80, seed=3, scale=0.06), "precomp"),
    "depth_ties": (_ties, "precomp"),
    "long_lists": (_long_lists, "precomp"),
    "bucket_lists_mid": (lambda: _bucket_lists(5000, 19), "precomp"),
    "bucket_lists_long": (lambda: _bucket_lists(11000, 23), "precomp"),
    "bucket_ties": (_bucket_ties, "precomp"),
    "huge": (_huge, "precomp"),
    "near_plane": (_near_plane, "sh"),
    "cov3d_precomp": (lambda: tiny_scene(P=300, W=48, H=48, seed=2), "cov3d"),
    "cfg1": (_cfg1, "sh"),
    "cfg2_view": (lambda: _street(600_000), "sh"),
    "cfg3_view": (lambda: _street(1_200_000), "precomp"),
    "cfg3_view_big_splats": (lambda: _street(1_200_000, scale_mult=2.5, cam=7), "precomp"),
}
SMALL = [k for k in SCENES if not k.startswith(("cfg2", "cfg3"))]
FULL = [k for k in SCENES if k.startswith(("cfg2", "cfg3"))]


def _checker_forward(chk, s, mode, oracle):
    if mode == "cov3d":
        cov = oracle_forward(oracle, s)["state"]["cov3D"].copy()
        return oracle_forward(chk, s, scales=None, rotations=None, cov3D_precomp=cov), cov
    return oracle_forward(chk, s, mode=mode), None


# ---- libs3g through the reference's `_C` signatures --------------------------------------------------------------------
def _gpu_forward(s, dev, mode, cov3D=None):
    from diff_gaussian_rasterization import _C
    from s3gaussian_amd import _debug
    cam = s["cam"]
    e = torch.Tensor([])
    P = s["means3D"].shape[0]
    H, W = cam["image_height"], cam["image_width"]
    d = lambda k: s[k].to(dev).contiguous()
    sh, col, deg = (d("shs"), e, 3) if mode == "sh" else (e, d("colors_precomp"), 0)
    sc, rot, cov = (e, e, torch.from_numpy(cov3D).to(dev)) if cov3D is not None else (d("scales"), d("rotations"), e)
    args = dict(bg=s["bg"].to(dev), means3D=d("means3D"), colors=col, opacity=d("opacities"), scales=sc, rotations=rot, cov=cov,
                view=cam["viewmatrix"].to(dev), proj=cam["projmatrix"].to(dev), campos=cam["campos"].to(dev), sh=sh, deg=deg)
    R, color, depth, radii, geom, binning, img = _C.rasterize_gaussians(
        args["bg"], args["means3D"], col, args["opacity"], sc, rot, 1.0, cov, args["view"], args["proj"], cam["tanfovx"],
        cam["tanfovy"], H, W, sh, deg, args["campos"], False, False)
    g, im, b = _debug.decode_geometry(geom, P), _debug.decode_image(img, W, H), _debug.decode_binning(binning, R)
    rect = g["rect"].long()
    n = lambda t: t.cpu().numpy()
    state = dict(depths=n(g["depths"]), means2D=n(g["means2D"]), cov3D=n(g["cov3D"]), conic_opacity=n(g["conic_opacity"]),
                 rgb=n(g["rgb"]), clamped=n(g["clamped"]).reshape(-1),
                 tiles_touched=n((rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1])).astype(np.uint32),
                 ranges=n(im["ranges"]).astype(np.uint32), final_T=n(im["final_T"]).reshape(-1),
                 n_contrib=n(im["n_contrib"]).reshape(-1).astype(np.uint32), point_list=n(b["point_list"]).astype(np.uint32))
    return dict(color=n(color), depth=n(depth), radii=n(radii), num_rendered=R, state=state,
                _raw=(args, cam, radii, geom, binning, img, R, H, W))


def _gpu_backward(fw, gc, gd):
    from diff_gaussian_rasterization import _C
    a, cam, radii, geom, binning, img, R, H, W = fw["_raw"]
    dev = a["means3D"].device
    out = _C.rasterize_gaussians_backward(
        a["bg"], a["means3D"], radii, a["colors"], a["scales"], a["rotations"], 1.0, a["cov"], a["view"], a["proj"],
        cam["tanfovx"], cam["tanfovy"], torch.from_numpy(gc).to(dev), torch.from_numpy(gd).to(dev).view(1, H, W), a["sh"], a["deg"],
        a["campos"], geom, R, binning, img, False, return_internals=True)
    m2, col, op, m3, cov, sh, sc, rot, conic, dep = [t.cpu().numpy() for t in out]
    return dict(dL_dmeans2D=m2, dL_dconic=conic, dL_dopacity=op, dL_dcolors=col, dL_ddepths=dep, dL_dmeans3D=m3, dL_dcov3D=cov,
                dL_dsh=sh, dL_dscales=sc, dL_drotations=rot)


# ---- comparisons -------------------------------------------------------------------------------------------------------
def _compare_forward(a, b, tag, scene, mode, exact_float_state=True, lists=True):
    """a = side under test, b = the pinning side.  Returns the bool [H*W] mask of flipped / out-of-tolerance pixels.
    The reference leaves geom.rgb / clamped unwritten with precomputed colours and geom.cov3D unwritten with a precomputed
    covariance (forward.cu:216-247): those arrays are compared only in the modes that define them."""
    sa, sb = a["state"], b["state"]
    np.testing.assert_array_equal(a["radii"], b["radii"])
    vis = b["radii"] > 0
    np.testing.assert_array_equal(sa["tiles_touched"][vis], sb["tiles_touched"][vis])
    if lists:
        assert a["num_rendered"] == b["num_rendered"]
        ra, rb = sa["ranges"].astype(np.int64), sb["ranges"].astype(np.int64)
        np.testing.assert_array_equal(ra[:, 1] - ra[:, 0], rb[:, 1] - rb[:, 0])
        nonempty = (rb[:, 1] - rb[:, 0]) > 0
        np.testing.assert_array_equal(ra[nonempty], rb[nonempty])
        np.testing.assert_array_equal(sa["point_list"], sb["point_list"])
        if "point_list_keys" in sa and "point_list_keys" in sb:
            np.testing.assert_array_equal(sa["point_list_keys"], sb["point_list_keys"])
    fstate = {}
    fields = [("depths", 1), ("means2D", 2), ("conic_opacity", 4)] + ([("cov3D", 6)] if mode != "cov3d" else []) + \
        ([("rgb", 3)] if mode == "sh" else [])
    for k, w in fields:
        x, y = sa[k].reshape(-1, w)[vis], sb[k].reshape(-1, w)[vis]
        fstate[k] = int((x.view(np.uint32) != y.view(np.uint32)).any(1).sum()) if x.size else 0
    if mode == "sh":
        x, y = sa["clamped"].reshape(-1, 3)[vis].astype(bool), sb["clamped"].reshape(-1, 3)[vis].astype(bool)
        fstate["clamped"] = int((x != y).any(1).sum()) if x.size else 0
    dc = np.abs(a["color"] - b["color"]).max(0).reshape(-1)
    dd = (np.abs(a["depth"] - b["depth"])[0] / (1 + np.abs(b["depth"][0]))).reshape(-1)
    dn = sa["n_contrib"] != sb["n_contrib"]
    dT = np.abs(sa["final_T"] - sb["final_T"])
    bad = dn | (dc > COLOR_TOL) | (dd > DEPTH_RTOL) | (dT > FINAL_T_TOL)
    good = ~bad
    _record(test=tag, scene=scene, P=int(a["radii"].size), R=int(b["num_rendered"]), visible=int(vis.sum()),
            pixels=int(bad.size), flipped_pixels=int(bad.sum()), n_contrib_mismatch=int(dn.sum()),
            color_max_abs_good=float(dc[good].max()) if good.any() else 0.0,
            depth_max_rel_good=float(dd[good].max()) if good.any() else 0.0,
            final_T_max_abs_good=float(dT[good].max()) if good.any() else 0.0, float_state_rows_not_bit_equal=fstate)
    if exact_float_state:
        assert all(v == 0 for v in fstate.values()), fstate
    assert bad.mean() <= OUTLIER_FRAC, f"{tag}/{scene}: {int(bad.sum())} of {bad.size} pixels flipped / outside tolerance"
    return bad


def _masked_grads(bad, H, W, seed=5):
    g = torch.Generator().manual_seed(seed)
    gc, gd = torch.randn(3, H, W, generator=g).numpy(), torch.randn(1, H, W, generator=g).numpy()
    keep = (~bad).reshape(1, H, W).astype(np.float32)
    return np.ascontiguousarray(gc * keep), np.ascontiguousarray(gd * keep)


def _compare_grads(ga, gb, tag, scene, tol=GRAD_TOL, skip=()):
    errs = {}
    for k in GRAD_NAMES:
        if k in skip or gb[k].size == 0:
            continue
        x, y = ga[k], gb[k]
        if k == "dL_dconic":   # [P,2,2]: .z (index [1,0]) is unused by the reference (backward.cu: conic.y carries b)
            x, y = x.reshape(-1, 4)[:, [0, 1, 3]], y.reshape(-1, 4)[:, [0, 1, 3]]
        if k == "dL_dmeans2D":  # third column is a dummy
            x, y = x[:, :2], y[:, :2]
        errs[k] = rel_l2(x, y) if np.linalg.norm(y) > 0 else float(np.abs(x).max())
    _record(test=tag + ":grads", scene=scene, rel_l2=errs)
    worst = max(errs, key=errs.get)
    assert errs[worst] <= tol, f"{tag}/{scene}: {worst} rel-L2 {errs[worst]:.3e} > {tol} ({errs})"
    return errs


# ---- tests -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", SMALL + FULL)
def test_cpu_oracle_is_pinned_by_the_reference_build(ref, oracle, scene):
    """oracle/raster_oracle.c against the reference's own kernels: this is what un-caps `parity unpinned`."""
    build, mode = SCENES[scene]
    s = build()
    H, W = s["cam"]["image_height"], s["cam"]["image_width"]
    r, cov = _checker_forward(ref, s, mode, oracle)
    o, _ = _checker_forward(oracle, s, mode, oracle)
    np.testing.assert_array_equal(o["state"]["point_offsets"][: o["radii"].size], r["state"]["point_offsets"][: r["radii"].size])
    bad = _compare_forward(o, r, "oracle_vs_ref", scene, mode)
    gc, gd = _masked_grads(bad, H, W)
    go, gr = oracle.backward(o, gc, gd), ref.backward(r, gc, gd)
    _compare_grads(go, gr, "oracle_vs_ref", scene)


@pytest.mark.parametrize("scene", SMALL + FULL)
def test_libs3g_matches_the_reference_build(gpu_device, ref, oracle, reference_binning, scene):
    """The product (C ABI, reference `_C` signatures, reference binning) against the reference's own kernels."""
    build, mode = SCENES[scene]
    s = build()
    H, W = s["cam"]["image_height"], s["cam"]["image_width"]
    r, cov = _checker_forward(ref, s, mode, oracle)
    g = _gpu_forward(s, gpu_device, mode, cov3D=cov)
    bad = _compare_forward(g, r, "libs3g_vs_ref", scene, mode)
    gc, gd = _masked_grads(bad, H, W)
    gg, gr = _gpu_backward(g, gc, gd), ref.backward(r, gc, gd)
    _compare_grads(gg, gr, "libs3g_vs_ref", scene)


@pytest.mark.parametrize("scene", FULL)
def test_libs3g_matches_the_cpu_oracle_at_baseline_size(gpu_device, oracle, reference_binning, scene):
    """cfg2 / cfg3 views at full size against the CPU oracle (no BASELINE config stays property-only)."""
    build, mode = SCENES[scene]
    s = build()
    H, W = s["cam"]["image_height"], s["cam"]["image_width"]
    o, _ = _checker_forward(oracle, s, mode, oracle)
    g = _gpu_forward(s, gpu_device, mode)
    bad = _compare_forward(g, o, "libs3g_vs_oracle", scene, mode)
    gc, gd = _masked_grads(bad, H, W)
    _compare_grads(_gpu_backward(g, gc, gd), oracle.backward(o, gc, gd), "libs3g_vs_oracle", scene)


@pytest.mark.parametrize("scene", ["state_2000", "cfg3_view"])
def test_exact_cull_default_path_matches_the_reference_images(gpu_device, ref, oracle, scene):
    """Default product configuration (exact tile culling ON: private lists are a subset): images, radii and gradients
    against the reference build; n_contrib is a list position and is not comparable in this mode."""
    build, mode = SCENES[scene]
    s = build()
    H, W = s["cam"]["image_height"], s["cam"]["image_width"]
    r, _ = _checker_forward(ref, s, mode, oracle)
    g = _gpu_forward(s, gpu_device, mode)
    np.testing.assert_array_equal(g["radii"], r["radii"])
    assert g["num_rendered"] <= r["num_rendered"]
    dc = np.abs(g["color"] - r["color"]).max(0).reshape(-1)
    dd = (np.abs(g["depth"] - r["depth"])[0] / (1 + np.abs(r["depth"][0]))).reshape(-1)
    dT = np.abs(g["state"]["final_T"] - r["state"]["final_T"])
    bad = (dc > COLOR_TOL) | (dd > DEPTH_RTOL) | (dT > FINAL_T_TOL)
    _record(test="libs3g_exact_cull_vs_ref", scene=scene, R_product=int(g["num_rendered"]), R_reference=int(r["num_rendered"]),
            flipped_pixels=int(bad.sum()), pixels=int(bad.size))
    assert bad.mean() <= OUTLIER_FRAC
    gc, gd = _masked_grads(bad, H, W)
    _compare_grads(_gpu_backward(g, gc, gd), ref.backward(r, gc, gd), "libs3g_exact_cull_vs_ref", scene)


def test_reference_backward_run_to_run_spread_and_ours_is_reproducible(gpu_device, ref, oracle, reference_binning):
    """The reference accumulates with float atomics (backward.cu:550-587): two runs on identical inputs differ.  Records
    that spread (the floor of any gradient comparison against it) and asserts the product's gradients are bit-reproducible."""
    s = _street(1_200_000)
    H, W = s["cam"]["image_height"], s["cam"]["image_width"]
    r = oracle_forward(ref, s)
    gc, gd = _masked_grads(np.zeros(H * W, bool), H, W)
    g1, g2 = ref.backward(r, gc, gd), ref.backward(r, gc, gd)
    spread = {k: rel_l2(g1[k], g2[k]) for k in GRAD_NAMES if g1[k].size and np.linalg.norm(g2[k]) > 0}
    g = _gpu_forward(s, gpu_device, "precomp")
    a, b = _gpu_backward(g, gc, gd), _gpu_backward(g, gc, gd)
    _record(test="reference_backward_run_to_run", scene="cfg3_view", rel_l2=spread,
            bit_identical_arrays=int(sum(np.array_equal(g1[k], g2[k]) for k in spread)))
    assert max(spread.values()) <= GRAD_TOL
    for k in GRAD_NAMES:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("scene", ["state_2000", "cfg1", "cfg3_view"])
def test_fma_build_of_the_reference_stays_inside_the_stated_tolerances(gpu_device, oracle, scene):
    """nvcc contracts a*b+c by default, hipcc too: the reference as a user runs it is the FMA build.  Its integer outputs
    may differ from the one-rounding build for Gaussians whose radius / rect / cull test sits within an ulp of a boundary
    (SURVEY 8c): count them (<= 0.05 % of the visible Gaussians) and hold images to the same tolerances on the pixels that
    none of those Gaussians touch."""
    from oracle.ref_raster import RefRaster
    build, mode = SCENES[scene]
    s = build()
    strict, _ = _checker_forward(RefRaster(), s, mode, oracle)
    fma, _ = _checker_forward(RefRaster(fma=True), s, mode, oracle)
    vis = strict["radii"] > 0
    d_radii = int((strict["radii"] != fma["radii"]).sum())
    d_tiles = int((strict["state"]["tiles_touched"] != fma["state"]["tiles_touched"]).sum())
    dc = np.abs(strict["color"] - fma["color"]).max(0)
    _record(test="ref_fma_vs_ref_strict", scene=scene, visible=int(vis.sum()), radii_differ=d_radii, tiles_touched_differ=d_tiles,
            num_rendered=[int(strict["num_rendered"]), int(fma["num_rendered"])], color_max_abs=float(dc.max()),
            pixels_over_tol=int((dc > COLOR_TOL).sum()), pixels=int(dc.size))
    assert d_radii <= max(2, 5e-4 * vis.sum())
    assert (dc > COLOR_TOL).mean() <= 2e-3


def test_mark_visible_matches_the_reference_build(gpu_device, ref):
    from diff_gaussian_rasterization import GaussianRasterizer
    from tests.util import settings_from
    s = tiny_scene(P=5000, W=32, H=32, zmin=-1.0, zmax=1.0)
    s["means3D"][:50, 2] = 0.2          # exactly on the cull plane: `p_view.z <= 0.2` culls (auxiliary.h:153)
    rast = GaussianRasterizer(raster_settings=settings_from(s, gpu_device))
    vis = rast.markVisible(s["means3D"].to(gpu_device)).cpu().numpy()
    want = ref.mark_visible(s["means3D"].numpy(), s["cam"]["viewmatrix"].numpy(), s["cam"]["projmatrix"].numpy())
    np.testing.assert_array_equal(vis, want)
