"""CPU-only: the reading of the opacity gradient that the blend backward implements, shown on the float64 oracle, and the
properties of the two test scenes that the GPU tests rely on.

The blend backward carries one term through the final transmittance, dL_dalpha += (-T_final / (1 - alpha)) * bg_dot with
bg_dot = bg . dL_dpixel.  A loss on A = 1 - T_final enters as bg_dot - dL/dA and nowhere else.  The truth it is held against is the
oracle's backward of a render with unit colours on black seeded with (g_A, 0, 0): there the gradient travels through the COLOUR
terms (c - accum) * dL_dpixel, a different piece of code."""
import numpy as np
import pytest

from tests import alpha_ref as R
from tests.util import oracle_forward, rel_l2

BAR = 1e-4             # tests/test_raster_gpu.py: GRAD_TOL, COLOR_TOL
OUTLIER_FRAC = 5e-4    # tests/test_raster_gpu.py
GRADS = ("dL_dmeans2D", "dL_dconic", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dscales", "dL_drotations")


@pytest.mark.parametrize("name", ["A", "B"])
def test_scenes_have_the_properties_the_gpu_tests_need(name):
    f = R.forward64(name)
    st, H, W = f["state"], f["_cfg"]["H"], f["_cfg"]["W"]
    counts = st["ranges"][:, 1].astype(np.int64) - st["ranges"][:, 0]
    A = R.alpha64(name)
    assert A.min() >= 0.0 and A.max() <= 1.0
    if name == "A":
        assert (W % 16, H % 16) != (0, 0) and counts[0] == 0 and counts.max() > 0        # partial tiles, an empty first tile
        assert (st["n_contrib"].reshape(H, W)[:16, :16] == 0).all() and (A[:16, :16] == 0.0).all()
        assert (st["n_contrib"] > 0).mean() > 0.3
    else:
        assert counts.max() > 64 and st["n_contrib"].max() > 32                          # more than one 32-entry batch
        g = R.oracle64()
        stopped = R.include_terminating_gaussian(oracle_forward(g, R.scene_b()))
        assert stopped >= 20, stopped                                                     # pixels that terminate early
        assert (st["conic_opacity"][f["radii"] > 0, 3] > 0.99).sum() > 50                 # alphas that reach the 0.99 cap


@pytest.mark.parametrize("name", ["A", "B"])
def test_fp32_oracle_stays_inside_the_flipped_pixel_allowance(name):
    """The GPU opacity is compared with the float64 oracle under the colour image's bar and allowance; the fp32 oracle (libm's exp,
    another rounding of every alpha test) must itself pass on these scenes, or the seeds are wrong."""
    from oracle.oracle import RasterOracle
    f32 = oracle_forward(RasterOracle(np.float32), R.SCENES[name]())
    H, W = f32["_cfg"]["H"], f32["_cfg"]["W"]
    bad = np.abs((1.0 - f32["state"]["final_T"].astype(np.float64)).reshape(H, W) - R.alpha64(name)) > BAR
    assert bad.mean() <= OUTLIER_FRAC, (int(bad.sum()), bad.size)


@pytest.mark.parametrize("name", ["A", "B"])
def test_alpha_is_the_unit_colour_render_on_black(name):
    f = R.forward64_unit(name)
    np.testing.assert_allclose(f["color"][0], R.alpha64(name), rtol=0, atol=1e-12)
    np.testing.assert_array_equal(f["color"][0], f["color"][2])


@pytest.mark.parametrize("name", ["A", "B"])
def test_bg_dot_reading_is_the_gradient_of_an_opacity_loss(name):
    H, W = R.alpha64(name).shape
    g_A = R.upstream(H, W)[2].numpy()
    truth = R.alpha_backward64(name, g_A)
    reading = R.bg_dot_reading64(name, g_A, sign=-1.0)
    for k in GRADS:
        assert np.abs(truth[k]).max() > 0, k
        assert rel_l2(reading[k], truth[k]) <= 1e-9, (k, rel_l2(reading[k], truth[k]))
    # (dL_dcolors is left out: the opacity does not depend on the colours, while both oracle renders above do on theirs)


@pytest.mark.parametrize("name", ["A", "B"])
def test_adding_instead_of_subtracting_is_caught(name):
    H, W = R.alpha64(name).shape
    g_A = R.upstream(H, W)[2].numpy()
    truth = R.alpha_backward64(name, g_A)
    wrong = R.bg_dot_reading64(name, g_A, sign=+1.0)
    for k in GRADS:
        assert rel_l2(wrong[k], truth[k]) >= 10 * BAR, (k, rel_l2(wrong[k], truth[k]))


def test_counting_the_terminating_gaussian_is_caught():
    """1 - sum(w) with the Gaussian that ended a pixel's walk included is another function: on scene B, whose pixels do stop early,
    at least one gradient moves by ten bars or more."""
    H, W = R.alpha64("B").shape
    g_A = R.upstream(H, W)[2].numpy()
    truth = R.alpha_backward64("B", g_A)

    def forward(s):
        f = oracle_forward(R.oracle64(), s)
        assert R.include_terminating_gaussian(f) > 0
        return f

    wrong = R.bg_dot_reading64("B", g_A, sign=-1.0, forward=forward)
    errs = {k: rel_l2(wrong[k], truth[k]) for k in GRADS}
    assert max(errs.values()) >= 10 * BAR, errs


def test_sky_loss_restatement_matches_the_formula():
    import torch
    a, s = R.sky_inputs(13, 11)
    loss, grad = R.sky_loss_ref(a, s)
    ad = torch.clamp(a.double(), R.LO, R.HI)
    sd = s.double()
    want = (-(1 - sd) * torch.log(ad) - sd * torch.log(1 - ad)).mean()
    assert abs(float(loss) - float(want)) <= 1e-12 * abs(float(want))
    outside = (a.double() < R.LO) | (a.double() > R.HI)
    assert outside.any() and (grad[outside] == 0).all() and (grad[~outside] != 0).any()


def test_video_key_restatement_reproduces_the_references_recorded_frames():
    """tests/golden/sky_frames.npz holds what the reference's own save_seperate_videos wrote for "opacities", "sky_masks" and
    "gt_sky_masks" (tests/golden/make_golden_sky_frames.py); alpha_ref.video_strips must give the same bytes."""
    from tests import frames_ref as fr
    z = np.load(R.SKY_FIXTURE)
    for H, W in fr.SIZES:
        tag = f"s{H}x{W}"
        mine = R.video_strips(list(z[f"{tag}_in_opacities"][:, 0]), list(z[f"{tag}_in_gt_sky_masks"][:, 0]), fr.NUM_CAMS)
        for k in R.VIDEO_KEYS:
            rec = z[f"{tag}_frames_{k}"]
            assert rec.shape == ((fr.NUM_TIMESTAMPS, H, fr.NUM_CAMS * W) + (() if k == "opacities" else (3,)))
            for t in range(fr.NUM_TIMESTAMPS):
                assert np.array_equal(mine[k][t], rec[t]), (tag, k, t)
            assert np.array_equal(mine[k][fr.NUM_TIMESTAMPS // 2], z[f"{tag}_middle_{k}"])
        # 1 - x is formed in fp32 BEFORE the byte: the byte of the complement is not the complement of the byte
        o = z[f"{tag}_in_opacities"][:, 0]
        assert (fr.to8b(1 - o) != 255 - fr.to8b(o)).any()


def test_surface_exists_and_refuses_cpu_tensors():
    """The names the feature adds, their place in the C ABI, and -- like every other operator here -- no CPU fallback."""
    import inspect
    import torch
    from s3gaussian_amd import _lib, pipeline, sky
    from s3gaussian_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    L = _lib.lib()
    for sym in ("s3g_raster_alpha", "s3g_raster_backward_alpha", "s3g_sky_loss", "s3g_sky_loss_workspace_bytes"):
        assert sym in _lib.EXPORTED_SYMBOLS and hasattr(L, sym), sym
    assert L.s3g_sky_loss_workspace_bytes(0, 5) == 0 and L.s3g_sky_loss_workspace_bytes(37, 29) == 128      # two partials, padded
    assert L.s3g_sky_loss_workspace_bytes(1600, 1066) >= 8 * ((1600 * 1066 + 1023) // 1024)
    assert L.s3g_raster_alpha(0, 4, None, None, None) == 1 and b"s3g_raster_alpha" in L.s3g_last_error()     # refused before any launch
    assert list(inspect.signature(GaussianRasterizer.forward).parameters) == list(inspect.signature(GaussianRasterizer.forward_alpha).parameters)
    assert inspect.signature(GaussianRasterizer.forward_pair).parameters["with_alpha"].default is False
    assert inspect.signature(pipeline.render).parameters["return_alpha"].default is False
    for fn, arg in ((pipeline.training_step, "sky_mask"), (pipeline.training_loss, "sky_mask"), (pipeline.training_step_views, "sky_masks"),
                    (pipeline.training_loss_views, "sky_masks"), (pipeline.evaluate_video, "sky_masks")):
        assert inspect.signature(fn).parameters[arg].default is None
    assert pipeline.SKY_VIDEO_KEYS == ("opacities", "sky_masks", "gt_sky_masks") and not set(pipeline.SKY_VIDEO_KEYS) & set(pipeline.VIDEO_KEYS)
    assert inspect.signature(pipeline.evaluate_video).parameters["sky_keys"].default == ()
    assert not hasattr(pipeline.default_opt(), "lambda_sky") and pipeline.default_opt(lambda_sky=0.1).lambda_sky == 0.1
    rs = GaussianRasterizationSettings(image_height=16, image_width=16, tanfovx=1.0, tanfovy=1.0, bg=torch.zeros(3), scale_modifier=1.0,
                                       viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0, campos=torch.zeros(3),
                                       prefiltered=False, debug=False)
    x = torch.rand(4, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        GaussianRasterizer(rs).forward_alpha(means3D=x, means2D=x, opacities=torch.zeros(4, 1), colors_precomp=x, scales=x,
                                             rotations=torch.zeros(4, 4))
    with pytest.raises(Exception, match="excatly one of either SHs or precomputed colors"):
        GaussianRasterizer(rs).forward_alpha(means3D=x, means2D=x, opacities=torch.zeros(4, 1), scales=x, rotations=torch.zeros(4, 4))
    with pytest.raises(RuntimeError, match="GPU"):
        sky.sky_opacity_loss(torch.rand(1, 4, 4), torch.rand(4, 4))
    with pytest.raises(RuntimeError, match="GPU"):
        sky.opacity_image(torch.zeros(64, dtype=torch.uint8), 4, 4)
