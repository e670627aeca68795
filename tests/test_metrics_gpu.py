"""GPU: s3gaussian_amd.metrics.image_metrics (csrc/metrics.hip) and pipeline.evaluate against the float64 restatement of
tests/metrics_ref.py and the recorded reference values of tests/golden/eval_metrics.npz.

Shapes (metrics_ref.SHAPES, tile 32 x 16): 7x7 (every window all border, one interior pixel), 9x23 (smaller than a tile, ragged), 37x53
(tile boundaries both ways, ragged last tiles), 64x96 (exact tile multiple), 70x100.  Masks: the fixture's random one (~20 %), full,
empty, absent, one pixel at (0,0), one at (H-1,W-1).

Bars (nothing here is derived from what the kernel gives):
  map, per pixel   8 x map_spread, map_spread = the largest |S_fp32 - S_fp64| of the restatement over the fixture inputs (1.79e-5,
                   measured by tests/golden/make_golden_metrics.py and recorded in the fixture) -> 1.43e-4
  ssim scalars     the same bar: each is a mean of map values
  psnr scalars     1e-5 dB against the float64 evaluation (fp32 differences squared and added in double: ~1.2e-7 relative on an MSE
                   = 5e-7 dB); against the reference's recorded fp32 value: that value's own recorded distance from float64 + 1e-5
tests/test_metrics_cpu.py shows that the plausible wrong readings of the definition are >= 10 bars away on every fixture input."""
import numpy as np
import pytest
import torch

from tests import metrics_ref as mr

pytestmark = pytest.mark.gpu

MASKS = ("random", "full", "empty", "absent", "first_pixel", "last_pixel")


def _mask(case, kind):
    H, W = case["mask"].shape
    if kind == "random":
        return case["mask"]
    if kind == "absent":
        return None
    m = np.full((H, W), 1 if kind == "full" else 0, np.uint8)
    if kind == "first_pixel":
        m[0, 0] = 1
    if kind == "last_pixel":
        m[H - 1, W - 1] = 1
    return m


@pytest.fixture(scope="module")
def ref():
    """The float64 restatement of every (case, mask) pair, computed once and only read afterwards."""
    cases, spread = mr.load_fixture()
    table = [{kind: mr.image_metrics(c["image"], c["gt"], _mask(c, kind), np.float64) for kind in MASKS} for c in cases]
    return cases, spread, table


def _dev(case, dev, kind="random"):
    m = _mask(case, kind)
    return (torch.from_numpy(case["image"]).to(dev), torch.from_numpy(case["gt"]).to(dev),
            None if m is None else torch.from_numpy(m).to(dev))


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


@pytest.mark.parametrize("k", range(len(mr.SHAPES)), ids=[f"{h}x{w}" for h, w in mr.SHAPES])
def test_map_matches_the_restatement_pixel_by_pixel(gpu_device, ref, k):
    from s3gaussian_amd.metrics import image_metrics
    cases, spread, table = ref
    image, gt, mask = _dev(cases[k], gpu_device)
    rec, smap = image_metrics(image, gt, mask, return_map=True)
    assert smap.shape == image.shape and smap.dtype == torch.float32
    err = np.abs(smap.cpu().numpy().astype(np.float64) - table[k]["random"]["map"])
    print(f"{mr.SHAPES[k]}: map max err {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}, bar {mr.MAP_BAR_FACTOR * spread:.3e}")
    assert err.max() <= mr.MAP_BAR_FACTOR * spread


@pytest.mark.parametrize("k", range(len(mr.SHAPES)), ids=[f"{h}x{w}" for h, w in mr.SHAPES])
def test_scalars_match_the_restatement_and_the_recorded_reference(gpu_device, ref, k):
    from s3gaussian_amd.metrics import MASKED_PIXELS, MASKED_PSNR, MASKED_SSIM, PSNR, SSIM, image_metrics
    cases, spread, table = ref
    c, bar = cases[k], mr.MAP_BAR_FACTOR * spread
    for kind in MASKS:
        image, gt, mask = _dev(c, gpu_device, kind)
        got = image_metrics(image, gt, mask).cpu().numpy()
        want = table[k][kind]
        print(f"{mr.SHAPES[k]} {kind:11s}: " + " ".join(f"{n} {got[i]:.9g} (err {abs(got[i] - want[n]):.2e})" for i, n in enumerate(mr.SCALARS))
              + f" pixels {got[MASKED_PIXELS]:.0f}")
        assert got[MASKED_PIXELS] == want["masked_pixels"]
        assert abs(got[PSNR] - want["psnr"]) <= mr.PSNR_BAR and abs(got[SSIM] - want["ssim"]) <= bar
        assert abs(got[PSNR] - c["psnr_ref"]) <= c["psnr_ref_err"] + mr.PSNR_BAR and abs(got[SSIM] - c["ssim_scipy"]) <= bar
        if kind in ("empty", "absent"):
            assert np.isnan(got[MASKED_PSNR]) and np.isnan(got[MASKED_SSIM]) and got[MASKED_PIXELS] == 0
            continue
        assert abs(got[MASKED_PSNR] - want["masked_psnr"]) <= mr.PSNR_BAR and abs(got[MASKED_SSIM] - want["masked_ssim"]) <= bar
        if kind == "random":
            assert abs(got[MASKED_PSNR] - c["masked_psnr_ref"]) <= c["masked_psnr_ref_err"] + mr.PSNR_BAR
            assert abs(got[MASKED_SSIM] - c["masked_ssim_scipy"]) <= bar
        if kind == "full":     # every pixel masked: the masked PSNR is the frame's
            assert got[MASKED_PIXELS] == c["mask"].size and got[MASKED_PSNR] == got[PSNR]


def test_a_channel_without_error_has_infinite_psnr(gpu_device, ref):
    """log10(1 / 0) = +inf for that channel (utils/image_utils.py:17-19), hence for the mean over the channels; identical images have
    S = 1 everywhere."""
    from s3gaussian_amd.metrics import MASKED_PSNR, MASKED_SSIM, PSNR, SSIM, image_metrics
    cases, spread, _ = ref
    image, gt, mask = _dev(cases[2], gpu_device)
    one = image.clone()
    one[1] = gt[1]
    got = image_metrics(one, gt, mask).cpu().numpy()
    assert got[PSNR] == np.inf and got[MASKED_PSNR] == np.inf and np.isfinite(got[SSIM]) and got[SSIM] < 0.99
    got, smap = image_metrics(gt, gt, mask, return_map=True)
    got = got.cpu().numpy()
    assert got[PSNR] == np.inf and got[MASKED_PSNR] == np.inf
    assert abs(got[SSIM] - 1.0) <= mr.MAP_BAR_FACTOR * spread and abs(got[MASKED_SSIM] - 1.0) <= mr.MAP_BAR_FACTOR * spread
    assert float((smap - 1.0).abs().max()) <= mr.MAP_BAR_FACTOR * spread


def test_strides_and_mask_dtypes_do_not_change_a_bit(gpu_device, ref):
    from s3gaussian_amd.metrics import image_metrics
    cases, _, _ = ref
    image, gt, mask = _dev(cases[4], gpu_device)
    base, base_map = image_metrics(image, gt, mask, return_map=True)
    hwc_image, hwc_gt = image.permute(1, 2, 0).contiguous().permute(2, 0, 1), gt.permute(1, 2, 0).contiguous().permute(2, 0, 1)
    assert not hwc_image.is_contiguous() and torch.equal(hwc_image, image)
    wide = torch.zeros(mask.shape[0], 2 * mask.shape[1], dtype=torch.uint8, device=gpu_device)
    wide[:, ::2] = mask
    for im, g, m in ((hwc_image, hwc_gt, mask), (image, gt, mask.bool()), (image, gt, mask.float() * 0.25), (image, gt, mask * 7),
                     (image, gt, wide[:, ::2]), (image, gt, mask[None])):
        rec, smap = image_metrics(im, g, m, return_map=True)
        assert torch.equal(_bits(rec), _bits(base)) and torch.equal(_bits(smap), _bits(base_map))


@pytest.mark.parametrize("k", (2, 4))
def test_two_runs_are_bit_identical(gpu_device, ref, k):
    from s3gaussian_amd.metrics import image_metrics
    cases, _, _ = ref
    image, gt, mask = _dev(cases[k], gpu_device)
    a, amap = image_metrics(image, gt, mask, return_map=True)
    b, bmap = image_metrics(image, gt, mask, return_map=True)
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(amap), _bits(bmap))
    assert torch.equal(_bits(image_metrics(image, gt, mask)), _bits(a))      # the map output does not change the record


def test_out_row_is_the_only_thing_written(gpu_device, ref):
    from s3gaussian_amd.metrics import image_metrics
    cases, _, _ = ref
    image, gt, mask = _dev(cases[1], gpu_device)
    table = torch.full((5, 5), float("nan"), dtype=torch.float64, device=gpu_device)
    back = image_metrics(image, gt, mask, out=table[2])
    assert back.data_ptr() == table[2].data_ptr()
    assert torch.isnan(table[[0, 1, 3, 4]]).all() and torch.equal(_bits(table[2]), _bits(image_metrics(image, gt, mask)))
    with pytest.raises(RuntimeError, match="out must be"):
        image_metrics(image, gt, mask, out=table[:, 2])


def test_images_smaller_than_the_window_raise(gpu_device):
    from s3gaussian_amd.metrics import image_metrics
    x = torch.rand(3, 6, 40, device=gpu_device)
    with pytest.raises(Exception, match="smaller than the 7 x 7"):
        image_metrics(x, x)


def test_evaluate_is_a_loop_of_render_and_image_metrics(gpu_device):
    """pipeline.evaluate on a small cfg1 scene (2 000 Gaussians, 64 x 96, four cameras at two timestamps; cameras 1 and 2 carry a mask,
    camera 2's is empty): its per-frame table equals the plain loop bit for bit, the scalars follow non_zero_mean
    (utils/video_utils.py:44-46), and without masks both masked scalars are -1."""
    from types import SimpleNamespace
    from s3gaussian_amd import synth
    from s3gaussian_amd.metrics import MASKED_PIXELS, MASKED_PSNR, MASKED_SSIM, PSNR, SSIM, image_metrics
    from s3gaussian_amd.pipeline import GaussianParams, default_hyper, evaluate, render
    dev = gpu_device
    scn = synth.cfg1_scene(P=2000, seed=3, width=96, height=64)
    torch.manual_seed(0)
    pc = GaussianParams(3, default_hyper())
    gs = scn["gaussians"]
    pc.init_from_tensors(gs["xyz"], gs["log_scales"], gs["rotations_raw"], gs["opacity_logit"], gs["shs"], dev)
    pc._deformation.deformation_net.set_aabb([2.5, 2.5, 6.5], [-2.5, -2.5, 2.5])
    cam0 = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in scn["cameras"][0].items()}
    cams = [dict(cam0, time=t) for t in (0.0, 0.0, 0.5, 1.0)]
    pipe = SimpleNamespace(convert_SHs_python=True, compute_cov3D_python=False, debug=False)
    bg = scn["bg"].to(dev)
    g = torch.Generator().manual_seed(1)
    gts = [torch.rand(3, 64, 96, generator=g).to(dev) for _ in cams]
    masks = [None, (torch.rand(64, 96, generator=g) < 0.2).to(dev), torch.zeros(64, 96, dtype=torch.bool, device=dev), None]
    out = evaluate(pc, cams, gts, pipe, bg, masks=masks)
    assert set(out) == {"psnr", "ssim", "masked_psnr", "masked_ssim", "per_frame"}
    with torch.no_grad():
        rows = [image_metrics(render(cam, pc, pipe, bg, stage="fine")["render"], gt, m).cpu() for cam, gt, m in zip(cams, gts, masks)]
    loop = torch.stack(rows)
    per_frame = out["per_frame"]
    assert per_frame.shape == (4, 5) and per_frame.dtype == torch.float64 and not per_frame.is_cuda
    assert torch.equal(_bits(per_frame), _bits(loop))
    assert per_frame[:, MASKED_PIXELS].tolist() == [0.0, float(masks[1].sum()), 0.0, 0.0] and per_frame[1, MASKED_PIXELS] > 0
    assert torch.isnan(per_frame[[0, 2, 3]][:, [MASKED_PSNR, MASKED_SSIM]]).all()
    assert out["psnr"] == pytest.approx(float(loop[:, PSNR].mean()), rel=1e-14)
    assert out["ssim"] == pytest.approx(float(loop[:, SSIM].mean()), rel=1e-14)
    assert out["masked_psnr"] == float(loop[1, MASKED_PSNR]) and out["masked_ssim"] == float(loop[1, MASKED_SSIM])
    assert np.isfinite([out[n] for n in mr.SCALARS]).all()
    bare = evaluate(pc, cams, gts, pipe, bg)
    assert bare["masked_psnr"] == -1 and bare["masked_ssim"] == -1 and bare["psnr"] == out["psnr"] and bare["ssim"] == out["ssim"]
    assert "lpips" not in bare
    split = evaluate(pc, cams[:2], gts[:2], pipe, bg, masks=masks[:2], return_decomposition=True)
    assert torch.equal(_bits(split["per_frame"]), _bits(loop[:2]))
