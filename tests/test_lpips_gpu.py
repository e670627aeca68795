"""GPU: s3gaussian_amd.lpips (csrc/lpips.hip) and pipeline.evaluate / evaluate_video with an LPIPS model, against the float64
restatement of tests/lpips_ref.py (which tests/test_lpips_cpu.py pins to the reference's own modules at 1e-12).

Sizes: the fixture's 31x31 (conv windows that are mostly padding, 1x1 deep layers), 35x47 and 67x93 (unused right and bottom columns
under stride 4, odd pool extents), 64x96, and 150x530, which is in no fixture: its layers are 36x131, 17x65 and 8x32, so every layer
spans several 128-pixel tiles and ends in a partial one.  Weights: lpips_ref.synthetic_weights(7); no test has seen the real ones.

Bar (nothing here is derived from what the kernel gives): computed on the CPU by lpips_ref.float32_route_errors -- the relative error
of the float32 restatement against the float64 one for every case and tap; the bar for every GPU tap value and total is 4 x the
largest of those (the 4 covers a different K summation order).  Measured here: float32 route 1.9e-8 .. 2.1e-6 per tap, bar 8.3e-6;
tap values 2.4e-3 .. 1.3e-2, totals 0.027 .. 0.039."""
import numpy as np
import pytest
import torch

from tests import lpips_ref as lr

pytestmark = pytest.mark.gpu

IDS = [f"{h}x{w}" for h, w in lr.FIXTURE_SIZES + (lr.EXTRA_SIZE,)]


@pytest.fixture(scope="module")
def ref():
    """Weights, the five image pairs, their float64 tap values and the bar: computed once on the CPU and only read afterwards."""
    weights = lr.synthetic_weights(lr.WEIGHT_SEED)
    cases = lr.all_cases()
    ref64, rel, bar = lr.float32_route_errors(weights, cases)
    return weights, cases, ref64, rel, bar


@pytest.fixture(scope="module")
def model(gpu_device, ref):
    from s3gaussian_amd.lpips import LPIPS
    return LPIPS.from_state_dicts(lr.alexnet_state_dict(ref[0]), lr.lin_state_dict(ref[0], upstream=True), gpu_device)


def _dev(case, dev):
    return torch.from_numpy(case[2]).to(dev), torch.from_numpy(case[3]).to(dev)


def _bits(t):
    return t.contiguous().view(torch.int64)


@pytest.mark.parametrize("k", range(5), ids=IDS)
def test_taps_and_total_match_the_float64_restatement(gpu_device, ref, model, k):
    from s3gaussian_amd.lpips import RECORD, TAP0, TOTAL, lpips
    _, cases, ref64, rel, bar = ref
    x, y = _dev(cases[k], gpu_device)
    rec = lpips(model, x, y)
    assert rec.shape == (RECORD,) and rec.dtype == torch.float64 and rec.is_cuda
    got = rec.cpu().numpy()
    err = np.abs(got[TAP0:] - ref64[k]) / ref64[k]
    total_err = abs(got[TOTAL] - ref64[k].sum()) / ref64[k].sum()
    print(f"{IDS[k]}: taps {got[TAP0:]} rel err {err} total {got[TOTAL]:.9g} rel err {total_err:.2e}; float32 route "
          f"{rel[k].max():.2e}, bar {bar:.2e}")
    assert np.isfinite(got).all()
    assert err.max() <= bar and total_err <= bar
    assert got[TOTAL] == (((got[1] + got[2]) + got[3]) + got[4]) + got[5]


@pytest.mark.parametrize("upstream", (True, False), ids=("upstream_keys", "renamed_keys"))
def test_recorded_reference_values_and_both_key_schemes(gpu_device, ref, model, upstream):
    """The reference's own recorded fp32 and float64 values of the four fixture cases; a model packed from the renamed lin keys gives
    the same bits as one packed from the upstream names."""
    from s3gaussian_amd.lpips import LPIPS, TOTAL, lpips
    weights, cases, _, _, bar = ref
    other = LPIPS.from_state_dicts(lr.alexnet_state_dict(weights), lr.lin_state_dict(weights, upstream=upstream), gpu_device)
    assert torch.equal(other.packed, model.packed)
    for k, c in enumerate(lr.load_fixture()):
        x, y = _dev(cases[k], gpu_device)
        got = float(lpips(other, x, y)[TOTAL])
        # the recorded fp32 value lies within one bar of the float64 one (test_lpips_cpu.py), the GPU value within another
        assert abs(got - c["ref_f64"]) <= bar * c["ref_f64"] and abs(got - c["ref_f32"]) <= 2 * bar * c["ref_f32"]


@pytest.mark.parametrize("k", range(5), ids=IDS)
def test_identical_images_give_exact_zero_and_the_slots_commute(gpu_device, ref, model, k):
    from s3gaussian_amd.lpips import lpips
    x, y = _dev(ref[1][k], gpu_device)
    same = lpips(model, x, x.clone())
    assert torch.equal(same, torch.zeros(6, dtype=torch.float64, device=gpu_device))
    xy, yx = lpips(model, x, y), lpips(model, y, x)
    assert float(xy[0]) > 0 and torch.equal(_bits(xy), _bits(yx))


@pytest.mark.parametrize("k", (2, 4), ids=(IDS[2], IDS[4]))
def test_two_runs_are_bit_identical(gpu_device, ref, model, k):
    from s3gaussian_amd.lpips import lpips
    x, y = _dev(ref[1][k], gpu_device)
    a = lpips(model, x, y)
    b = lpips(model, x, y)
    assert torch.equal(_bits(a), _bits(b))


def test_strides_do_not_change_a_bit_and_out_is_the_only_row_written(gpu_device, ref, model):
    from s3gaussian_amd.lpips import lpips
    x, y = _dev(ref[1][1], gpu_device)
    base = lpips(model, x, y)
    hwc_x, hwc_y = x.permute(1, 2, 0).contiguous().permute(2, 0, 1), y.permute(1, 2, 0).contiguous().permute(2, 0, 1)
    assert not hwc_x.is_contiguous() and torch.equal(hwc_x, x)
    assert torch.equal(_bits(lpips(model, hwc_x, hwc_y)), _bits(base))
    table = torch.full((4, 6), float("nan"), dtype=torch.float64, device=gpu_device)
    back = lpips(model, x, y, out=table[2])
    assert back.data_ptr() == table[2].data_ptr()
    assert torch.isnan(table[[0, 1, 3]]).all() and torch.equal(_bits(table[2]), _bits(base))
    with pytest.raises(RuntimeError, match="out must be"):
        lpips(model, x, y, out=table[:, 2])


def test_small_images_and_other_networks_are_refused(gpu_device, model):
    from s3gaussian_amd.lpips import LPIPS, lpips
    for shape in ((3, 30, 64), (3, 64, 30)):
        x = torch.rand(shape, device=gpu_device)
        with pytest.raises(Exception, match="smaller than 31 x 31"):
            lpips(model, x, x)
    x = torch.rand(3, 40, 40, device=gpu_device)
    with pytest.raises(NotImplementedError, match="vgg"):
        lpips(model, x, x, net_type="vgg")
    with pytest.raises(NotImplementedError, match="squeeze"):
        LPIPS(model.packed, net_type="squeeze")
    with pytest.raises(RuntimeError, match="GPU"):
        lpips(model, x.cpu(), x.cpu())


def test_evaluate_with_a_model_is_a_loop_of_render_and_lpips(gpu_device, model):
    """pipeline.evaluate(..., lpips=model) on the 64 x 96 four-camera scene of test_metrics_gpu.py: "lpips_per_frame" equals the plain
    loop of render + lpips bit for bit, "lpips" follows non_zero_mean (utils/video_utils.py:44-46), the five keys evaluate() has
    without a model keep their bits, and evaluate_video reports the same LPIPS bits on those cameras."""
    from types import SimpleNamespace
    from s3gaussian_amd import synth
    from s3gaussian_amd.lpips import TOTAL, lpips
    from s3gaussian_amd.pipeline import GaussianParams, default_hyper, evaluate, evaluate_video, render
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
    bare = evaluate(pc, cams, gts, pipe, bg, masks=masks)
    out = evaluate(pc, cams, gts, pipe, bg, masks=masks, lpips=model)
    assert set(bare) == {"psnr", "ssim", "masked_psnr", "masked_ssim", "per_frame"}
    assert set(out) == set(bare) | {"lpips", "lpips_per_frame"}
    for name in ("psnr", "ssim", "masked_psnr", "masked_ssim"):
        assert out[name] == bare[name]
    assert torch.equal(_bits(out["per_frame"]), _bits(bare["per_frame"]))
    with torch.no_grad():
        loop = torch.stack([lpips(model, render(cam, pc, pipe, bg, stage="fine")["render"], gt).cpu() for cam, gt in zip(cams, gts)])
    per_frame = out["lpips_per_frame"]
    assert per_frame.shape == (4, 6) and per_frame.dtype == torch.float64 and not per_frame.is_cuda
    assert torch.equal(_bits(per_frame), _bits(loop))
    assert (per_frame[:, TOTAL] > 0).all()
    assert out["lpips"] == float(loop[:, TOTAL].sum() / 4)
    video = evaluate_video(pc, cams, gts, pipe, bg, masks=masks, num_cams=2, keys=("rgbs",), lpips=model)
    assert video["lpips"] == out["lpips"] and torch.equal(_bits(video["lpips_per_frame"]), _bits(per_frame))
    assert video["psnr"] == bare["psnr"] and video["ssim"] == bare["ssim"]
    plain_video = evaluate_video(pc, cams[:2], gts[:2], pipe, bg, num_cams=2, keys=("rgbs",))
    assert "lpips" not in plain_video and "lpips_per_frame" not in plain_video
    with pytest.raises(RuntimeError, match="compute_metrics"):
        evaluate_video(pc, cams[:2], gts[:2], pipe, bg, num_cams=2, keys=("rgbs",), compute_metrics=False, lpips=model)
    with pytest.raises(TypeError, match="LPIPS model"):
        evaluate(pc, cams[:1], gts[:1], pipe, bg, lpips="alex")
