"""GPU: s3gaussian_amd.lpips_vgg (csrc/lpips_vgg.hip) and pipeline.evaluate / evaluate_video with an LPIPSVGG model, against the
float64 restatement of tests/lpips_vgg_ref.py (which tests/test_lpips_vgg_cpu.py pins to the reference's own modules at 1e-12).

Sizes: the fixture's 16x16 (every window mostly padding, 1x1 fifth block), 17x23 and 40x52 (odd extents at every pool), and 150x210,
which is in no fixture: its blocks are 150x210, 75x105, 37x52, 18x26 and 9x13, so every block spans several 128-row tiles and ends
in a partial one, and every channel tiling of the conv kernel (co = 64, 128, 256, 512) runs with more than one workgroup.
Weights: lpips_vgg_ref.synthetic_weights(7); no test has seen the real ones.

Bar (nothing here is derived from what the kernel gives): computed on the CPU by lpips_vgg_ref.float32_route_errors -- the relative
error of two float32 restatements (F.conv2d; nine shifted 1x1 convolutions added in order) against the float64 one for every case
and tap; the bar for every GPU tap value and total is 4 x the largest of those.  Computed here: F.conv2d route 1.9e-9 .. 2.8e-6,
shifted route 1.9e-9 .. 4.0e-6, bar 1.6e-5; tap values 2.3e-4 .. 1.8e-2.  The routes' errors, and with them the bar, depend on the
summation order of the host's convolution library: on the MI355X host the F.conv2d route reaches 7.3e-6 (16x16, tap 5) and the bar
is 2.91e-5.  Measured there: every GPU tap within 6.2e-6 except that same tap -- one pixel, value 2.3e-4 -- at 1.93e-5: inside the
bar computed where the test ran, outside the 1.6e-5 computed where the fixture was generated.  The factor stays 4.  The measured
errors of the last run are written to profiles/lpips_vgg_errors.json."""
import json
import os

import numpy as np
import pytest
import torch

from tests import lpips_vgg_ref as lv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [f"{h}x{w}" for h, w in lv.FIXTURE_SIZES + (lv.EXTRA_SIZE,)]
MEASURED = {}


@pytest.fixture(scope="module")
def ref():
    """Weights, the four image pairs, their float64 tap values and the bar: computed once on the CPU and only read afterwards."""
    weights = lv.synthetic_weights(lv.WEIGHT_SEED)
    cases = lv.all_cases()
    ref64, rel, bar = lv.float32_route_errors()
    return weights, cases, ref64, rel, bar


@pytest.fixture(scope="module")
def model(gpu_device, ref):
    from s3gaussian_amd.lpips_vgg import LPIPSVGG
    return LPIPSVGG.from_state_dicts(lv.vgg_state_dict(ref[0]), lv.lin_state_dict(ref[0], upstream=True), gpu_device)


def _dev(case, dev):
    return torch.from_numpy(case[2]).to(dev), torch.from_numpy(case[3]).to(dev)


def _bits(t):
    return t.contiguous().view(torch.int64)


@pytest.mark.parametrize("k", range(4), ids=IDS)
def test_taps_and_total_match_the_float64_restatement(gpu_device, ref, model, k):
    from s3gaussian_amd.lpips_vgg import RECORD, TAP0, TOTAL, lpips_vgg
    _, cases, ref64, rel, bar = ref
    x, y = _dev(cases[k], gpu_device)
    rec = lpips_vgg(model, x, y)
    assert rec.shape == (RECORD,) and rec.dtype == torch.float64 and rec.is_cuda
    got = rec.cpu().numpy()
    err = np.abs(got[TAP0:] - ref64[k]) / ref64[k]
    total_err = abs(got[TOTAL] - ref64[k].sum()) / ref64[k].sum()
    print(f"{IDS[k]}: taps {got[TAP0:]} rel err {err} total {got[TOTAL]:.9g} rel err {total_err:.2e}; float32 routes "
          f"{rel[:, k].max():.2e}, bar {bar:.2e}")
    MEASURED[IDS[k]] = {"tap_rel_err": err.tolist(), "total_rel_err": float(total_err), "float32_routes_rel_err": rel[:, k].tolist(),
                        "bar": bar}
    if len(MEASURED) == 4:
        try:
            with open(os.path.join(ROOT, "profiles", "lpips_vgg_errors.json"), "w") as f:
                json.dump(MEASURED, f, indent=1)
                f.write("\n")
        except OSError:          # a read-only checkout: the record is a by-product, the assertions below are the test
            pass
    assert np.isfinite(got).all()
    assert err.max() <= bar and total_err <= bar
    assert got[TOTAL] == (((got[1] + got[2]) + got[3]) + got[4]) + got[5]


@pytest.mark.parametrize("upstream", (True, False), ids=("upstream_keys", "renamed_keys"))
def test_recorded_reference_values_and_both_key_schemes(gpu_device, ref, model, upstream):
    """The reference's own recorded fp32 and float64 values of the three fixture cases; a model packed from the renamed lin keys is
    the same blob as one packed from the upstream names."""
    from s3gaussian_amd.lpips_vgg import LPIPSVGG, TOTAL, lpips_vgg
    weights, cases, _, _, bar = ref
    other = LPIPSVGG.from_state_dicts(lv.vgg_state_dict(weights), lv.lin_state_dict(weights, upstream=upstream), gpu_device)
    assert torch.equal(other.packed, model.packed)
    for k, c in enumerate(lv.load_fixture()):
        x, y = _dev(cases[k], gpu_device)
        got = float(lpips_vgg(other, x, y)[TOTAL])
        # the recorded fp32 value lies within one bar of the float64 one (test_lpips_vgg_cpu.py), the GPU value within another
        assert abs(got - c["ref_f64"]) <= bar * c["ref_f64"] and abs(got - c["ref_f32"]) <= 2 * bar * c["ref_f32"]


@pytest.mark.parametrize("k", range(4), ids=IDS)
def test_identical_images_give_exact_zero_and_the_slots_commute(gpu_device, ref, model, k):
    from s3gaussian_amd.lpips_vgg import lpips_vgg
    x, y = _dev(ref[1][k], gpu_device)
    same = lpips_vgg(model, x, x.clone())
    assert torch.equal(same, torch.zeros(6, dtype=torch.float64, device=gpu_device))
    xy, yx = lpips_vgg(model, x, y), lpips_vgg(model, y, x)
    assert float(xy[0]) > 0 and torch.equal(_bits(xy), _bits(yx))


@pytest.mark.parametrize("k", (1, 3), ids=(IDS[1], IDS[3]))
def test_two_runs_are_bit_identical(gpu_device, ref, model, k):
    from s3gaussian_amd.lpips_vgg import lpips_vgg
    x, y = _dev(ref[1][k], gpu_device)
    a = lpips_vgg(model, x, y)
    b = lpips_vgg(model, x, y)
    assert torch.equal(_bits(a), _bits(b))


def test_strides_do_not_change_a_bit_and_out_is_the_only_row_written(gpu_device, ref, model):
    from s3gaussian_amd.lpips_vgg import lpips_vgg
    x, y = _dev(ref[1][1], gpu_device)
    base = lpips_vgg(model, x, y)
    hwc_x, hwc_y = x.permute(1, 2, 0).contiguous().permute(2, 0, 1), y.permute(1, 2, 0).contiguous().permute(2, 0, 1)
    assert not hwc_x.is_contiguous() and torch.equal(hwc_x, x)
    assert torch.equal(_bits(lpips_vgg(model, hwc_x, hwc_y)), _bits(base))
    table = torch.full((4, 6), float("nan"), dtype=torch.float64, device=gpu_device)
    back = lpips_vgg(model, x, y, out=table[2])
    assert back.data_ptr() == table[2].data_ptr()
    assert torch.isnan(table[[0, 1, 3]]).all() and torch.equal(_bits(table[2]), _bits(base))
    with pytest.raises(RuntimeError, match="out must be"):
        lpips_vgg(model, x, y, out=table[:, 2])


def test_small_images_and_cpu_tensors_are_refused(gpu_device, model):
    from s3gaussian_amd.lpips_vgg import lpips_vgg
    for shape in ((3, 15, 64), (3, 64, 15)):
        x = torch.rand(shape, device=gpu_device)
        with pytest.raises(Exception, match="smaller than 16 x 16"):
            lpips_vgg(model, x, x)
    x = torch.rand(3, 40, 40, device=gpu_device)
    with pytest.raises(RuntimeError, match="GPU"):
        lpips_vgg(model, x.cpu(), x.cpu())


def test_evaluate_dispatches_on_the_kind_of_model(gpu_device, ref, model):
    """pipeline.evaluate(..., lpips=vgg_model) on the 64 x 96 four-camera scene of test_lpips_gpu.py: "lpips_per_frame" equals the plain
    loop of render + lpips_vgg bit for bit, "lpips" follows non_zero_mean, evaluate_video reports the same bits, the other keys keep
    theirs; an AlexNet model still gives the bits of the plain render + lpips loop, under the same two keys and no new one."""
    from types import SimpleNamespace
    from s3gaussian_amd import synth
    from s3gaussian_amd.lpips import LPIPS, lpips
    from s3gaussian_amd.lpips_vgg import TOTAL, lpips_vgg
    from s3gaussian_amd.pipeline import GaussianParams, default_hyper, evaluate, evaluate_video, render
    from tests import lpips_ref as lr
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
    assert set(out) == set(bare) | {"lpips", "lpips_per_frame"}
    for name in ("psnr", "ssim", "masked_psnr", "masked_ssim"):
        assert out[name] == bare[name]
    assert torch.equal(_bits(out["per_frame"]), _bits(bare["per_frame"]))
    with torch.no_grad():
        renders = [render(cam, pc, pipe, bg, stage="fine")["render"] for cam in cams]
        loop = torch.stack([lpips_vgg(model, r, gt).cpu() for r, gt in zip(renders, gts)])
    per_frame = out["lpips_per_frame"]
    assert per_frame.shape == (4, 6) and per_frame.dtype == torch.float64 and not per_frame.is_cuda
    assert torch.equal(_bits(per_frame), _bits(loop))
    assert (per_frame[:, TOTAL] > 0).all()
    assert out["lpips"] == float(loop[:, TOTAL].sum() / 4)
    video = evaluate_video(pc, cams, gts, pipe, bg, masks=masks, num_cams=2, keys=("rgbs",), lpips=model)
    assert video["lpips"] == out["lpips"] and torch.equal(_bits(video["lpips_per_frame"]), _bits(per_frame))
    assert video["psnr"] == bare["psnr"] and video["ssim"] == bare["ssim"]
    # an AlexNet model: the same keys, its own bits
    w = lr.synthetic_weights(lr.WEIGHT_SEED)
    alex = LPIPS.from_state_dicts(lr.alexnet_state_dict(w), lr.lin_state_dict(w), dev)
    alex_out = evaluate(pc, cams, gts, pipe, bg, masks=masks, lpips=alex)
    assert set(alex_out) == set(out)
    alex_loop = torch.stack([lpips(alex, r, gt).cpu() for r, gt in zip(renders, gts)])
    assert torch.equal(_bits(alex_out["lpips_per_frame"]), _bits(alex_loop))
    assert not torch.equal(_bits(alex_out["lpips_per_frame"]), _bits(per_frame))
    with pytest.raises(TypeError, match="LPIPS model"):
        evaluate(pc, cams[:1], gts[:1], pipe, bg, lpips="vgg")
