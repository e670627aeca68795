"""CPU-only: the checker of the evaluation metrics is itself checked, and the binding refuses what it must without a device.

tests/metrics_ref.py (pure numpy) is what tests/test_metrics_gpu.py compares the kernel with on a machine that has neither the
reference tree nor scikit-image.  Here it is tied to scipy's own uniform_filter (the filter scikit-image's structural_similarity calls),
to the reference's psnr values recorded in tests/golden/eval_metrics.npz, and shown to tell the definition apart from six plausible
misreadings of it by at least ten times the bars the GPU tests use."""
import os
import re

import numpy as np
import pytest
import torch

from tests import metrics_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fixture():
    return mr.load_fixture()


@pytest.fixture(scope="module")
def restated(fixture):
    cases, _ = fixture
    return [mr.image_metrics(c["image"], c["gt"], c["mask"], np.float64) for c in cases]


def test_restatement_equals_the_scipy_evaluation(fixture, restated):
    """structural_similarity's algorithm on scipy.ndimage.uniform_filter(mode='reflect') in float64, map and scalars, against the
    restatement (np.pad 'symmetric' + exact windows): <= 1e-10; the scalars the generator stored from the same evaluation too."""
    ndimage = pytest.importorskip("scipy.ndimage")
    cases, _ = fixture
    for c, r in zip(cases, restated):
        a, b = c["image"].astype(np.float64), c["gt"].astype(np.float64)
        H, W = a.shape[1:]
        f = lambda t: np.stack([ndimage.uniform_filter(t[k], size=7, mode="reflect") for k in range(3)])
        ux, uy, uxx, uyy, uxy = f(a), f(b), f(a * a), f(b * b), f(a * b)
        vx, vy, vxy = (49.0 / 48.0) * (uxx - ux * ux), (49.0 / 48.0) * (uyy - uy * uy), (49.0 / 48.0) * (uxy - ux * uy)
        S = ((2 * ux * uy + 0.01 ** 2) * (2 * vxy + 0.03 ** 2)) / ((ux ** 2 + uy ** 2 + 0.01 ** 2) * (vx + vy + 0.03 ** 2))
        assert np.abs(S - r["map"]).max() <= 1e-10, (H, W)
        assert abs(float(np.mean([S[k, 3:H - 3, 3:W - 3].mean() for k in range(3)])) - r["ssim"]) <= 1e-10
        assert abs(float(S[:, c["mask"] != 0].mean()) - r["masked_ssim"]) <= 1e-10
        assert abs(c["ssim_scipy"] - r["ssim"]) <= 1e-10 and abs(c["masked_ssim_scipy"] - r["masked_ssim"]) <= 1e-10


def test_restatement_reproduces_the_references_psnr(fixture, restated):
    """psnr_ref is the reference's own fp32 utils/image_utils.py::psnr on the fixture's inputs; psnr_ref_err its recorded distance from
    the float64 evaluation.  4.34 dB x the relative error of an MSE: an fp32 mean of at most 7000 squares is good to 2e-5 relative, so
    that distance stays below 1e-4 dB -- and the restatement, evaluated here, lands where the generator saw it."""
    cases, _ = fixture
    for c, r in zip(cases, restated):
        assert r["masked_pixels"] == int((c["mask"] != 0).sum()) > 0
        for name in ("psnr", "masked_psnr"):
            assert c[name + "_ref_err"] <= 1e-4, (name, c[name + "_ref_err"])
            assert abs(r[name] - c[name + "_ref"]) <= c[name + "_ref_err"] + 1e-9, (name, r[name], c[name + "_ref"])
            r32 = mr.image_metrics(c["image"], c["gt"], c["mask"], np.float32)
            assert abs(r32[name] - c[name + "_ref"]) <= 1e-4, (name, r32[name], c[name + "_ref"])


def test_recorded_map_spread_is_the_restatements_own(fixture, restated):
    """The per-pixel tolerance of the GPU tests is 8 x map_spread: the largest |S_fp32 - S_fp64| of the restatement over the cases."""
    cases, spread = fixture
    seen = max(float(np.abs(mr.ssim_map(c["image"], c["gt"], np.float32).astype(np.float64) - r["map"]).max())
               for c, r in zip(cases, restated))
    print(f"map_spread: recorded {spread:.4e}, evaluated here {seen:.4e}")
    assert 1e-6 < spread < 1e-4 and abs(seen - spread) <= 1e-9


def test_wrong_readings_of_the_definition_are_far_outside_the_bars(fixture, restated):
    """Zero padding, torch-style reflect padding, population covariance, an uncropped mean for ssim, a cropped mean for masked_ssim and
    the PSNR of the pooled MSE each move at least one scalar by >= 10 x its bar on EVERY fixture input."""
    cases, spread = fixture
    bar = lambda name: mr.PSNR_BAR if "psnr" in name else mr.MAP_BAR_FACTOR * spread
    for c, good in zip(cases, restated):
        for v in mr.VARIANTS:
            bad = mr.image_metrics(c["image"], c["gt"], c["mask"], np.float64, variant=v)
            moved = max(abs(bad[n] - good[n]) / bar(n) for n in mr.SCALARS)
            assert moved >= 10.0, (c["image"].shape, v, moved)


def test_empty_and_absent_masks_give_nan_in_the_restatement(fixture):
    c = fixture[0][1]
    for mask in (None, np.zeros_like(c["mask"])):
        r = mr.image_metrics(c["image"], c["gt"], mask)
        assert np.isnan(r["masked_psnr"]) and np.isnan(r["masked_ssim"]) and r["masked_pixels"] == 0


def test_image_metrics_has_no_cpu_fallback():
    from s3gaussian_amd.metrics import image_metrics
    x = torch.rand(3, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        image_metrics(x, x)


def test_record_layout_matches_the_header():
    from s3gaussian_amd import metrics
    txt = open(os.path.join(ROOT, "include", "s3g_metrics.h")).read()
    layout = dict(re.findall(r"#define S3G_METRICS_([A-Z_]+) (\d+)", txt))
    assert {k: int(v) for k, v in layout.items()} == {"PSNR": metrics.PSNR, "SSIM": metrics.SSIM, "MASKED_PSNR": metrics.MASKED_PSNR,
                                                      "MASKED_SSIM": metrics.MASKED_SSIM, "MASKED_PIXELS": metrics.MASKED_PIXELS,
                                                      "RECORD": metrics.RECORD}


def test_images_smaller_than_the_window_are_refused_before_any_device_call():
    """H = 6 or W = 6: return code 1 and a message, with NULL pointers and no GPU in the machine (scikit-image raises there too)."""
    from s3gaussian_amd import metrics
    L = metrics._bind()
    for H, W in ((6, 64), (64, 6), (6, 6)):
        assert L.s3g_image_metrics(H, W, None, None, None, None, None, None, None) == 1
        assert b"smaller than the 7 x 7" in L.s3g_last_error()
    assert L.s3g_image_metrics(7, 7, None, None, None, None, None, None, None) == 1 and b"NULL" in L.s3g_last_error()


def test_workspace_bytes_are_monotone():
    from s3gaussian_amd import metrics
    L = metrics._bind()
    sizes = (1, 6, 7, 8, 15, 16, 17, 31, 32, 33, 64, 100, 640, 1066, 1600, 4000)
    for fixed in (7, 640):
        over_h = [L.s3g_image_metrics_workspace_bytes(h, fixed) for h in sizes]
        over_w = [L.s3g_image_metrics_workspace_bytes(fixed, w) for w in sizes]
        assert over_h == sorted(over_h) and over_w == sorted(over_w) and over_h[0] > 0 and over_w[0] > 0
    assert L.s3g_image_metrics_workspace_bytes(1066, 1600) < L.s3g_image_metrics_workspace_bytes(2132, 1600)
