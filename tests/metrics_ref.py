"""Pure-numpy restatement of the four numbers the reference's evaluation loop reports per frame (utils/video_utils.py:210-241), in a
selectable dtype: the checker of s3gaussian_amd.metrics on a machine that has neither the reference tree nor scikit-image.

  psnr          utils/image_utils.py:17-19 per channel, then the mean over the channels
  ssim          scikit-image's structural_similarity(data_range=1.0, channel_axis=0) with its defaults: 7x7 uniform window, borders of
                scipy.ndimage.uniform_filter(mode='reflect') = np.pad(mode='symmetric'), sample covariance (49/48), C1 = 0.01^2,
                C2 = 0.03^2, mean over the interior [3:H-3, 3:W-3]
  masked_*      the same psnr over the masked pixels; the mean of the UNCROPPED map S over the masked pixels and channels

Every box mean is the exact 7x7 window, and is rounded to `dtype` ONCE: the 49 shifted slices of the padded image (whose products
a * a, a * b, b * b are formed in `dtype`) are added and divided by 49 in float64, as scipy's uniform_filter accumulates a float32 image in
double; everything after the box means is `dtype` arithmetic in scikit-image's order.  In float32 this is scikit-image's arithmetic for a
float32 image up to the order of the additions; |S_fp32 - S_fp64| of it is the yardstick of the per-pixel tolerance.
`variant` switches ONE step to a plausible wrong reading (tests/test_metrics_cpu.py shows that each moves a scalar far beyond the bars
the GPU tests use, so passing those tests rules them out)."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "eval_metrics.npz")
SHAPES = ((7, 7), (9, 23), (37, 53), (64, 96), (70, 100))
WIN, R = 7, 3
VARIANTS = ("zero_pad", "torch_reflect", "population_cov", "uncropped_ssim", "cropped_masked_ssim", "pooled_psnr")
PSNR_BAR = 1e-5     # dB, against the float64 evaluation
MAP_BAR_FACTOR = 8  # x the fixture's measured |S_fp32 - S_fp64| spread of this restatement


def box_mean(x, dtype, pad_mode="symmetric"):
    """x [C,H,W] in dtype -> 7x7 window means [C,H,W], accumulated in float64 and rounded to dtype once."""
    x = np.asarray(x, dtype)
    p = np.pad(x, ((0, 0), (R, R), (R, R)), mode=pad_mode).astype(np.float64)
    H, W = x.shape[1:]
    s = np.zeros(x.shape, np.float64)
    for dy in range(WIN):
        for dx in range(WIN):
            s = s + p[:, dy:dy + H, dx:dx + W]
    return (s / float(WIN * WIN)).astype(dtype)


def ssim_map(image, gt, dtype=np.float64, variant=None):
    """The full map S [3,H,W] of structural_similarity for channel-first images in [0,1]."""
    a, b = np.asarray(image, dtype), np.asarray(gt, dtype)
    pad = {"zero_pad": "constant", "torch_reflect": "reflect"}.get(variant, "symmetric")
    ux, uy = box_mean(a, dtype, pad), box_mean(b, dtype, pad)
    uxx, uyy, uxy = box_mean(a * a, dtype, pad), box_mean(b * b, dtype, pad), box_mean(a * b, dtype, pad)
    cov_norm = dtype(1.0) if variant == "population_cov" else dtype(49.0 / 48.0)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    C1, C2 = dtype(0.01 ** 2), dtype(0.03 ** 2)
    A1, A2, B1, B2 = dtype(2) * ux * uy + C1, dtype(2) * vxy + C2, ux * ux + uy * uy + C1, vx + vy + C2
    return ((A1 * A2) / (B1 * B2)).astype(dtype)


def psnr(a, b, dtype=np.float64, pooled=False):
    """a, b [3,N] (or [3,H,W]): mean over the channels of 20 log10(1 / sqrt(mse_c)); pooled=True is the wrong single-MSE form."""
    a, b = np.asarray(a, dtype).reshape(3, -1), np.asarray(b, dtype).reshape(3, -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        sq = (a - b) ** 2
        mse = sq.mean(dtype=dtype) if pooled else sq.mean(axis=1, dtype=dtype)
        return float(np.mean(dtype(20) * np.log10(dtype(1) / np.sqrt(mse)), dtype=np.float64))


def image_metrics(image, gt, mask=None, dtype=np.float64, variant=None):
    """-> dict(psnr, ssim, masked_psnr, masked_ssim, masked_pixels, map).  image, gt [3,H,W]; mask [H,W] (anything non-zero is set) or
    None.  An empty or absent mask gives NaN in the masked pair and 0 pixels."""
    image, gt = np.asarray(image), np.asarray(gt)
    H, W = image.shape[1:]
    assert image.shape == gt.shape == (3, H, W) and H >= WIN and W >= WIN
    S = ssim_map(image, gt, dtype, variant)
    m = np.zeros((H, W), bool) if mask is None else (np.asarray(mask).reshape(H, W) != 0)
    pooled = variant == "pooled_psnr"
    out = {"psnr": psnr(image, gt, dtype, pooled), "map": S, "masked_pixels": int(m.sum()),
           "ssim": float((S if variant == "uncropped_ssim" else S[:, R:H - R, R:W - R]).mean(dtype=np.float64))}
    if m.any():
        out["masked_psnr"] = psnr(image[:, m], gt[:, m], dtype, pooled)
        with np.errstate(invalid="ignore"):
            out["masked_ssim"] = (float(S[:, R:H - R, R:W - R][:, m[R:H - R, R:W - R]].mean(dtype=np.float64))
                                  if variant == "cropped_masked_ssim" else float(S[:, m].mean(dtype=np.float64)))
    else:
        out["masked_psnr"] = out["masked_ssim"] = float("nan")
    return out


SCALARS = ("psnr", "ssim", "masked_psnr", "masked_ssim")


def load_fixture():
    """tests/golden/eval_metrics.npz -> (cases, map_spread).  A case: image [3,H,W] fp32, gt [3,H,W] fp32 (stored as bytes, k / 255),
    mask [H,W] uint8, and the recorded reference values (see tests/golden/make_golden_metrics.py)."""
    z = np.load(FIXTURE)
    cases = []
    for k in range(len(SHAPES)):
        g = lambda name: z[f"c{k}_{name}"]
        cases.append({"image": g("image"), "gt": g("gt_u8").astype(np.float32) / np.float32(255.0), "mask": g("mask"),
                      "psnr_ref": float(g("psnr_ref")), "masked_psnr_ref": float(g("masked_psnr_ref")),
                      "psnr_ref_err": float(g("psnr_ref_err")), "masked_psnr_ref_err": float(g("masked_psnr_ref_err")),
                      "ssim_scipy": float(g("ssim_scipy")), "masked_ssim_scipy": float(g("masked_ssim_scipy"))})
        assert cases[-1]["image"].shape[1:] == SHAPES[k]
    return cases, float(z["map_spread"])
