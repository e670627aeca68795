"""Generate tests/golden/eval_metrics.npz: inputs and reference values for the evaluation metrics (s3gaussian_amd/metrics.py).

    python tests/golden/make_golden_metrics.py        # rewrites eval_metrics.npz next to this file

Runs in the build container only: `psnr_ref` / `masked_psnr_ref` are recorded from the REFERENCE'S OWN utils/image_utils.py::psnr
(loaded from the reference tree, never copied), called the way utils/video_utils.py:211 and :225-231 call it -- `.mean().double()`
of the per-channel values, the masked form on the `permute(1, 2, 0)[mask].permute(1, 0)` gather.  Without the reference tree this
script refuses to run.

scikit-image is NOT installed in that container, so the SSIM entries are not scikit-image's output: they are its algorithm
(skimage/metrics/_structural_similarity.py: uniform_filter(size=7) of x, y, xx, yy, xy, sample covariance, C1, C2, crop(3).mean())
evaluated in float64 with scipy.ndimage.uniform_filter(mode='reflect') -- the very filter structural_similarity calls -- so the
border handling is scipy's, not a restatement of it.  tests/test_metrics_cpu.py ties tests/metrics_ref.py to this evaluation.

One case per shape of metrics_ref.SHAPES, chosen so that every wrong reading of the definition shows (asserted at the end):
  gt     a dark, slowly varying pattern (0.1 .. 0.3) plus a little noise, 8 bit like a stored photograph (kept as bytes, gt = k / 255
         in fp32), with a flat patch in the top-left corner.  Window variances are of the order of C2 = 0.03^2, where S is most
         sensitive to the covariance normalisation (49/48 against 1);
  image  gt + noise whose amplitude differs by channel (0.02, 0.035, 0.06: per-channel and pooled PSNR differ) and grows towards the
         borders (the interior mean and the whole-map mean of S differ), plus 0.15 on the top row and the left column (an edge
         artefact: padding that repeats the edge pixel and padding that skips it weigh it differently);
  mask   random, about 20 % set, always with the centre pixel.

Stored per case k: c{k}_image fp32, c{k}_gt_u8, c{k}_mask, c{k}_psnr_ref, c{k}_masked_psnr_ref (the reference's fp32 evaluation),
c{k}_psnr_ref_err, c{k}_masked_psnr_ref_err (|that - the float64 evaluation| on the same input), c{k}_ssim_scipy,
c{k}_masked_ssim_scipy.  `map_spread`: the largest |S_fp32 - S_fp64| of the restatement of tests/metrics_ref.py over all cases, the
yardstick of the per-pixel tolerance (8 x).  The generator asserts that every wrong variant of metrics_ref.VARIANTS moves a scalar by at
least 10 x the bars on every case."""
import importlib.util
import os
import sys

import numpy as np
import torch

REF = os.environ.get("S3G_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import metrics_ref as mr  # noqa: E402


def reference_psnr():
    path = os.path.join(REF, "utils", "image_utils.py")
    if not os.path.isfile(path):
        raise SystemExit(f"{path} is missing: the fixture records the reference's own psnr and cannot be written without it")
    spec = importlib.util.spec_from_file_location("_reference_image_utils", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.psnr


def make_case(H, W, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    gt = np.stack([0.2 + 0.1 * np.sin(0.05 * x + 1.3 * c) * np.cos(0.04 * y + 0.7 * c) for c in range(3)])
    gt = np.clip(gt + 0.005 * rng.standard_normal(gt.shape), 0.0, 1.0)
    ph, pw = max(3, H // 3), max(3, W // 3)
    gt[:, :ph, :pw] = 0.2
    gt_u8 = np.round(gt * 255.0).astype(np.uint8)
    gt32 = gt_u8.astype(np.float32) / np.float32(255.0)
    edge = np.maximum(np.abs(2 * y / (H - 1) - 1), np.abs(2 * x / (W - 1) - 1)) ** 2
    amp = np.array([0.02, 0.035, 0.06])[:, None, None] * (0.5 + 1.5 * edge)[None]
    image = gt32.astype(np.float64) + amp * rng.standard_normal(gt.shape)
    ring = np.zeros((H, W), bool)
    ring[0, :] = ring[:, 0] = True
    image[:, ring] += 0.15
    image = np.clip(image, 0.0, 1.0).astype(np.float32)
    mask = (rng.random((H, W)) < 0.2).astype(np.uint8)
    mask[H // 2, W // 2] = 1
    return image, gt_u8, gt32, mask


def scipy_evaluation(image, gt, mask):
    """structural_similarity's algorithm in float64 on scipy's own filter -> (ssim, masked_ssim, map)."""
    from scipy.ndimage import uniform_filter
    a, b = image.astype(np.float64), gt.astype(np.float64)
    f = lambda t: np.stack([uniform_filter(t[c], size=7, mode="reflect") for c in range(3)])
    ux, uy, uxx, uyy, uxy = f(a), f(b), f(a * a), f(b * b), f(a * b)
    cov_norm = 49.0 / 48.0
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
    H, W = a.shape[1:]
    return float(np.mean([S[c, 3:H - 3, 3:W - 3].mean() for c in range(3)])), float(S[:, mask != 0].mean()), S


def main():
    ref_psnr = reference_psnr()
    out, spread = {}, 0.0
    for k, (H, W) in enumerate(mr.SHAPES):
        image, gt_u8, gt, mask = make_case(H, W, seed=100 + k)
        m = mask.astype(bool)
        rgb, gt_rgb = torch.from_numpy(image), torch.from_numpy(gt)
        p = ref_psnr(rgb, gt_rgb).mean().double().item()                                       # video_utils.py:211
        rgb_d, gt_d = rgb.permute(1, 2, 0)[m].permute(1, 0), gt_rgb.permute(1, 2, 0)[m].permute(1, 0)   # :225-228
        pm = ref_psnr(rgb_d, gt_d).mean().double().item()                                      # :230-232
        r64, r32 = mr.image_metrics(image, gt, mask, np.float64), mr.image_metrics(image, gt, mask, np.float32)
        s, sm, smap = scipy_evaluation(image, gt, mask)
        assert np.abs(smap - r64["map"]).max() < 1e-10, np.abs(smap - r64["map"]).max()
        spread = max(spread, float(np.abs(r32["map"].astype(np.float64) - r64["map"]).max()))
        out.update({f"c{k}_image": image, f"c{k}_gt_u8": gt_u8, f"c{k}_mask": mask, f"c{k}_psnr_ref": p, f"c{k}_masked_psnr_ref": pm,
                    f"c{k}_psnr_ref_err": abs(p - r64["psnr"]), f"c{k}_masked_psnr_ref_err": abs(pm - r64["masked_psnr"]),
                    f"c{k}_ssim_scipy": s, f"c{k}_masked_ssim_scipy": sm})
        print(f"{H:3d} x {W:3d}: psnr {p:.6f} (fp64 {r64['psnr']:.6f}) masked {pm:.6f}; ssim {s:.6f} masked {sm:.6f}; "
              f"masked pixels {int(m.sum())}; |S_fp32 - S_fp64| max {np.abs(r32['map'].astype(np.float64) - r64['map']).max():.3e}")
    print(f"map_spread = {spread:.4e}  ->  per-pixel bar {mr.MAP_BAR_FACTOR * spread:.4e}")
    for k, (H, W) in enumerate(mr.SHAPES):            # every wrong variant is at least 10 bars away on every case
        image, gt, mask = out[f"c{k}_image"], out[f"c{k}_gt_u8"].astype(np.float32) / np.float32(255.0), out[f"c{k}_mask"]
        good = mr.image_metrics(image, gt, mask)
        for v in mr.VARIANTS:
            bad = mr.image_metrics(image, gt, mask, variant=v)
            moved = max(abs(bad[n] - good[n]) / (mr.PSNR_BAR if "psnr" in n else mr.MAP_BAR_FACTOR * spread) for n in mr.SCALARS)
            print(f"  {H:3d} x {W:3d} {v:20s} moves a scalar by {moved:10.1f} bars")
            assert moved >= 10.0, (H, W, v, moved)
    out["map_spread"] = np.float64(spread)
    np.savez_compressed(os.path.join(HERE, "eval_metrics.npz"), **out)
    print("wrote", os.path.join(HERE, "eval_metrics.npz"), os.path.getsize(os.path.join(HERE, "eval_metrics.npz")), "bytes")


if __name__ == "__main__":
    main()
