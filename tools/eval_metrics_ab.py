#!/usr/bin/env python
"""The four evaluation numbers of one frame: the native route (s3gaussian_amd/metrics.py: a tile kernel and a fixed-order reduction, no
host synchronisation) against the torch-op route a user had to write on the device before it existed -- the arithmetic of the
reference's evaluation loop (utils/video_utils.py:210-241: psnr, scikit-image's structural_similarity, their masked forms) restated on
torch ops: `F.avg_pool2d` over an edge-repeating ("symmetric") padded image for the five 7x7 box means, boolean gathers for the masked
pair, and one `.item()` per number as the reference's loop has.  (The reference itself copies the image to the host twice and runs
scikit-image on the CPU; that is not timed here.)

    python tools/eval_metrics_ab.py [--reps 30] [--warmup 5] [--out profiles/eval_metrics_ab.txt]

Frames of 640 x 960 and 1066 x 1600, a mask with about 20 % of the pixels set.  The two routes alternate; every call is bracketed by
events on the current stream (the torch route's four host reads fall inside its bracket: they are part of what it costs); medians over
the repetitions.  The two routes' numbers are compared as well.  Exits non-zero if the native call is slower at either size."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = ((640, 960), (1066, 1600))


def symmetric_pad(x, r=3):
    """np.pad(mode='symmetric') on the last two axes: the edge pixel is repeated (torch's 'reflect' skips it)."""
    x = torch.cat([x[..., :r].flip(-1), x, x[..., -r:].flip(-1)], dim=-1)
    return torch.cat([x[..., :r, :].flip(-2), x, x[..., -r:, :].flip(-2)], dim=-2)


def torch_psnr(a, b):                                             # utils/image_utils.py:17-19
    mse = ((a - b) ** 2).view(a.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def torch_route(image, gt, mask):
    """-> [psnr, ssim, masked_psnr, masked_ssim]; mask: bool [H,W]."""
    out = [torch_psnr(image, gt).mean().double().item()]
    box = lambda t: F.avg_pool2d(symmetric_pad(t)[None], 7, stride=1)[0]
    ux, uy, uxx, uyy, uxy = box(image), box(gt), box(image * image), box(gt * gt), box(image * gt)
    cov_norm = 49.0 / 48.0
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
    out.append(S[:, 3:-3, 3:-3].mean().double().item())
    if mask.sum() > 0:                                            # video_utils.py:224 (a host read of its own)
        rgb_d, gt_d = image.permute(1, 2, 0)[mask].permute(1, 0), gt.permute(1, 2, 0)[mask].permute(1, 0)
        out.append(torch_psnr(rgb_d, gt_d).mean().double().item())
        out.append(S.permute(1, 2, 0)[mask].mean().double().item())
    return out


def make_frame(H, W, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    gt = torch.stack([0.5 + 0.3 * torch.sin(0.02 * x + c) * torch.cos(0.015 * y + 0.5 * c) for c in range(3)])
    gt = (gt + 0.03 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    image = (gt + 0.05 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    coarse = torch.rand(1, 1, (H + 31) // 32, (W + 31) // 32, generator=g) < 0.2          # 32 x 32 blocks, like object masks
    mask = F.interpolate(coarse.float(), scale_factor=32, mode="nearest")[0, 0, :H, :W] > 0
    return image.to(dev), gt.to(dev), mask.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_metrics_ab.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_metrics_ab.py measures on the GPU; there is none here (nothing measured)")
    from s3gaussian_amd.metrics import image_metrics
    dev = torch.device("cuda:0")
    lines = [f"# tools/eval_metrics_ab.py --reps {args.reps} --warmup {args.warmup}: PSNR, SSIM, masked PSNR, masked SSIM of one frame, native",
             f"# route vs torch-op route, alternated, events around every call, medians.  {torch.cuda.get_device_name(0)}"]
    slower = False
    for H, W in SIZES:
        image, gt, mask = make_frame(H, W, dev)
        record = torch.empty(5, dtype=torch.float64, device=dev)
        times = {"native": [], "torch": []}
        numbers = {}
        for rep in range(args.warmup + args.reps):
            for route in ("native", "torch"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                if route == "native":
                    image_metrics(image, gt, mask, out=record)
                else:
                    numbers["torch"] = torch_route(image, gt, mask)
                e1.record()
                torch.cuda.synchronize()
                if rep >= args.warmup:
                    times[route].append(e0.elapsed_time(e1))
        numbers["native"] = record.cpu().tolist()
        med = {k: statistics.median(v) for k, v in times.items()}
        lines.append(f"{H} x {W}, {int(numbers['native'][4])} masked pixels ({100.0 * numbers['native'][4] / (H * W):.1f} %)")
        for k in ("native", "torch"):
            v = times[k]
            lines.append(f"  {k:6s} ms per frame: median {med[k]:.4f}  min {min(v):.4f}  max {max(v):.4f}")
        lines.append(f"  torch / native (medians): {med['torch'] / med['native']:.1f} x")
        for i, name in enumerate(("psnr", "ssim", "masked_psnr", "masked_ssim")):
            lines.append(f"  {name:12s} native {numbers['native'][i]:.9f}  torch {numbers['torch'][i]:.9f}  "
                         f"difference {abs(numbers['native'][i] - numbers['torch'][i]):.2e}")
        slower = slower or med["native"] > med["torch"]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")
    if slower:
        raise SystemExit("the native call is SLOWER than the torch route")


if __name__ == "__main__":
    main()
