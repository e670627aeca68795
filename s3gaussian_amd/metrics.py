"""Evaluation metrics on the MI355X: what the reference's evaluation loop reports for one rendered frame
(utils/video_utils.py:210-241) -- `psnr(rgb, gt).mean()`, scikit-image's `structural_similarity(rgb, gt, data_range=1.0,
channel_axis=0)` and both under the camera's dynamic mask -- from one tile kernel and a fixed-order reduction
(include/s3g_metrics.h).  The training SSIM of losses.py (11x11 Gaussian window, zero padding) is a different function."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

PSNR, SSIM, MASKED_PSNR, MASKED_SSIM, MASKED_PIXELS = range(5)   # S3G_METRICS_* (include/s3g_metrics.h)
RECORD = 5

_bound = False


def _bind():
    global _bound
    L = _lib.lib()
    if not _bound:
        vp = C.c_void_p
        L.s3g_image_metrics_workspace_bytes.restype = C.c_size_t
        L.s3g_image_metrics_workspace_bytes.argtypes = [C.c_int, C.c_int]
        L.s3g_image_metrics.restype = C.c_int
        L.s3g_image_metrics.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp]
        _bound = True
    return L


def image_metrics(image: torch.Tensor, gt: torch.Tensor, mask=None, out=None, return_map: bool = False):
    """{psnr, ssim, masked_psnr, masked_ssim, masked_pixels} of one frame as a float64 device tensor of 5 entries.

    image, gt: [3,H,W] on the GPU, any strides (a permuted [H,W,3] view is fine), values in [0,1].
    mask: None, or [H,W] / [1,H,W]; bool and uint8 are taken as they are, any other dtype counts `> 0` as set.  Without a mask, or
    with an empty one, the two masked entries are NaN and masked_pixels is 0.
    out: a contiguous float64 tensor of 5 entries on the same device -- one row of an [N,5] tensor -- written in place and returned.
    return_map: also return scikit-image's full SSIM map S [3,H,W] (fp32).
    Nothing here waits for the device."""
    if not (torch.is_tensor(image) and image.is_cuda and torch.is_tensor(gt) and gt.is_cuda):
        where = image.device if torch.is_tensor(image) else type(image).__name__
        raise RuntimeError(f"image_metrics: images must live on the GPU (got {where}); no CPU fallback")
    if image.dim() != 3 or image.shape[0] != 3 or gt.shape != image.shape:
        raise RuntimeError("image_metrics expects image and gt of shape [3,H,W]")
    L = _bind()
    dev = image.device
    img, ref = image.detach().float().contiguous(), gt.detach().to(dev).float().contiguous()
    _, H, W = img.shape
    m = None
    if mask is not None:
        m = mask.detach().to(dev)
        if m.numel() != H * W:
            raise RuntimeError(f"image_metrics: the mask must have H*W = {H * W} elements")
        if m.dtype not in (torch.bool, torch.uint8):
            m = m > 0
        m = m.reshape(H, W).contiguous()
        if m.dtype == torch.bool:
            m = m.view(torch.uint8)
    if out is None:
        out = torch.empty(RECORD, dtype=torch.float64, device=dev)
    elif not (out.is_cuda and out.device == dev and out.dtype == torch.float64 and out.numel() == RECORD and out.is_contiguous()):
        raise RuntimeError("image_metrics: out must be a contiguous float64 tensor of 5 entries on the images' device")
    smap = torch.empty((3, H, W), dtype=torch.float32, device=dev) if return_map else None
    work = torch.empty(max(int(L.s3g_image_metrics_workspace_bytes(H, W)), 1), dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        _lib.check(L.s3g_image_metrics(H, W, img.data_ptr(), ref.data_ptr(), None if m is None else m.data_ptr(), out.data_ptr(),
                                       None if smap is None else smap.data_ptr(), work.data_ptr(), _lib.stream_ptr()))
    return (out, smap) if return_map else out
