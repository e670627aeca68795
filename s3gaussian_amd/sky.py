"""Accumulated-opacity image and the sky-mask loss on it (include/s3g_alpha.h).  The reference loads a `sky_mask` per frame
(scene/dataset_readers.py:424-427, scene/cameras.py:66) and declares `opacities` / `sky_masks` video keys
(utils/video_utils.py:148-149, 461-471) that nothing fills, because its rasterizer returns no accumulated opacity.  Here the
opacity is one pass over the transmittance image the blend forward keeps anyway, and the loss

    mean( -(1 - s) log(a) - s log(1 - a) ),   a = clamp(A, 1e-6, 1 - 1e-6),   s = 1 on sky

is one pass over the opacity image that leaves its own gradient image behind.  GPU only, no CPU fallback."""
from __future__ import annotations

import torch

from . import _lib
from . import raster_C as _C


def _gpu(t, name: str) -> None:
    if not (torch.is_tensor(t) and t.is_cuda):
        where = t.device if torch.is_tensor(t) else type(t).__name__
        raise RuntimeError(f"{name} must live on the GPU (got {where}); the sky loss has no CPU fallback")


def opacity_image(image_buffer: torch.Tensor, image_height: int, image_width: int) -> torch.Tensor:
    """A = 1 - final transmittance, [1,H,W] fp32, of the rasterizer forward that filled `image_buffer` (the imgBuffer that
    raster_C.rasterize_gaussians returns).  No autograd: the differentiable route is GaussianRasterizer.forward_alpha."""
    _gpu(image_buffer, "image_buffer")
    return _C.raster_alpha(image_buffer, image_height, image_width)


def _plane(t: torch.Tensor, name: str, dev=None) -> torch.Tensor:
    """[H,W] or [1,H,W] -> contiguous fp32 [H,W] on the device."""
    if t.dim() == 3 and t.shape[0] == 1:
        t = t[0]
    if t.dim() != 2:
        raise RuntimeError(f"{name} must have shape [H,W] or [1,H,W], got {tuple(t.shape)}")
    if dev is not None:
        t = t.to(dev)
    return t.detach().float().contiguous()


def sky_loss_raw(alpha: torch.Tensor, sky_mask: torch.Tensor, weight: float = 1.0, slot: int = 0, total: torch.Tensor = None):
    """One s3g_sky_loss call, no autograd.  alpha: the opacity image [H,W] / [1,H,W].
    -> (loss fp32 [1], d loss / d A fp32 [H,W], total float64 [1]).  slot > 0 adds this view's weighted loss to `total` (the
    tensor an earlier call returned) instead of starting it."""
    _gpu(alpha, "alpha")
    a = _plane(alpha, "alpha")
    H, W = a.shape
    dev = a.device
    m = _plane(sky_mask, "sky_mask", dev)
    if m.shape != a.shape:
        raise RuntimeError(f"sky_mask {tuple(m.shape)} does not match the {H} x {W} image")
    if slot > 0 and total is None:
        raise RuntimeError("sky_loss_raw: slot > 0 adds to the `total` of the earlier slots")
    L = _lib.lib()
    if total is None:
        total = torch.empty(1, dtype=torch.float64, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    grad = torch.empty((H, W), dtype=torch.float32, device=dev)
    work = torch.empty(max(int(L.s3g_sky_loss_workspace_bytes(W, H)), 1), dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        _lib.check(L.s3g_sky_loss(W, H, a.data_ptr(), m.data_ptr(), float(weight), int(slot), grad.data_ptr(), total.data_ptr(),
                                  loss.data_ptr(), work.data_ptr(), _lib.stream_ptr()))
    return loss, grad, total


class _SkyLoss(torch.autograd.Function):
    """weight * mean over V*H*W of the sky cross entropy of V opacity images: one pass per view, which also leaves the view's
    gradient image; the backward scales those images by the upstream scalar on the device."""

    @staticmethod
    def forward(ctx, weight, masks, *alphas):
        V = len(alphas)
        total, grads = None, []
        for v, (a, m) in enumerate(zip(alphas, masks)):
            loss, g, total = sky_loss_raw(a, m, weight / V, slot=v, total=total)
            grads.append(g)
        ctx.save_for_backward(*grads)
        ctx.shapes = [tuple(a.shape) for a in alphas]
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        return (None, None, *((gi * g).reshape(sh) for gi, sh in zip(ctx.saved_tensors, ctx.shapes)))


def sky_opacity_loss(alpha_source, sky_mask, weight: float = 1.0) -> torch.Tensor:
    """weight * mean( -(1 - s) log(a) - s log(1 - a) ) with a = clamp(alpha, 1e-6, 1 - 1e-6): binary cross entropy of the
    accumulated opacity against `1 - sky_mask` (sky pixels should stay transparent).
    alpha_source: an opacity image [1,H,W] / [H,W] (the `alpha` of GaussianRasterizer.forward_alpha, out["alpha"] of
    pipeline.render(return_alpha=True)), or a result dict carrying one under "alpha"; or a sequence of V of those with a
    sequence of V masks: the mean then runs over V*H*W, every view weighted 1/V.
    sky_mask: [H,W] or [1,H,W], values in [0,1] (1 = sky; soft values from a bilinear resize are fine).
    -> 0-dim fp32 tensor on the device, differentiable w.r.t. the opacity images.  Nothing waits for the device."""
    many = isinstance(alpha_source, (list, tuple))
    sources = list(alpha_source) if many else [alpha_source]
    masks = list(sky_mask) if many else [sky_mask]
    if len(sources) == 0 or len(sources) != len(masks):
        raise RuntimeError("sky_opacity_loss: one sky mask per opacity image")
    alphas = [s["alpha"] if isinstance(s, dict) else s for s in sources]
    for a in alphas:
        _gpu(a, "alpha")
    return _SkyLoss.apply(float(weight), tuple(masks), *alphas)
