"""Loss kernels of the hot path on the MI355X.  `ssim(img1, img2)` has the signature and value of the reference's
utils/loss_utils.py::ssim (:66-96, window 11, size_average=True) for [C,H,W] or [1,C,H,W] images; the gradient flows
to img1 only (the rendered image), which is how train.py:416-418 uses it."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

_bound = False
SUM_DOUBLES = 64 * 16   # S3G_SUM_DOUBLES (include/s3g_loss.h): one slotted accumulator
# allocators of the kernels' outputs: every element is written, which the tests check by poisoning what these return
_new_grad = torch.empty_like
_new_maps = torch.empty


class _PlaneRegDesc(C.Structure):
    """struct s3g_plane_reg_desc (include/s3g_loss.h)."""
    _fields_ = [("plane", C.c_void_p), ("grad", C.c_void_p), ("H", C.c_int), ("W", C.c_int), ("w_smooth", C.c_float),
                ("w_l1", C.c_float)]


def _bind():
    global _bound
    L = _lib.lib()
    if not _bound:
        vp = C.c_void_p
        L.s3g_ssim_forward.restype = C.c_int
        L.s3g_ssim_forward.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp]
        L.s3g_ssim_backward.restype = C.c_int
        L.s3g_ssim_backward.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
        L.s3g_pixel_losses_forward.restype = C.c_int
        L.s3g_pixel_losses_forward.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.c_float, vp, vp]
        L.s3g_pixel_losses_combine.restype = C.c_int
        L.s3g_pixel_losses_combine.argtypes = [C.c_int, C.c_int, vp, vp, C.c_float, C.c_float, C.c_float, C.c_float, vp, vp]
        L.s3g_pixel_losses_combine_views.restype = C.c_int
        L.s3g_pixel_losses_combine_views.argtypes = [C.c_int] * 4 + [vp] * 2 + [C.c_float] * 4 + [vp] * 2
        L.s3g_pixel_losses_backward.restype = C.c_int
        L.s3g_pixel_losses_backward.argtypes = ([C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.c_float, vp, vp, C.c_float,
                                                 C.c_float, C.c_float, vp, C.c_int, vp, vp, vp])
        L.s3g_photometric_forward.restype = C.c_int
        L.s3g_photometric_forward.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.c_float, vp, vp, vp, vp, vp]
        L.s3g_photometric_backward.restype = C.c_int
        L.s3g_photometric_backward.argtypes = ([C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.c_float, vp, vp, vp, vp, vp,
                                                C.c_float, C.c_float, C.c_float, C.c_float, vp, vp, vp, vp])
        L.s3g_plane_regulation.restype = C.c_int
        L.s3g_plane_regulation.argtypes = [C.c_int, C.POINTER(_PlaneRegDesc), vp, vp]
        _bound = True
    return L


class _SSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img1, img2):
        if not img1.is_cuda:
            raise RuntimeError(f"ssim: images must live on the GPU (got {img1.device}); no CPU fallback")
        L = _bind()
        a = img1.detach().reshape(-1, img1.shape[-2], img1.shape[-1]).contiguous().float()
        b = img2.detach().reshape(-1, img2.shape[-2], img2.shape[-1]).contiguous().float()
        if a.shape != b.shape:
            raise RuntimeError("ssim: shape mismatch")
        Cn, H, W = a.shape
        total = torch.zeros(SUM_DOUBLES, dtype=torch.float64, device=a.device)
        maps = _new_maps((3, Cn, H, W), dtype=torch.float32, device=a.device)
        with _lib.on_device(a.device):
            _lib.check(L.s3g_ssim_forward(Cn, H, W, a.data_ptr(), b.data_ptr(), total.data_ptr(), maps[0].data_ptr(),
                                          maps[1].data_ptr(), maps[2].data_ptr(), _lib.stream_ptr()))
        ctx.save_for_backward(a, b, maps)
        ctx.shape = img1.shape
        return (total.sum() / float(Cn * H * W)).float()

    @staticmethod
    def backward(ctx, g):
        a, b, maps = ctx.saved_tensors
        L = _bind()
        Cn, H, W = a.shape
        g = g.detach().reshape(1).contiguous().float()
        out = _new_grad(a)
        with _lib.on_device(a.device):
            _lib.check(L.s3g_ssim_backward(Cn, H, W, a.data_ptr(), b.data_ptr(), maps[0].data_ptr(), maps[1].data_ptr(),
                                           maps[2].data_ptr(), g.data_ptr(), out.data_ptr(),
                                           _lib.stream_ptr()))
        return out.view(ctx.shape), None


def ssim(img1: torch.Tensor, img2: torch.Tensor, window_size: int = 11, size_average: bool = True) -> torch.Tensor:
    if window_size != 11 or not size_average:
        raise NotImplementedError("only the reference's call signature ssim(img1, img2) is accelerated")
    return _SSIM.apply(img1, img2)


class _PixelLoss(torch.autograd.Function):
    """The per-pixel terms of train.py:389-425 over the concatenated batch of V >= 1 views of one H x W, as ONE node:
        w_l1 * l1(images, gts) + w_depth * depth_l2(depths, gt_depths) + w_ssim * (1 - ssim(images, gts)) + w_feat * l2(feats, gt_feats)
    `flat` is the six lists images, gt_images, depths, gt_depths, feats, gt_feats one after the other, V entries each, None where a
    view has no such pair; the public functions below validate them and decide which pairs take part.  The images may be absent
    only when w_ssim == 0.  With an SSIM term: V fused strip-walking launches ADD into one set of accumulators, one 64-lane combine,
    V backward launches (include/s3g_loss.h::s3g_photometric_*); without it the pixel-loss entry points (s3g_pixel_losses_*).  L1
    and SSIM are means over V*3*H*W, the depth term over the batch's joint count of valid pixels, the feature term over the views
    that have one."""

    @staticmethod
    def forward(ctx, H, W, w_l1, w_ssim, w_depth, w_feat, max_depth, *flat):
        L = _bind()
        V = len(flat) // 6
        w_l1, w_ssim, w_depth, w_feat, max_depth = float(w_l1), float(w_ssim), float(w_depth), float(w_feat), float(max_depth)
        c = lambda t: None if t is None else t.detach().contiguous().float()
        views = [tuple(c(flat[k * V + v]) for k in range(6)) for v in range(V)]   # (img, gt, dep, gdep, ft, gft) per view
        dev = next(t for t in views[0] if t is not None).device
        has_image = views[0][0] is not None
        any_depth = any(vw[2] is not None for vw in views)
        n_feat = sum(1 for vw in views if vw[4] is not None)
        sums = torch.zeros(5 * SUM_DOUBLES + 5, dtype=torch.float64, device=dev)   # 5 accumulators + their 5 totals
        totals = sums[5 * SUM_DOUBLES:]
        maps = [_new_maps((3, 3, H, W), dtype=torch.float32, device=dev) for _ in range(V)] if w_ssim != 0.0 else None
        loss = torch.empty((), dtype=torch.float32, device=dev)
        p = lambda t: None if t is None else t.data_ptr()
        with _lib.on_device(dev):
            st = _lib.stream_ptr()
            for v, (img, gt, dep, gdep, ft, gft) in enumerate(views):
                if maps is not None:
                    m = maps[v]
                    _lib.check(L.s3g_photometric_forward(H, W, p(img), p(gt), p(dep), p(gdep), p(ft), p(gft), max_depth, p(sums),
                                                         p(m[0]), p(m[1]), p(m[2]), st))
                else:
                    _lib.check(L.s3g_pixel_losses_forward(H, W, p(img), p(gt), p(dep), p(gdep), p(ft), p(gft), max_depth,
                                                          p(sums), st))
            _lib.check(L.s3g_pixel_losses_combine_views(H, W, V, n_feat, p(sums), p(totals), w_l1 if has_image else 0.0,
                                                        w_depth if any_depth else 0.0, w_ssim, w_feat if n_feat else 0.0,
                                                        p(loss), st))
        ctx.save_for_backward(*(t for vw in views for t in vw if t is not None), *(maps or ()), totals)
        ctx.present = [[t is not None for t in vw] for vw in views]
        ctx.cfg = (H, W, n_feat, w_l1, w_ssim, w_depth, w_feat, max_depth)
        ctx.shapes = [None if t is None else t.shape for t in flat]
        return loss

    @staticmethod
    def backward(ctx, g):
        H, W, n_feat, w_l1, w_ssim, w_depth, w_feat, max_depth = ctx.cfg
        L = _bind()
        V = len(ctx.present)
        saved = iter(ctx.saved_tensors)
        views = [tuple(next(saved) if there else None for there in row) for row in ctx.present]
        maps = [next(saved) for _ in range(V)] if w_ssim != 0.0 else None
        totals = next(saved)
        g = g.detach().reshape(1).contiguous().float()
        # the kernels divide by this view's 3*H*W: the batch means take 1/V (1/n_feat) more.  The depth weight stays whole:
        # totals[3], which the kernels divide by, already is the joint count
        w_l1_v, w_ssim_v, w_feat_v = w_l1 / V, w_ssim / V, (w_feat / n_feat if n_feat else 0.0)
        need = ctx.needs_input_grad[7:]
        p = lambda t: None if t is None else t.data_ptr()
        grads = [None] * (6 * V)
        with _lib.on_device(totals.device):
            st = _lib.stream_ptr()
            for v, (img, gt, dep, gdep, ft, gft) in enumerate(views):
                # a gradient nobody asked for is not formed, except the image's on the SSIM route, whose entry point requires it
                g_img = _new_grad(img) if img is not None and (maps is not None or need[v]) else None
                g_dep = _new_grad(dep) if dep is not None and need[2 * V + v] else None
                g_ft = _new_grad(ft) if ft is not None and need[4 * V + v] else None
                if maps is not None:
                    m = maps[v]
                    _lib.check(L.s3g_photometric_backward(H, W, p(img), p(gt), p(dep), p(gdep), p(ft), p(gft), max_depth, p(m[0]),
                                                          p(m[1]), p(m[2]), p(totals), p(g), w_ssim_v, w_l1_v, w_depth, w_feat_v,
                                                          p(g_img), p(g_dep), p(g_ft), st))
                else:
                    _lib.check(L.s3g_pixel_losses_backward(H, W, p(img), p(gt), p(dep), p(gdep), p(ft), p(gft), max_depth, p(totals),
                                                           p(g), w_l1_v, w_depth, w_feat_v, p(g_img), 0, p(g_dep), p(g_ft), st))
                for k, t in ((0, g_img), (2, g_dep), (4, g_ft)):
                    if t is not None:
                        grads[k * V + v] = t.view(ctx.shapes[k * V + v])   # the caller's shape
        return (None,) * 7 + tuple(grads)


def _require_gpu(name, t):
    if not t.is_cuda:
        raise RuntimeError(f"{name}: images must live on the GPU (got {t.device}); no CPU fallback")


def _require_pairs(name, pairs):
    for what, a, b, n in pairs:
        if (a is None) != (b is None) or (a is not None and (a.numel() != n or b.numel() != n)):
            raise RuntimeError(f"{name}: {what} and its target must both be given, {n} elements each")


def _photometric(name, images, gt_images, depths, gt_depths, feats, gt_feats, w_ssim, w_depth, w_feat, max_depth):
    """photometric_loss / photometric_loss_views: [3,H,W] images of one size; a depth or feature pair takes part when its weight is
    not 0 and its prediction is there."""
    V = len(images)
    _require_gpu(name, images[0])
    w_depth, w_feat = float(w_depth), float(w_feat)
    depths, gt_depths, feats, gt_feats = list(depths), list(gt_depths), list(feats), list(gt_feats)
    for v, (img, gt) in enumerate(zip(images, gt_images)):
        if img.dim() != 3 or img.shape[0] != 3 or gt.shape != img.shape:
            raise RuntimeError(f"{name}: view {v}: image and gt_image must be [3,H,W] (got {tuple(img.shape)}, {tuple(gt.shape)})")
        if v == 0:
            _, H, W = img.shape
        elif tuple(img.shape[1:]) != (H, W):
            raise RuntimeError(f"{name}: view {v} is {img.shape[1]}x{img.shape[2]}, view 0 is {H}x{W}: all views of a batch must "
                               "have one size")
        if depths[v] is None or w_depth == 0.0:
            depths[v] = gt_depths[v] = None
        if feats[v] is None or w_feat == 0.0:
            feats[v] = gt_feats[v] = None
        _require_pairs(f"{name}: view {v}", (("depth", depths[v], gt_depths[v], H * W), ("feat", feats[v], gt_feats[v], 3 * H * W)))
    return _PixelLoss.apply(H, W, 1.0, w_ssim, w_depth, w_feat, max_depth, *images, *gt_images, *depths, *gt_depths, *feats,
                            *gt_feats)


def photometric_loss(image, gt_image, depth=None, gt_depth=None, feat=None, gt_feat=None, lambda_dssim=0.0,
                     lambda_depth=0.0, lambda_feat=0.0, max_depth=80.0):
    """The per-pixel part of train.py:395-425 for one view:
        l1_loss(image, gt_image) + lambda_depth * compute_depth("l2", depth, gt_depth)
        + lambda_dssim * (1 - ssim(image, gt_image)) + lambda_feat * l2_loss(feat, gt_feat)
    image/gt_image/feat/gt_feat [3,H,W], depth/gt_depth [1,H,W] or [H,W]; a zero weight (or a missing pair) skips a term."""
    return _photometric("photometric_loss", [image], [gt_image], [depth], [gt_depth], [feat], [gt_feat], lambda_dssim,
                        lambda_depth, lambda_feat, max_depth)


def photometric_loss_views(images, gt_images, depths=None, gt_depths=None, feats=None, gt_feats=None, lambda_dssim=0.0,
                           lambda_depth=0.0, lambda_feat=0.0, max_depth=80.0):
    """photometric_loss for a batch of V views of one H x W, with the reference's batch semantics (train.py:389-425 on the
    concatenated tensors), as ONE autograd node:
        l1_loss(cat(images), cat(gt_images)) + lambda_depth * compute_depth("l2", cat(depths), cat(gt_depths))
        + lambda_dssim * (1 - ssim(cat(images), cat(gt_images))) + lambda_feat * l2_loss(cat(feats'), cat(gt_feats'))
    L1 and SSIM are means over V*3*H*W elements; the depth term is the mean over the valid pixels of the WHOLE batch (one joint
    count, not the mean of per-view means); feats / gt_feats are lists with None for a view whose feature image is not
    supervised (the reference supervises the last view's only), the mean is over the views that have one."""
    V = len(images)
    if V < 1:
        raise RuntimeError("photometric_loss_views: no views")
    lists = [[None] * V if l is None else list(l) for l in (images, gt_images, depths, gt_depths, feats, gt_feats)]
    for name, l in zip(("images", "gt_images", "depths", "gt_depths", "feats", "gt_feats"), lists):
        if len(l) != V:
            raise RuntimeError(f"photometric_loss_views: {name} has {len(l)} entries for {V} views")
    return _photometric("photometric_loss_views", *lists, lambda_dssim, lambda_depth, lambda_feat, max_depth)


def pixel_terms(image=None, gt_image=None, depth=None, gt_depth=None, feat=None, gt_feat=None, w_l1=0.0, w_depth=0.0,
                w_feat=0.0, max_depth=80.0):
    """Any subset of: w_l1 * l1_loss(image, gt_image) [3,H,W]; w_depth * compute_depth("l2", depth, gt_depth) [1,H,W] or [H,W];
    w_feat * l2_loss(feat, gt_feat) [3,H,W]   (utils/loss_utils.py:21-54).  The zero-edit route (s3gaussian_amd.patch) calls it
    once per term, because train.py:395-425 adds them one function call at a time; photometric_loss above is the all-in-one form.
    H and W are the last two dims of the first tensor given; the others are checked by their element counts."""
    if image is None and depth is None and feat is None:
        raise RuntimeError("pixel_terms: nothing to do")
    first = next(t for t in (image, depth, feat) if t is not None)
    _require_gpu("pixel_terms", first)
    H, W = first.shape[-2], first.shape[-1]
    _require_pairs("pixel_terms", (("image", image, gt_image, 3 * H * W), ("depth", depth, gt_depth, H * W),
                                   ("feat", feat, gt_feat, 3 * H * W)))
    return _PixelLoss.apply(H, W, w_l1, 0.0, w_depth, w_feat, max_depth, image, gt_image, depth, gt_depth, feat, gt_feat)


def _plane_regulation_launch(planes, weights, grads):
    """Value of the regulariser over [1,32,H,W] channels_last `planes` with one (w_smooth, w_l1) per plane; the gradient of
    plane i is written into grads[i] (include/s3g_loss.h::s3g_plane_regulation)."""
    L = _bind()
    dev = planes[0].device
    if not planes[0].is_cuda:
        raise RuntimeError("plane regulation: planes must live on the GPU; no CPU fallback")
    descs = (_PlaneRegDesc * len(planes))()
    for i, (p, g, (ws, wl)) in enumerate(zip(planes, grads, weights)):
        if p.dim() != 4 or p.shape[1] != 32 or not p.is_contiguous(memory_format=torch.channels_last):
            raise RuntimeError("plane regulation expects [1,32,H,W] channels_last planes")
        if not g.is_contiguous(memory_format=torch.channels_last):
            raise RuntimeError("plane regulation: gradient views must be channels_last")
        descs[i] = _PlaneRegDesc(p.data_ptr(), g.data_ptr(), p.shape[2], p.shape[3], ws, wl)
    value = torch.zeros(SUM_DOUBLES, dtype=torch.float64, device=dev)
    with _lib.on_device(dev):
        _lib.check(L.s3g_plane_regulation(len(planes), descs, value.data_ptr(), _lib.stream_ptr()))
    return value.sum().float()


class _PlaneRegulation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weights, *planes):
        ctx.grads = [torch.empty_like(p) for p in planes]  # preserves channels_last
        return _plane_regulation_launch(planes, weights, ctx.grads)

    @staticmethod
    def backward(ctx, g):
        grads = ctx.grads
        torch._foreach_mul_(grads, g)
        return (None, *grads)


def _plane_weights(n_planes, time_smoothness_weight, l1_time_planes_weight, plane_tv_weight):
    return [(float(time_smoothness_weight), float(l1_time_planes_weight)) if i % 6 in (2, 4, 5) else (float(plane_tv_weight), 0.0)
            for i in range(n_planes)]


def plane_regulation_into(planes, reg_weights, grad_views):
    """Value of compute_regulation over `planes` (level-major list of the 6 planes per level) with the gradient written
    into the caller's channels_last views (no autograd here: s3gaussian_amd.hexplane folds it into the sampler's node).
    reg_weights = (time_smoothness_weight, l1_time_planes_weight, plane_tv_weight)."""
    return _plane_regulation_launch(planes, _plane_weights(len(planes), *reg_weights), grad_views)


def plane_regulation(grids, time_smoothness_weight, l1_time_planes_weight, plane_tv_weight):
    """GaussianModel.compute_regulation (scene/gaussian_model.py:748-749) over HexPlaneField.grids (6 planes per level), value
    and gradient in one fused pass."""
    planes = [p for level in grids for p in level]
    weights = _plane_weights(len(planes), time_smoothness_weight, l1_time_planes_weight, plane_tv_weight)
    return _PlaneRegulation.apply(tuple(weights), *planes)
