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
        L.s3g_pixel_losses_backward.restype = C.c_int
        L.s3g_pixel_losses_backward.argtypes = ([C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.c_float, vp, vp, C.c_float,
                                                 C.c_float, C.c_float, vp, C.c_int, vp, vp, vp])
        L.s3g_photometric_forward.restype = C.c_int
        L.s3g_photometric_forward.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.c_float, vp, vp, vp, vp, vp]
        L.s3g_photometric_backward.restype = C.c_int
        L.s3g_photometric_backward.argtypes = ([C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, C.c_float, vp, vp, vp, vp, vp,
                                                C.c_float, C.c_float, C.c_float, C.c_float, vp, vp, vp, vp])
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


class _PhotometricLoss(torch.autograd.Function):
    """l1(image, gt) + w_depth * depth_l2 + w_ssim * (1 - ssim(image, gt)) + w_feat * l2(feat, gt_feat): with an SSIM term one
    fused launch plus the 64-lane combine forward and one launch backward (include/s3g_loss.h::s3g_photometric_*); without it
    the pixel-loss entry points."""

    @staticmethod
    def forward(ctx, image, gt_image, depth, gt_depth, feat, gt_feat, w_ssim, w_depth, w_feat, max_depth):
        if not image.is_cuda:
            raise RuntimeError(f"photometric_loss: images must live on the GPU (got {image.device}); no CPU fallback")
        L = _bind()
        c = lambda t: None if t is None else t.detach().contiguous().float()
        img, gt = c(image), c(gt_image)
        if img.dim() != 3 or img.shape[0] != 3 or gt.shape != img.shape:
            raise RuntimeError("photometric_loss expects image and gt_image of shape [3,H,W]")
        _, H, W = img.shape
        dev = img.device
        w_ssim, w_depth, w_feat = float(w_ssim), float(w_depth), float(w_feat)
        dep, gdep = (c(depth), c(gt_depth)) if (depth is not None and w_depth != 0.0) else (None, None)
        ft, gft = (c(feat), c(gt_feat)) if (feat is not None and w_feat != 0.0) else (None, None)
        for a, b, n in ((dep, gdep, H * W), (ft, gft, 3 * H * W)):
            if a is not None and (a.numel() != n or b.numel() != n):
                raise RuntimeError("photometric_loss: depth must have H*W and feat 3*H*W elements, like their targets")
        sums = torch.zeros(5 * SUM_DOUBLES + 5, dtype=torch.float64, device=dev)   # 5 accumulators + their 5 totals
        totals = sums[5 * SUM_DOUBLES:]
        maps = _new_maps((3, 3, H, W), dtype=torch.float32, device=dev) if w_ssim != 0.0 else None
        loss = torch.empty((), dtype=torch.float32, device=dev)
        p = lambda t: None if t is None else t.data_ptr()
        with _lib.on_device(dev):
            st = _lib.stream_ptr()
            if maps is not None:
                _lib.check(L.s3g_photometric_forward(H, W, p(img), p(gt), p(dep), p(gdep), p(ft), p(gft), float(max_depth),
                                                     p(sums), p(maps[0]), p(maps[1]), p(maps[2]), st))
            else:
                _lib.check(L.s3g_pixel_losses_forward(H, W, p(img), p(gt), p(dep), p(gdep), p(ft), p(gft), float(max_depth),
                                                      p(sums), st))
            _lib.check(L.s3g_pixel_losses_combine(H, W, p(sums), p(totals), 1.0, w_depth if dep is not None else 0.0, w_ssim,
                                                  w_feat if ft is not None else 0.0, p(loss), st))
        ctx.save_for_backward(img, gt, *(t for t in (dep, gdep, ft, gft, maps) if t is not None), totals)
        ctx.cfg = (H, W, dep is not None, ft is not None, maps is not None, w_ssim, w_depth, w_feat, float(max_depth),
                   None if depth is None else depth.shape, None if feat is None else feat.shape, image.shape)
        return loss

    @staticmethod
    def backward(ctx, g):
        H, W, has_d, has_f, has_s, w_ssim, w_depth, w_feat, max_depth, dshape, fshape, ishape = ctx.cfg
        saved = list(ctx.saved_tensors)
        img, gt = saved[0], saved[1]
        k = 2
        dep = gdep = ft = gft = maps = None
        if has_d:
            dep, gdep = saved[k], saved[k + 1]
            k += 2
        if has_f:
            ft, gft = saved[k], saved[k + 1]
            k += 2
        if has_s:
            maps = saved[k]
            k += 1
        sums = saved[k]
        L = _bind()
        dev = img.device
        g = g.detach().reshape(1).contiguous().float()
        g_img = _new_grad(img)
        g_dep = _new_grad(dep) if has_d else None
        g_ft = _new_grad(ft) if has_f else None
        p = lambda t: None if t is None else t.data_ptr()
        with _lib.on_device(dev):
            st = _lib.stream_ptr()
            if has_s:
                _lib.check(L.s3g_photometric_backward(H, W, p(img), p(gt), p(dep), p(gdep), p(ft), p(gft), max_depth, p(maps[0]),
                                                      p(maps[1]), p(maps[2]), p(sums), p(g), w_ssim, 1.0, w_depth, w_feat,
                                                      p(g_img), p(g_dep), p(g_ft), st))
            else:
                _lib.check(L.s3g_pixel_losses_backward(H, W, p(img), p(gt), p(dep), p(gdep), p(ft), p(gft), max_depth, p(sums),
                                                       p(g), 1.0, w_depth, w_feat, p(g_img), 0, p(g_dep), p(g_ft), st))
        return (g_img.view(ishape), None, g_dep.view(dshape) if has_d else None, None,
                g_ft.view(fshape) if has_f else None, None, None, None, None, None)


def photometric_loss(image, gt_image, depth=None, gt_depth=None, feat=None, gt_feat=None, lambda_dssim=0.0,
                     lambda_depth=0.0, lambda_feat=0.0, max_depth=80.0):
    """The per-pixel part of train.py:395-425 for one view:
        l1_loss(image, gt_image) + lambda_depth * compute_depth("l2", depth, gt_depth)
        + lambda_dssim * (1 - ssim(image, gt_image)) + lambda_feat * l2_loss(feat, gt_feat)
    image/gt_image/feat/gt_feat [3,H,W], depth/gt_depth [1,H,W] or [H,W]; a zero weight (or a missing pair) skips a term."""
    return _PhotometricLoss.apply(image, gt_image, depth, gt_depth, feat, gt_feat, lambda_dssim, lambda_depth, lambda_feat,
                                  max_depth)


class _PhotometricLossViews(torch.autograd.Function):
    """_PhotometricLoss over the concatenated batch of V views of one H x W (train.py:389-425): V forward launches ADD into one
    set of accumulators, one combine (include/s3g_loss.h::s3g_pixel_losses_combine_views), V backward launches.  L1 and SSIM are
    means over V*3*H*W, the depth term over the batch's joint count of valid pixels, the feature term over the views that have one."""

    @staticmethod
    def forward(ctx, V, w_ssim, w_depth, w_feat, max_depth, *flat):
        images, gts, depths, gt_depths, feats, gt_feats = (list(flat[k * V:(k + 1) * V]) for k in range(6))
        if not images[0].is_cuda:
            raise RuntimeError(f"photometric_loss_views: images must live on the GPU (got {images[0].device}); no CPU fallback")
        L = _bind()
        L.s3g_pixel_losses_combine_views.restype = C.c_int
        L.s3g_pixel_losses_combine_views.argtypes = ([C.c_int] * 4 + [C.c_void_p] * 2 + [C.c_float] * 4 + [C.c_void_p] * 2)
        c = lambda t: None if t is None else t.detach().contiguous().float()
        w_ssim, w_depth, w_feat, max_depth = float(w_ssim), float(w_depth), float(w_feat), float(max_depth)
        _, H, W = images[0].shape
        dev = images[0].device
        views = []
        for v in range(V):
            img, gt = c(images[v]), c(gts[v])
            if img.dim() != 3 or img.shape[0] != 3 or gt.shape != img.shape:
                raise RuntimeError(f"photometric_loss_views: view {v}: image and gt_image must be [3,H,W] (got {tuple(img.shape)}, "
                                   f"{tuple(gt.shape)})")
            if tuple(img.shape[1:]) != (H, W):
                raise RuntimeError(f"photometric_loss_views: view {v} is {img.shape[1]}x{img.shape[2]}, view 0 is {H}x{W}: "
                                   "all views of a batch must have one size")
            dep, gdep = (c(depths[v]), c(gt_depths[v])) if (depths[v] is not None and w_depth != 0.0) else (None, None)
            ft, gft = (c(feats[v]), c(gt_feats[v])) if (feats[v] is not None and w_feat != 0.0) else (None, None)
            for a, b, n in ((dep, gdep, H * W), (ft, gft, 3 * H * W)):
                if a is not None and (b is None or a.numel() != n or b.numel() != n):
                    raise RuntimeError(f"photometric_loss_views: view {v}: depth must have H*W and feat 3*H*W elements, like "
                                       "their targets")
            views.append((img, gt, dep, gdep, ft, gft))
        n_feat = sum(1 for vw in views if vw[4] is not None)
        any_depth = any(vw[2] is not None for vw in views)
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
            _lib.check(L.s3g_pixel_losses_combine_views(H, W, V, n_feat, p(sums), p(totals), 1.0, w_depth if any_depth else 0.0,
                                                        w_ssim, w_feat if n_feat else 0.0, p(loss), st))
        ctx.save_for_backward(*(t for vw in views for t in vw if t is not None), *(maps or ()), totals)
        ctx.present = [[t is not None for t in vw] for vw in views]
        ctx.cfg = (V, H, W, n_feat, w_ssim, w_depth, w_feat, max_depth)
        ctx.shapes = [tuple(None if t is None else t.shape for t in (images[v], depths[v], feats[v])) for v in range(V)]
        return loss

    @staticmethod
    def backward(ctx, g):
        V, H, W, n_feat, w_ssim, w_depth, w_feat, max_depth = ctx.cfg
        L = _bind()
        saved = iter(ctx.saved_tensors)
        views = [tuple(next(saved) if there else None for there in row) for row in ctx.present]
        maps = [next(saved) for _ in range(V)] if w_ssim != 0.0 else None
        totals = next(saved)
        g = g.detach().reshape(1).contiguous().float()
        # the kernels divide by this view's 3*H*W: the batch means take 1/V (1/n_feat) more.  The depth weight stays whole:
        # totals[3], which the kernels divide by, already is the joint count
        w_l1_v, w_ssim_v, w_feat_v = 1.0 / V, w_ssim / V, (w_feat / n_feat if n_feat else 0.0)
        p = lambda t: None if t is None else t.data_ptr()
        g_imgs, g_deps, g_fts = [], [], []
        with _lib.on_device(totals.device):
            st = _lib.stream_ptr()
            for v, (img, gt, dep, gdep, ft, gft) in enumerate(views):
                g_img = _new_grad(img)
                g_dep = _new_grad(dep) if dep is not None else None
                g_ft = _new_grad(ft) if ft is not None else None
                if maps is not None:
                    m = maps[v]
                    _lib.check(L.s3g_photometric_backward(H, W, p(img), p(gt), p(dep), p(gdep), p(ft), p(gft), max_depth, p(m[0]),
                                                          p(m[1]), p(m[2]), p(totals), p(g), w_ssim_v, w_l1_v, w_depth, w_feat_v,
                                                          p(g_img), p(g_dep), p(g_ft), st))
                else:
                    _lib.check(L.s3g_pixel_losses_backward(H, W, p(img), p(gt), p(dep), p(gdep), p(ft), p(gft), max_depth, p(totals),
                                                           p(g), w_l1_v, w_depth, w_feat_v, p(g_img), 0, p(g_dep), p(g_ft), st))
                ishape, dshape, fshape = ctx.shapes[v]
                g_imgs.append(g_img.view(ishape))
                g_deps.append(None if g_dep is None else g_dep.view(dshape))
                g_fts.append(None if g_ft is None else g_ft.view(fshape))
        none = [None] * V
        return (None, None, None, None, None, *g_imgs, *none, *g_deps, *none, *g_fts, *none)


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
    none = [None] * V
    lists = [list(images), list(gt_images), list(depths) if depths is not None else none,
             list(gt_depths) if gt_depths is not None else none, list(feats) if feats is not None else none,
             list(gt_feats) if gt_feats is not None else none]
    for name, l in zip(("images", "gt_images", "depths", "gt_depths", "feats", "gt_feats"), lists):
        if len(l) != V:
            raise RuntimeError(f"photometric_loss_views: {name} has {len(l)} entries for {V} views")
    flat = [t for l in lists for t in l]
    return _PhotometricLossViews.apply(V, lambda_dssim, lambda_depth, lambda_feat, max_depth, *flat)


class _PixelTerms(torch.autograd.Function):
    """w_l1 * l1(image, gt) + w_depth * depth_l2(depth, gt_depth) + w_feat * l2(feat, gt_feat) with any subset of the three
    pairs present: one kernel forward (+ the 64-lane combine), one backward (include/s3g_loss.h::s3g_pixel_losses_*).  The
    zero-edit route (s3gaussian_amd.patch) calls it once per term, because train.py:395-425 adds them one function call at a
    time; photometric_loss above is the all-in-one form."""

    @staticmethod
    def forward(ctx, image, gt_image, depth, gt_depth, feat, gt_feat, w_l1, w_depth, w_feat, max_depth):
        first = next(t for t in (image, depth, feat) if t is not None)
        if not first.is_cuda:
            raise RuntimeError(f"pixel_terms: images must live on the GPU (got {first.device}); no CPU fallback")
        L = _bind()
        c = lambda t: None if t is None else t.detach().contiguous().float()
        img, gt, dep, gdep, ft, gft = c(image), c(gt_image), c(depth), c(gt_depth), c(feat), c(gt_feat)
        H, W = first.shape[-2], first.shape[-1]
        for a, b, n, name in ((img, gt, 3 * H * W, "image"), (dep, gdep, H * W, "depth"), (ft, gft, 3 * H * W, "feat")):
            if (a is None) != (b is None) or (a is not None and (a.numel() != n or b.numel() != n)):
                raise RuntimeError(f"pixel_terms: {name} and its target must both be given, {n} elements each")
        dev = first.device
        sums = torch.zeros(5 * SUM_DOUBLES + 5, dtype=torch.float64, device=dev)
        totals = sums[5 * SUM_DOUBLES:]
        loss = torch.empty((), dtype=torch.float32, device=dev)
        p = lambda t: None if t is None else t.data_ptr()
        wl, wd, wf = (float(w_l1) if img is not None else 0.0, float(w_depth) if dep is not None else 0.0,
                      float(w_feat) if ft is not None else 0.0)
        with _lib.on_device(dev):
            st = _lib.stream_ptr()
            _lib.check(L.s3g_pixel_losses_forward(H, W, p(img), p(gt), p(dep), p(gdep), p(ft), p(gft), float(max_depth), p(sums), st))
            _lib.check(L.s3g_pixel_losses_combine(H, W, p(sums), p(totals), wl, wd, 0.0, wf, p(loss), st))
        ctx.save_for_backward(*(t for t in (img, gt, dep, gdep, ft, gft) if t is not None), totals)
        ctx.cfg = (H, W, img is not None, dep is not None, ft is not None, wl, wd, wf, float(max_depth),
                   None if image is None else image.shape, None if depth is None else depth.shape, None if feat is None else feat.shape)
        return loss

    @staticmethod
    def backward(ctx, g):
        H, W, has_i, has_d, has_f, wl, wd, wf, max_depth, ishape, dshape, fshape = ctx.cfg
        saved = list(ctx.saved_tensors)
        img = gt = dep = gdep = ft = gft = None
        k = 0
        if has_i:
            img, gt = saved[k], saved[k + 1]
            k += 2
        if has_d:
            dep, gdep = saved[k], saved[k + 1]
            k += 2
        if has_f:
            ft, gft = saved[k], saved[k + 1]
            k += 2
        totals = saved[k]
        L = _bind()
        g = g.detach().reshape(1).contiguous().float()
        need = ctx.needs_input_grad
        g_img = _new_grad(img) if (has_i and need[0]) else None
        g_dep = _new_grad(dep) if (has_d and need[2]) else None
        g_ft = _new_grad(ft) if (has_f and need[4]) else None
        p = lambda t: None if t is None else t.data_ptr()
        with _lib.on_device(totals.device):
            _lib.check(L.s3g_pixel_losses_backward(H, W, p(img), p(gt), p(dep), p(gdep), p(ft), p(gft), max_depth, p(totals), p(g),
                                                   wl, wd, wf, p(g_img), 0, p(g_dep), p(g_ft), _lib.stream_ptr()))
        return (None if g_img is None else g_img.view(ishape), None, None if g_dep is None else g_dep.view(dshape), None,
                None if g_ft is None else g_ft.view(fshape), None, None, None, None, None)


def pixel_terms(image=None, gt_image=None, depth=None, gt_depth=None, feat=None, gt_feat=None, w_l1=0.0, w_depth=0.0,
                w_feat=0.0, max_depth=80.0):
    """Any subset of: w_l1 * l1_loss(image, gt_image) [3,H,W]; w_depth * compute_depth("l2", depth, gt_depth) [1,H,W] or [H,W];
    w_feat * l2_loss(feat, gt_feat) [3,H,W]   (utils/loss_utils.py:21-54)."""
    if image is None and depth is None and feat is None:
        raise RuntimeError("pixel_terms: nothing to do")
    return _PixelTerms.apply(image, gt_image, depth, gt_depth, feat, gt_feat, w_l1, w_depth, w_feat, max_depth)


class _PlaneRegDesc(C.Structure):
    """struct s3g_plane_reg_desc (include/s3g_loss.h)."""
    _fields_ = [("plane", C.c_void_p), ("grad", C.c_void_p), ("H", C.c_int), ("W", C.c_int), ("w_smooth", C.c_float),
                ("w_l1", C.c_float)]


class _PlaneRegulation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, weights, *planes):
        L = _lib.lib()
        L.s3g_plane_regulation.restype = C.c_int
        L.s3g_plane_regulation.argtypes = [C.c_int, C.POINTER(_PlaneRegDesc), C.c_void_p, C.c_void_p]
        dev = planes[0].device
        if not planes[0].is_cuda:
            raise RuntimeError("plane regulation: planes must live on the GPU; no CPU fallback")
        grads = [torch.empty_like(p) for p in planes]  # preserves channels_last
        descs = (_PlaneRegDesc * len(planes))()
        for i, (p, g, (ws, wl)) in enumerate(zip(planes, grads, weights)):
            if p.dim() != 4 or p.shape[1] != 32 or not p.is_contiguous(memory_format=torch.channels_last):
                raise RuntimeError("plane regulation expects [1,32,H,W] channels_last planes")
            descs[i] = _PlaneRegDesc(p.data_ptr(), g.data_ptr(), p.shape[2], p.shape[3], ws, wl)
        value = torch.zeros(SUM_DOUBLES, dtype=torch.float64, device=dev)
        with _lib.on_device(dev):
            _lib.check(L.s3g_plane_regulation(len(planes), descs, value.data_ptr(), _lib.stream_ptr()))
        ctx.grads = grads
        return value.sum().float()

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
    L = _lib.lib()
    L.s3g_plane_regulation.restype = C.c_int
    L.s3g_plane_regulation.argtypes = [C.c_int, C.POINTER(_PlaneRegDesc), C.c_void_p, C.c_void_p]
    dev = planes[0].device
    weights = _plane_weights(len(planes), *reg_weights)
    descs = (_PlaneRegDesc * len(planes))()
    for i, (p, g, (ws, wl)) in enumerate(zip(planes, grad_views, weights)):
        if p.dim() != 4 or p.shape[1] != 32 or not p.is_contiguous(memory_format=torch.channels_last):
            raise RuntimeError("plane regulation expects [1,32,H,W] channels_last planes")
        if not g.is_contiguous(memory_format=torch.channels_last):
            raise RuntimeError("plane regulation: gradient views must be channels_last")
        descs[i] = _PlaneRegDesc(p.data_ptr(), g.data_ptr(), p.shape[2], p.shape[3], ws, wl)
    value = torch.zeros(SUM_DOUBLES, dtype=torch.float64, device=dev)
    with _lib.on_device(dev):
        _lib.check(L.s3g_plane_regulation(len(planes), descs, value.data_ptr(), _lib.stream_ptr()))
    return value.sum().float()


def plane_regulation(grids, time_smoothness_weight, l1_time_planes_weight, plane_tv_weight):
    """GaussianModel.compute_regulation (scene/gaussian_model.py:748-749) over HexPlaneField.grids, value and
    gradient in one fused pass."""
    planes, weights = [], []
    for level in grids:
        for i, p in enumerate(level):
            planes.append(p)
            weights.append((float(time_smoothness_weight), float(l1_time_planes_weight)) if i in (2, 4, 5)
                           else (float(plane_tv_weight), 0.0))
    return _PlaneRegulation.apply(tuple(weights), *planes)
