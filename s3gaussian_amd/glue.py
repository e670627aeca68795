"""Fused per-Gaussian render glue (activations + SH->RGB) on the MI355X; see include/s3g_glue.h."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

_bound = False


def _bind():
    global _bound
    L = _lib.lib()
    if not _bound:
        vp = C.c_void_p
        L.s3g_glue_forward.restype = C.c_int
        L.s3g_glue_forward.argtypes = [C.c_int, C.c_int] + [vp] * 14
        L.s3g_glue_backward.restype = C.c_int
        L.s3g_glue_backward.argtypes = [C.c_int, C.c_int] + [vp] * 23
        L.s3g_glue_forward_views.restype = C.c_int
        L.s3g_glue_forward_views.argtypes = [C.c_int, C.c_int, C.c_int] + [vp] * 14
        L.s3g_glue_backward_views.restype = C.c_int
        L.s3g_glue_backward_views.argtypes = [C.c_int, C.c_int, C.c_int] + [vp] * 23
        L.s3g_glue_backward_views_campos_workspace_bytes.restype = C.c_size_t
        L.s3g_glue_backward_views_campos_workspace_bytes.argtypes = [C.c_int, C.c_int]
        L.s3g_glue_backward_views_campos.restype = C.c_int
        L.s3g_glue_backward_views_campos.argtypes = [C.c_int, C.c_int, C.c_int] + [vp] * 26
        _bound = True
    return L


def _p(t):
    return None if t is None else t.data_ptr()


class _Glue(torch.autograd.Function):
    @staticmethod
    def forward(ctx, deg, f_dc, f_rest, dshs, xyz, campos, log_scales, rot_raw, opacity_logit, want_dshs_l1):
        if not xyz.is_cuda:
            raise RuntimeError(f"render glue: tensors must live on the GPU (got {xyz.device}); no CPU fallback")
        L = _bind()
        c = lambda t: None if t is None else t.detach().contiguous().float()
        f_dc, f_rest, dshs, xyz_c, campos_c = c(f_dc), c(f_rest), c(dshs), c(xyz), c(campos)
        ls, rr, ol = c(log_scales), c(rot_raw), c(opacity_logit)
        P, dev = xyz_c.shape[0], xyz_c.device
        if f_dc.shape != (P, 1, 3) or f_rest.shape != (P, 15, 3):
            raise RuntimeError("render glue expects f_dc [P,1,3] and f_rest [P,15,3] (sh_degree 3 storage)")
        colors = torch.empty((P, 3), dtype=torch.float32, device=dev)
        scales = torch.empty((P, 3), dtype=torch.float32, device=dev)
        rot = torch.empty((P, 4), dtype=torch.float32, device=dev)
        opac = torch.empty((P, 1), dtype=torch.float32, device=dev)
        asked_l1 = bool(want_dshs_l1)
        want_dshs_l1 = asked_l1 and dshs is not None and P > 0
        abs_sum = torch.zeros(64 * 16, dtype=torch.float64, device=dev) if want_dshs_l1 else None   # S3G_SUM_DOUBLES
        with _lib.on_device(dev):
            _lib.check(L.s3g_glue_forward(P, int(deg), _p(f_dc), _p(f_rest), _p(dshs), _p(xyz_c), _p(campos_c), _p(ls), _p(rr),
                                          _p(ol), _p(colors), _p(scales), _p(rot), _p(opac), _p(abs_sum),
                                          _lib.stream_ptr()))
        ctx.deg = int(deg)
        ctx.has_dshs = dshs is not None
        ctx.campos_shape = campos.shape
        ctx.save_for_backward(f_dc, f_rest, dshs if dshs is not None else torch.empty(0, device=dev), xyz_c, campos_c, rr,
                              colors, scales, rot, opac)
        ctx.want_dshs_l1 = want_dshs_l1
        if want_dshs_l1:
            dshs_l1 = (abs_sum.sum() / (48.0 * P)).float()
        elif asked_l1:
            dshs_l1 = torch.zeros((), dtype=torch.float32, device=dev)     # asked for, nothing to sum (no dshs / P == 0)
        else:
            dshs_l1 = torch.empty((), dtype=torch.float32, device=dev)     # not asked for: dropped by the wrapper, no fill launch
        return colors, scales, rot, opac, dshs_l1

    @staticmethod
    def backward(ctx, g_colors, g_scales, g_rot, g_opac, g_l1):
        f_dc, f_rest, dshs, xyz, campos, rr, colors, scales, rot, opac = ctx.saved_tensors
        L = _bind()
        P, dev = xyz.shape[0], xyz.device
        dshs = dshs if ctx.has_dshs else None
        c = lambda t: None if t is None else t.contiguous().float()
        g_colors, g_scales, g_rot, g_opac = c(g_colors), c(g_scales), c(g_rot), c(g_opac)
        e = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        g_f_dc, g_f_rest, g_xyz, g_ls, g_rr, g_ol = e(P, 1, 3), e(P, 15, 3), e(P, 3), e(P, 3), e(P, 4), e(P, 1)
        g_dshs = e(P, 16, 3) if ctx.has_dshs else None
        g_l1 = g_l1.contiguous().float() if (ctx.want_dshs_l1 and g_l1 is not None) else None
        with _lib.on_device(dev):
            _lib.check(L.s3g_glue_backward(P, ctx.deg, _p(f_dc), _p(f_rest), _p(dshs), _p(xyz), _p(campos), _p(rr), _p(colors),
                                           _p(scales), _p(rot), _p(opac), _p(g_colors), _p(g_scales), _p(g_rot), _p(g_opac),
                                           _p(g_f_dc), _p(g_f_rest), _p(g_dshs), _p(g_xyz), _p(g_ls), _p(g_rr), _p(g_ol), _p(g_l1),
                                           _lib.stream_ptr()))
        g_campos = None
        if ctx.needs_input_grad[5]:
            # the colours depend on xyz - campos only: dL/dcampos = -sum_p g_xyz[p], summed in double in a fixed order
            from . import raster_C
            g_campos = raster_C.camera_backward(P, dev, g_dir=g_xyz)[32:35].to(torch.float32).view(ctx.campos_shape)
        return None, g_f_dc, g_f_rest, g_dshs, g_xyz, g_campos, g_ls, g_rr, g_ol, None


def activations_and_colors(deg, f_dc, f_rest, dshs, xyz, campos, log_scales, rot_raw, opacity_logit, with_dshs_l1=False):
    """-> (colors_precomp [P,3], scales [P,3], rotations [P,4], opacity [P,1]); dshs may be None (coarse stage).
    with_dshs_l1=True appends mean|dshs| (the train.py:407-410 regulariser, differentiable) computed in the same pass."""
    out = _Glue.apply(deg, f_dc, f_rest, dshs, xyz, campos, log_scales, rot_raw, opacity_logit, with_dshs_l1)
    return out if with_dshs_l1 else out[:4]


MAX_VIEWS = 8   # S3G_GLUE_MAX_VIEWS (include/s3g_glue.h)


def _ptr_array(tensors):
    """Host array of device pointers (None -> NULL), as the *_views entry points take them."""
    return (C.c_void_p * len(tensors))(*[_p(t) for t in tensors])


class _GlueViews(torch.autograd.Function):
    """_Glue for V camera centres of one timestamp: outputs (colors_0 .. colors_{V-1}, scales, rot, opacity, dshs_l1).  Every
    view's colours are a tensor of their own: the rasterizer of view v hands back the gradient of colors_v and nothing is sliced
    out of or assembled into a [V,P,3] block.  campos_grad: the backward also returns the gradient of `campos` ([V,3]) when it
    requires one (s3g_glue_backward_views_campos); False launches what it always did."""

    @staticmethod
    def forward(ctx, deg, f_dc, f_rest, dshs, xyz, campos, log_scales, rot_raw, opacity_logit, want_dshs_l1, campos_grad=False):
        if not xyz.is_cuda:
            raise RuntimeError(f"render glue: tensors must live on the GPU (got {xyz.device}); no CPU fallback")
        L = _bind()
        c = lambda t: None if t is None else t.detach().contiguous().float()
        f_dc, f_rest, dshs, xyz_c, campos_c = c(f_dc), c(f_rest), c(dshs), c(xyz), c(campos)
        ls, rr, ol = c(log_scales), c(rot_raw), c(opacity_logit)
        P, dev, V = xyz_c.shape[0], xyz_c.device, campos_c.shape[0]
        if f_dc.shape != (P, 1, 3) or f_rest.shape != (P, 15, 3):
            raise RuntimeError("render glue expects f_dc [P,1,3] and f_rest [P,15,3] (sh_degree 3 storage)")
        colors = [torch.empty((P, 3), dtype=torch.float32, device=dev) for _ in range(V)]
        scales = torch.empty((P, 3), dtype=torch.float32, device=dev)
        rot = torch.empty((P, 4), dtype=torch.float32, device=dev)
        opac = torch.empty((P, 1), dtype=torch.float32, device=dev)
        asked_l1 = bool(want_dshs_l1)
        want_dshs_l1 = asked_l1 and dshs is not None and P > 0
        abs_sum = torch.zeros(64 * 16, dtype=torch.float64, device=dev) if want_dshs_l1 else None   # S3G_SUM_DOUBLES
        with _lib.on_device(dev):
            _lib.check(L.s3g_glue_forward_views(P, int(deg), V, _p(f_dc), _p(f_rest), _p(dshs), _p(xyz_c), _p(campos_c), _p(ls),
                                                _p(rr), _p(ol), _ptr_array(colors), _p(scales), _p(rot), _p(opac), _p(abs_sum),
                                                _lib.stream_ptr()))
        ctx.deg, ctx.V = int(deg), V
        ctx.campos_grad, ctx.campos_shape = bool(campos_grad), campos.shape
        ctx.has_dshs = dshs is not None
        ctx.save_for_backward(f_dc, f_rest, dshs if dshs is not None else torch.empty(0, device=dev), xyz_c, campos_c, rr,
                              scales, rot, opac, *colors)
        ctx.want_dshs_l1 = want_dshs_l1
        ctx.set_materialize_grads(False)     # a view whose colours fed nothing passes NULL instead of a [P,3] block of zeros
        if want_dshs_l1:
            dshs_l1 = (abs_sum.sum() / (48.0 * P)).float()
        elif asked_l1:
            dshs_l1 = torch.zeros((), dtype=torch.float32, device=dev)     # asked for, nothing to sum (no dshs / P == 0)
        else:
            dshs_l1 = torch.empty((), dtype=torch.float32, device=dev)     # not asked for: dropped by the wrapper, no fill launch
        return (*colors, scales, rot, opac, dshs_l1)

    @staticmethod
    def backward(ctx, *grads):
        V = ctx.V
        f_dc, f_rest, dshs, xyz, campos, rr, scales, rot, opac, *colors = ctx.saved_tensors
        L = _bind()
        P, dev = xyz.shape[0], xyz.device
        dshs = dshs if ctx.has_dshs else None
        c = lambda t: None if t is None else t.contiguous().float()
        g_colors = [c(g) for g in grads[:V]]
        g_scales, g_rot, g_opac, g_l1 = (c(g) for g in grads[V:V + 4])
        e = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        g_f_dc, g_f_rest, g_xyz, g_ls, g_rr, g_ol = e(P, 1, 3), e(P, 15, 3), e(P, 3), e(P, 3), e(P, 4), e(P, 1)
        g_dshs = e(P, 16, 3) if ctx.has_dshs else None
        g_l1 = g_l1 if ctx.want_dshs_l1 else None
        args = (P, ctx.deg, V, _p(f_dc), _p(f_rest), _p(dshs), _p(xyz), _p(campos), _p(rr), _ptr_array(colors), _p(scales), _p(rot),
                _p(opac), _ptr_array(g_colors), _p(g_scales), _p(g_rot), _p(g_opac), _p(g_f_dc), _p(g_f_rest), _p(g_dshs), _p(g_xyz),
                _p(g_ls), _p(g_rr), _p(g_ol), _p(g_l1))
        g_campos = None
        if ctx.campos_grad and ctx.needs_input_grad[5]:
            # every view's own direction term, summed over P in double in camera_backward's order: per view, the bits that
            # _Glue.backward returns for that camera alone
            tv = [e(P, 3) for _ in range(V)]
            work = torch.empty(L.s3g_glue_backward_views_campos_workspace_bytes(P, V), dtype=torch.uint8, device=dev)
            g_campos64 = torch.empty((V, 3), dtype=torch.float64, device=dev)
            with _lib.on_device(dev):
                _lib.check(L.s3g_glue_backward_views_campos(*args, _ptr_array(tv), _p(work) if work.numel() else None,
                                                            _p(g_campos64), _lib.stream_ptr()))
            g_campos = g_campos64.to(torch.float32).view(ctx.campos_shape)
        else:
            with _lib.on_device(dev):
                _lib.check(L.s3g_glue_backward_views(*args, _lib.stream_ptr()))
        return None, g_f_dc, g_f_rest, g_dshs, g_xyz, g_campos, g_ls, g_rr, g_ol, None, None


def activations_and_colors_views(deg, f_dc, f_rest, dshs, xyz, campos_list, log_scales, rot_raw, opacity_logit,
                                 with_dshs_l1=False, campos_grad=False):
    """activations_and_colors for the V cameras of one timestamp (1 <= V <= 8) in one pass each way
    (include/s3g_glue.h::s3g_glue_*_views): -> ([colors_0 .. colors_{V-1}], scales, rotations, opacity[, dshs_l1]).
    campos_list: V camera centres ([3] each) or one [V,3] tensor.  Colours are bit-identical to V single-camera calls; the
    gradients are their fp32 sum, view 0 first.
    campos_grad=True (pose refinement of a rig's cameras): the camera centres may require a gradient; every view then gets its own,
    fp32 in the shape it was given, bit-identical to what activations_and_colors returns for that camera alone (the sum over the
    Gaussians runs in double in the same fixed order).  Two more launches in the backward, and V x [P,3] floats of scratch.  With
    the default a camera centre that requires a gradient is refused and nothing new is launched."""
    if not campos_grad and torch.is_grad_enabled() and \
            any(torch.is_tensor(cp) and cp.requires_grad for cp in ([campos_list] if torch.is_tensor(campos_list) else campos_list)):
        raise RuntimeError("activations_and_colors_views: a camera centre requires a gradient; camera gradients are served with "
                           "campos_grad=True, or by activations_and_colors (one view per call)")
    campos = campos_list if torch.is_tensor(campos_list) else torch.stack([torch.as_tensor(cp).reshape(3) for cp in campos_list])
    campos = campos.reshape(-1, 3)
    V = campos.shape[0]
    if not 1 <= V <= MAX_VIEWS:
        raise RuntimeError(f"render glue: {V} views in one call (1 .. {MAX_VIEWS} are served)")
    out = _GlueViews.apply(deg, f_dc, f_rest, dshs, xyz, campos.to(xyz.device), log_scales, rot_raw, opacity_logit, with_dshs_l1,
                           bool(campos_grad))
    res = (list(out[:V]), out[V], out[V + 1], out[V + 2])
    return res + (out[V + 3],) if with_dshs_l1 else res
