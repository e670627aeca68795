"""Python surface of the rasterizer: same public names, fields, call signatures and error behaviour as
RAST/diff_gaussian_rasterization/__init__.py:158-221 so that the reference's gaussian_renderer/__init__.py:18,44-57,
127-135 imports and calls it unchanged.  The top-level package `diff_gaussian_rasterization` re-exports these.
"""
from __future__ import annotations

from typing import NamedTuple

import torch
from torch import nn

from . import raster_C as _C


class GaussianRasterizationSettings(NamedTuple):
    """12 fields, keyword-constructed by the caller (gaussian_renderer/__init__.py:44-57)."""
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


def _snapshot(args):
    """debug=True: keep a host copy of every argument so a failing call can be dumped (reference :17-19, :83-90)."""
    return tuple(a.detach().cpu().clone() if isinstance(a, torch.Tensor) else a for a in args)


def _or_zero_images(grads, channels, rs, device):
    """Output gradients with a zero image in place of each one that never arrived (an output that feeds no loss)."""
    return [torch.zeros((c, rs.image_height, rs.image_width), device=device) if g is None else g for g, c in zip(grads, channels)]


def _camera_inputs(rs) -> tuple:
    """(viewmatrix, projmatrix, campos) of the settings when autograd wants a gradient for one of them, else ().  The settings are
    a NamedTuple and no autograd input: the nodes below take the three tensors as real inputs behind their other arguments, ask
    their backward for the internals and hand them to raster_C.camera_backward.  Without a camera that requires a gradient
    nothing changes: the same call, the same launches, the same ctx."""
    cams = (rs.viewmatrix, rs.projmatrix, rs.campos)
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in cams):
        return cams
    return ()


def _camera_grads(ctx, first, means3D, radii, geom, sh, cov3Ds_precomp, g_means2D, g_conic, g_depths, g_colors) -> tuple:
    """The gradients of the three camera inputs (positions first .. first + 2 of the node), fp32 in the tensors' shapes."""
    rs = ctx.raster_settings
    has_sh = sh is not None and sh.numel() != 0
    g = _C.camera_backward(means3D.size(0), means3D.device, means3D=means3D, radii=radii, geomBuffer=geom, viewmatrix=rs.viewmatrix,
                           projmatrix=rs.projmatrix, campos=rs.campos, tan_fovx=rs.tanfovx, tan_fovy=rs.tanfovy,
                           image_height=rs.image_height, image_width=rs.image_width, dL_dmeans2D=g_means2D, dL_dconic=g_conic,
                           dL_ddepths=g_depths, dL_dcolors=g_colors if has_sh else None, sh=sh if has_sh else None,
                           degree=rs.sh_degree, cov3D_precomp=cov3Ds_precomp, debug=rs.debug)
    g32 = g.to(torch.float32)
    parts = (g32[:16], g32[16:32], g32[32:35])
    return tuple(part.view(t.shape) if need else None
                 for part, t, need in zip(parts, (rs.viewmatrix, rs.projmatrix, rs.campos), ctx.needs_input_grad[first:first + 3]))


class _RasterizeGaussians(torch.autograd.Function):
    """autograd node; forward keeps the three private arenas alive for backward (reference :44-156).
    with_alpha (extension): the accumulated opacity A = 1 - final_T as a fourth, differentiable output: one image-sized pass forward
    (s3g_raster_alpha), and a backward that hands grad_alpha to the blend backward (s3g_raster_backward_alpha).  Without a gradient
    on A -- or without with_alpha -- the backward is the reference's."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings,
                forward_only=False, with_alpha=False, viewmatrix=None, projmatrix=None, campos=None):
        rs = raster_settings
        if viewmatrix is not None:
            ctx.camera = True       # (viewmatrix, projmatrix, campos) = the settings' own tensors: _camera_inputs
        native_args = (rs.bg, means3D, colors_precomp, opacities, scales, rotations, rs.scale_modifier, cov3Ds_precomp,
                       rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, sh,
                       rs.sh_degree, rs.campos, rs.prefiltered, rs.debug)
        if rs.debug:
            saved = _snapshot(native_args)
            try:
                out = _C.rasterize_gaussians(*native_args)
            except Exception:
                torch.save(saved, "snapshot_fw.dump")
                print("\nAn error occured in forward. Please forward snapshot_fw.dump for debugging.")
                raise
        else:
            # num_rendered only travels to the backward below as the key of the arenas: the call may run host-asynchronously
            out = _C.rasterize_gaussians(*native_args, allow_async=True, forward_only=forward_only)
        num_rendered, color, depth, radii, geom, binning, img = out
        ctx.raster_settings = rs
        ctx.num_rendered = num_rendered
        ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geom, binning, img)
        ctx.mark_non_differentiable(radii)
        if not with_alpha:
            return color, radii, depth
        ctx.set_materialize_grads(False)      # an output that feeds no loss arrives as None in backward, not as a zero image
        return color, radii, depth, _C.raster_alpha(img, rs.image_height, rs.image_width)

    @staticmethod
    def backward(ctx, grad_out_color, _grad_radii, grad_out_depth, grad_alpha=None):
        rs = ctx.raster_settings
        colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geom, binning, img = ctx.saved_tensors
        grad_out_color, grad_out_depth = _or_zero_images((grad_out_color, grad_out_depth), (3, 1), rs, means3D.device)
        camera = getattr(ctx, "camera", False)
        internals = dict(return_internals=True) if camera else {}
        if grad_alpha is None:
            native_args = (rs.bg, means3D, radii, colors_precomp, scales, rotations, rs.scale_modifier, cov3Ds_precomp,
                           rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, grad_out_color, grad_out_depth, sh,
                           rs.sh_degree, rs.campos, geom, ctx.num_rendered, binning, img, rs.debug)
            if rs.debug:
                saved = _snapshot(native_args)
                try:
                    grads = _C.rasterize_gaussians_backward(*native_args, **internals)
                except Exception:
                    torch.save(saved, "snapshot_bw.dump")
                    print("\nAn error occured in backward. Writing snapshot_bw.dump for debugging.\n")
                    raise
            else:
                grads = _C.rasterize_gaussians_backward(*native_args, **internals)
            g_means2D, g_colors, g_opac, g_means3D, g_cov3D, g_sh, g_scales, g_rot, *g_int = grads
        else:
            (g_means2D, g_colors, _, g_opac, g_means3D, g_cov3D, g_sh, g_scales, g_rot, *g_int) = _C.rasterize_gaussians_backward_alpha(
                rs.bg, means3D, radii, colors_precomp, None, scales, rotations, rs.scale_modifier, cov3Ds_precomp, rs.viewmatrix,
                rs.projmatrix, rs.tanfovx, rs.tanfovy, grad_out_color, grad_out_depth, None, grad_alpha, sh, rs.sh_degree, rs.campos,
                geom, ctx.num_rendered, binning, img, rs.debug, **internals)
        # order of forward's inputs: means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, settings, ...
        g_camera = _camera_grads(ctx, 11, means3D, radii, geom, sh, cov3Ds_precomp, g_means2D, *g_int, g_colors) if camera else ()
        return (g_means3D, g_means2D, g_sh, g_colors, g_opac, g_scales, g_rot, g_cov3D, None, None, None, *g_camera)


class _RasterizeGaussiansPair(torch.autograd.Function):
    """Two renders of one geometry (colours_a -> image + depth, colours_b -> second image) as ONE autograd node: one
    blend pass forward (s3g_raster_forward2) and one backward (s3g_raster_backward2) instead of two each, whose gradients
    autograd would then add.  with_alpha: the accumulated opacity as a fifth, differentiable output (see _RasterizeGaussians)."""

    @staticmethod
    def forward(ctx, means3D, means2D, colors_a, colors_b, opacities, scales, rotations, cov3Ds_precomp, raster_settings,
                densify_accum=None, forward_only=False, with_alpha=False, viewmatrix=None, projmatrix=None, campos=None):
        rs = raster_settings
        if viewmatrix is not None:
            ctx.camera = True       # see _RasterizeGaussians
        empty = torch.Tensor([])
        common = (opacities, scales, rotations, rs.scale_modifier, cov3Ds_precomp, rs.viewmatrix, rs.projmatrix, rs.tanfovx,
                  rs.tanfovy, rs.image_height, rs.image_width, empty, rs.sh_degree, rs.campos, rs.prefiltered, rs.debug)
        num_rendered, color, depth, radii, geom, binning, img, color2 = _C.rasterize_gaussians(
            rs.bg, means3D, colors_a, *common, colors2=colors_b, allow_async=True, forward_only=forward_only)
        ctx.raster_settings = rs
        ctx.num_rendered = num_rendered
        ctx.densify_accum = densify_accum
        ctx.save_for_backward(colors_a, colors_b, means3D, scales, rotations, cov3Ds_precomp, radii, geom, binning, img)
        ctx.mark_non_differentiable(radii)
        if not with_alpha:
            return color, radii, depth, color2
        ctx.set_materialize_grads(False)      # see _RasterizeGaussians
        return color, radii, depth, color2, _C.raster_alpha(img, rs.image_height, rs.image_width)

    @staticmethod
    def backward(ctx, grad_color, _grad_radii, grad_depth, grad_color2, grad_alpha=None):
        rs = ctx.raster_settings
        colors_a, colors_b, means3D, scales, rotations, cov3Ds_precomp, radii, geom, binning, img = ctx.saved_tensors
        grad_color, grad_depth, grad_color2 = _or_zero_images((grad_color, grad_depth, grad_color2), (3, 1, 3), rs, means3D.device)
        head = (rs.bg, means3D, radii, colors_a, colors_b, scales, rotations, rs.scale_modifier, cov3Ds_precomp, rs.viewmatrix,
                rs.projmatrix, rs.tanfovx, rs.tanfovy, grad_color, grad_depth, grad_color2)
        tail = (rs.campos, geom, ctx.num_rendered, binning, img, rs.debug)
        camera = getattr(ctx, "camera", False)
        internals = dict(return_internals=True) if camera else {}
        if grad_alpha is None:
            (g_means2D, g_col_a, g_col_b, g_opac, g_means3D, g_cov3D, g_scales, g_rot, *g_int) = _C.rasterize_gaussians_backward2(
                *head, *tail, densify_accum=ctx.densify_accum, **internals)
        else:
            (g_means2D, g_col_a, g_col_b, g_opac, g_means3D, g_cov3D, _, g_scales, g_rot, *g_int) = _C.rasterize_gaussians_backward_alpha(
                *head, grad_alpha, torch.Tensor([]), 0, *tail, densify_accum=ctx.densify_accum, **internals)
        # both colour sets are precomputed: the camera centre enters neither image
        g_camera = _camera_grads(ctx, 12, means3D, radii, geom, None, cov3Ds_precomp, g_means2D, *g_int, None) if camera else ()
        return (g_means3D, g_means2D, g_col_a, g_col_b, g_opac, g_scales, g_rot, g_cov3D, None, None, None, None, *g_camera)


def _check_arguments(scales, rotations, cov3D_precomp, colour_sources=None):
    """The reference's two argument checks (:192-196), messages included.  colour_sources = (shs, colors_precomp), or None for an
    entry point that takes precomputed colours only."""
    if colour_sources is not None and (colour_sources[0] is None) == (colour_sources[1] is None):
        raise Exception('Please provide excatly one of either SHs or precomputed colors!')
    has_sr = scales is not None or rotations is not None
    if ((scales is None or rotations is None) and cov3D_precomp is None) or (has_sr and cov3D_precomp is not None):
        raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')


def _or_empty(t):
    """The reference's "not provided" sentinel: numel() == 0 -> NULL at the C ABI."""
    return torch.Tensor([]) if t is None else t


def _no_backward(*tensors) -> bool:
    """True when autograd will record nothing for a node over these inputs (no_grad, or no input requires a gradient): the
    forward may then skip what only a backward would read (raster_C.rasterize_gaussians: forward_only)."""
    return not (torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors))


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings):
    tensors = (means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp)
    cams = _camera_inputs(raster_settings)
    if cams:
        return _RasterizeGaussians.apply(*tensors, raster_settings, False, False, *cams)
    return _RasterizeGaussians.apply(*tensors, raster_settings, _no_backward(*tensors))


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions):
        """bool[P]: Gaussians in front of the near cull plane (view z > 0.2)."""
        with torch.no_grad():
            rs = self.raster_settings
            return _C.mark_visible(positions, rs.viewmatrix, rs.projmatrix)

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None):
        _check_arguments(scales, rotations, cov3D_precomp, colour_sources=(shs, colors_precomp))
        return rasterize_gaussians(means3D, means2D, _or_empty(shs), _or_empty(colors_precomp), opacities, _or_empty(scales),
                                   _or_empty(rotations), _or_empty(cov3D_precomp), self.raster_settings)

    def forward_alpha(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                      cov3D_precomp=None):
        """Extension (not in the reference, whose rasterizer returns no accumulated opacity): `forward` plus the opacity image.
        -> (color [3,H,W], radii [P], depth [1,H,W], alpha [1,H,W]); alpha = 1 - the final transmittance of the pixel, i.e. what
        unit colours on a black background would render, and a loss on it back-propagates through the same backward pass."""
        _check_arguments(scales, rotations, cov3D_precomp, colour_sources=(shs, colors_precomp))
        tensors = (means3D, means2D, _or_empty(shs), _or_empty(colors_precomp), opacities, _or_empty(scales), _or_empty(rotations),
                   _or_empty(cov3D_precomp))
        cams = _camera_inputs(self.raster_settings)
        return _RasterizeGaussians.apply(*tensors, self.raster_settings, False if cams else _no_backward(*tensors), True, *cams)

    @torch.no_grad()
    def forward_decomposed(self, means3D, opacities, dynamic_mask, shs=None, colors_precomp=None, scales=None, rotations=None,
                           cov3D_precomp=None, with_alpha=False):
        """Extension for the evaluation path (gaussian_renderer/__init__.py:168-204, `return_decomposition=True`): the full
        render plus the dynamic-only and static-only renders, sharing ONE preprocess / binning / sort; the two subset images
        come from one extra blend pass and equal `self(...)` on the masked inputs bit for bit.  Inference only (no autograd).
        -> dict(render, radii, depth, render_d, depth_d, render_s, depth_s); with_alpha adds alpha [1,H,W], the accumulated
        opacity of the FULL render (forward_alpha)."""
        rs = self.raster_settings
        _check_arguments(scales, rotations, cov3D_precomp, colour_sources=(shs, colors_precomp))
        n = _or_empty
        P = means3D.shape[0]
        R, color, depth, radii, geom, binning, img = _C.rasterize_gaussians(
            rs.bg, means3D, n(colors_precomp), opacities, n(scales), n(rotations), rs.scale_modifier, n(cov3D_precomp),
            rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, rs.image_height, rs.image_width, n(shs), rs.sh_degree,
            rs.campos, rs.prefiltered, rs.debug, allow_async=True, forward_only=True)
        extra = dict(alpha=_C.raster_alpha(img, rs.image_height, rs.image_width)) if with_alpha else {}
        if P == 0:
            z3, z1 = torch.zeros_like(color), torch.zeros_like(depth)
            return dict(render=color, radii=radii, depth=depth, render_d=z3, depth_d=z1, render_s=z3.clone(), depth_s=z1.clone(), **extra)
        cd, dd, cs, ds = _C.rasterize_decomposition(rs.bg, n(colors_precomp), dynamic_mask, rs.tanfovx, rs.tanfovy,
                                                    rs.image_height, rs.image_width, P, R, geom, binning, img, rs.debug)
        return dict(render=color, radii=radii, depth=depth, render_d=cd, depth_d=dd, render_s=cs, depth_s=ds, **extra)

    def forward_pair(self, means3D, means2D, opacities, colors_a, colors_b, scales=None, rotations=None, cov3D_precomp=None,
                     densify_accum=None, with_alpha=False):
        """Extension (not in the reference): render the SAME Gaussians with two sets of precomputed colours, e.g. RGB and the
        feature head's output (gaussian_renderer/__init__.py:127-166 does this with two calls).
        -> (image_a [3,H,W], radii [P], depth [1,H,W], image_b [3,H,W]); gradients equal those of the two separate calls.
        densify_accum = (xyz_gradient_accum, denom, max_radii2D): the backward of this node also performs the reference's
        densification bookkeeping (train.py:489-493) in its per-Gaussian pass -- valid because this node yields the whole
        viewspace gradient of the iteration.
        with_alpha=True appends the opacity image of forward_alpha: -> (image_a, radii, depth, image_b, alpha [1,H,W])."""
        _check_arguments(scales, rotations, cov3D_precomp)
        if means3D.shape[0] == 0 or self.raster_settings.debug:
            # nothing to share / debug snapshots wanted: fall back to two ordinary nodes
            if densify_accum is not None:   # direct callers only: pipeline.render() decides before calling
                raise RuntimeError("densify_accum needs the fused two-image node (P > 0, debug off)")
            first = self.forward_alpha if with_alpha else self.forward
            a, radii, depth, *alpha = first(means3D, means2D, opacities, colors_precomp=colors_a, scales=scales, rotations=rotations,
                                            cov3D_precomp=cov3D_precomp)
            b, _, _ = self.forward(means3D, means2D, opacities, colors_precomp=colors_b, scales=scales, rotations=rotations,
                                   cov3D_precomp=cov3D_precomp)
            return (a, radii, depth, b, *alpha)
        tensors = (means3D, means2D, colors_a, colors_b, opacities, _or_empty(scales), _or_empty(rotations), _or_empty(cov3D_precomp))
        cams = _camera_inputs(self.raster_settings)
        return _RasterizeGaussiansPair.apply(*tensors, self.raster_settings, densify_accum, False if cams else _no_backward(*tensors),
                                             bool(with_alpha), *cams)
