"""Geometry heads of the deformation MLP (scales_deform / rotations_deform / opacity_deform) on the MI355X matrix cores: a second
autograd node beside mlp._DeformMLP that recomputes hidden = feature_out(features) itself; see include/s3g_mlp_geom.h."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib

_NAMES = ["W0", "b0", "C1", "cb1", "C2", "cb2", "R1", "rb1", "R2", "rb2", "O1", "ob1", "O2", "ob2"]
_SHAPES = [(64, 128), (64,), (64, 64), (64,), (3, 64), (3,), (64, 64), (64,), (4, 64), (4,), (64, 64), (64,), (1, 64), (1,)]
_WIDTH = (3, 4, 1)      # columns of ds, dr, do


class _GeomParams(C.Structure):
    """struct s3g_geom_params (include/s3g_mlp_geom.h)."""
    _fields_ = [(n, C.c_void_p) for n in _NAMES]


_bound = False


def _bind():
    global _bound
    L = _lib.lib()
    if not _bound:
        vp = C.c_void_p
        L.s3g_deform_geom_stash_bytes.restype = C.c_size_t
        L.s3g_deform_geom_stash_bytes.argtypes = [C.c_int]
        L.s3g_deform_geom_workspace_bytes.restype = C.c_size_t
        L.s3g_deform_geom_workspace_bytes.argtypes = [C.c_int]
        L.s3g_deform_geom_forward.restype = C.c_int
        L.s3g_deform_geom_forward.argtypes = [C.POINTER(_GeomParams), C.c_int, vp, vp, vp, vp, vp, C.c_int, vp]
        L.s3g_deform_geom_backward.restype = C.c_int
        L.s3g_deform_geom_backward.argtypes = [C.POINTER(_GeomParams), C.c_int, vp, vp, vp, vp, vp, vp, C.POINTER(_GeomParams), vp, vp]
        _bound = True
    return L


def _slots(present, tensors):
    """The 14 slots of _NAMES from W0, b0 and the four tensors of each present head (absent heads: None)."""
    it = iter(tensors)
    out = [next(it), next(it)]
    for on in present:
        out += [next(it) for _ in range(4)] if on else [None] * 4
    return out


def _pack(slots) -> _GeomParams:
    p = _GeomParams()
    for n, shape, t in zip(_NAMES, _SHAPES, slots):
        if t is None:      # an absent head: NULL, never read
            continue
        if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError(f"geometry heads: parameter {n} must be contiguous float32 {shape}, got {tuple(t.shape)} {t.dtype}")
        setattr(p, n, t.data_ptr())
    return p


class _GeometryHeads(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, grad_mode, present, *params):
        # `params`: W0, b0, then weight / bias of the two Linear of every PRESENT head; an absent head's parameters are no inputs
        if not features.is_cuda:
            raise RuntimeError(f"geometry heads: features must live on the GPU (got {features.device}); no CPU fallback")
        L = _bind()
        x = features.contiguous().float()
        P, dev = x.shape[0], x.device
        outs = [torch.empty((P, n), dtype=torch.float32, device=dev) if on else None for on, n in zip(present, _WIDTH)]
        # needs_input_grad is True for parameters even under torch.no_grad(); the caller's grad mode decides (as in mlp._DeformMLP)
        need_bwd = bool(grad_mode) and any(ctx.needs_input_grad)
        stash = torch.empty(L.s3g_deform_geom_stash_bytes(P if need_bwd else 0) // 4, dtype=torch.float32, device=dev)
        w = _pack(_slots(present, [p.detach() for p in params]))
        with _lib.on_device(dev):
            _lib.check(L.s3g_deform_geom_forward(C.byref(w), P, x.data_ptr(), *(o.data_ptr() if o is not None else None for o in outs),
                                                 stash.data_ptr(), int(need_bwd), _lib.stream_ptr()))
        if need_bwd:
            ctx.save_for_backward(x, stash, *params)
            ctx.present = present
            ctx.set_materialize_grads(False)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *g_outs):
        x, stash, *params = ctx.saved_tensors
        L = _bind()
        P, dev = x.shape[0], x.device
        present = ctx.present
        # a present head whose output received no gradient is fed zeros (the z() convention of mlp._DeformMLP.backward)
        gs = [None if not on else (torch.zeros((P, n), dtype=torch.float32, device=dev) if g is None else g.contiguous().float())
              for on, n, g in zip(present, _WIDTH, g_outs)]
        gx = torch.empty_like(x)
        flat = torch.zeros(sum(p.numel() for p in params), dtype=torch.float32, device=dev)   # one fill, up to 14 views
        grads, off = [], 0
        for p in params:
            grads.append(flat[off:off + p.numel()].view(p.shape))
            off += p.numel()
        ws = torch.empty(L.s3g_deform_geom_workspace_bytes(P) // 4, dtype=torch.float32, device=dev)
        w, gw = _pack(_slots(present, [p.detach() for p in params])), _pack(_slots(present, grads))
        with _lib.on_device(dev):
            _lib.check(L.s3g_deform_geom_backward(C.byref(w), P, x.data_ptr(), stash.data_ptr(),
                                                  *(g.data_ptr() if g is not None else None for g in gs), gx.data_ptr(), C.byref(gw),
                                                  ws.data_ptr(), _lib.stream_ptr()))
        return (gx, None, None, *grads)


def geometry_heads(features, feature_out, scales_deform, rotations_deform, opacity_deform):
    """features [P,128] -> (ds [P,3], dr [P,4], do [P,1]) with the reference's Sequential modules as parameter holders
    (feature_out = Sequential(Linear); heads = Sequential(ReLU, Linear, ReLU, Linear)).
    Any of the three head modules may be None (ModelHiddenParams no_ds / no_dr / no_do): that head is skipped in every kernel, its
    output is None and its parameters are not inputs of the autograd node -- their .grad stays None, as under the reference's
    autograd.  The node's gradients with respect to `features` and feature_out's parameters are this family's own terms; autograd
    adds them to those of mlp.deform_mlp on the same tensors.  Under torch.no_grad() no stash is saved."""
    heads = (scales_deform, rotations_deform, opacity_deform)
    present = tuple(h is not None for h in heads)
    if not any(present):
        raise ValueError("geometry_heads: at least one of scales_deform, rotations_deform, opacity_deform must be given")
    if not features.is_cuda:
        raise RuntimeError(f"geometry heads: features must live on the GPU (got {features.device}); no CPU fallback")
    ps = [feature_out[0].weight, feature_out[0].bias]
    for h in heads:
        if h is not None:
            ps += [h[1].weight, h[1].bias, h[3].weight, h[3].bias]
    return _GeometryHeads.apply(features, torch.is_grad_enabled(), present, *ps)
