"""Fused deformation MLP (feature_out + pos/shs/dino heads) on the MI355X matrix cores; see include/s3g_mlp.h."""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _lib

_NAMES = ["W0", "b0", "P1", "pb1", "P2", "pb2", "S1", "sb1", "S2", "sb2", "D0", "db0", "D1", "db1", "D2", "db2"]
_SHAPES = [(64, 128), (64,), (64, 64), (64,), (3, 64), (3,), (64, 64), (64,), (48, 64), (48,), (64, 64), (64,), (64, 64),
           (64,), (3, 64), (3,)]


class _Params(C.Structure):
    """struct s3g_mlp_params (include/s3g_mlp.h)."""
    _fields_ = [(n, C.c_void_p) for n in _NAMES]


_bound = False


def _bind():
    global _bound
    L = _lib.lib()
    if not _bound:
        vp = C.c_void_p
        L.s3g_deform_mlp_stash_bytes.restype = C.c_size_t
        L.s3g_deform_mlp_stash_bytes.argtypes = [C.c_int]
        L.s3g_deform_mlp_forward.restype = C.c_int
        L.s3g_deform_mlp_forward.argtypes = [C.POINTER(_Params), C.c_int, vp, vp, vp, vp, vp, C.c_int, vp]
        L.s3g_deform_mlp_pack_bytes.restype = C.c_size_t
        L.s3g_deform_mlp_backward.restype = C.c_int
        L.s3g_deform_mlp_backward.argtypes = [C.POINTER(_Params), C.c_int, vp, vp, vp, vp, vp, vp, C.POINTER(_Params), vp, vp]
        L.s3g_deform_mlp_backward_ordered.restype = C.c_int
        L.s3g_deform_mlp_backward_ordered.argtypes = [C.POINTER(_Params), C.c_int, vp, vp, vp, vp, vp, vp, C.POINTER(_Params), vp, vp, vp]
        L.s3g_deform_mlp_wgrad_partial_bytes.restype = C.c_size_t
        from .hexplane import _HexDesc
        L.s3g_deform_infer_workspace_bytes.restype = C.c_size_t
        L.s3g_deform_infer_workspace_bytes.argtypes = [C.POINTER(_HexDesc)]
        L.s3g_deform_infer.restype = C.c_int
        L.s3g_deform_infer.argtypes = [C.POINTER(_HexDesc), C.POINTER(_Params), C.c_int, vp, vp, vp, vp, vp, vp, vp]
        L.s3g_deform_infer_split.restype = C.c_int
        L.s3g_deform_infer_split.argtypes = L.s3g_deform_infer.argtypes
        from .mlp_geom import _GeomParams
        L.s3g_deform_infer_heads_lds_bytes.restype = C.c_size_t
        L.s3g_deform_infer_heads_lds_bytes.argtypes = [C.c_int]
        L.s3g_deform_infer_heads.restype = C.c_int
        L.s3g_deform_infer_heads.argtypes = [C.POINTER(_HexDesc), C.POINTER(_Params), C.POINTER(_GeomParams), C.c_int] + [vp] * 10
        L.s3g_deform_mlp_set_arithmetic.restype = C.c_int
        L.s3g_deform_mlp_set_arithmetic.argtypes = [C.c_int]
        L.s3g_deform_mlp_get_arithmetic.restype = C.c_int
        _bound = True
        set_mlp_arithmetic(os.environ.get("S3G_MLP_ARITHMETIC") or DEFAULT_ARITHMETIC)
    return L


_ARITHMETIC = {"f32": 0, "bf16x3": 1, "bf16x3_onthefly": 2}     # S3G_MLP_F32, S3G_MLP_BF16X3, S3G_MLP_BF16X3_ONTHEFLY (include/s3g_mlp.h)
# Round 6: the per-point GEMM chains run on the bf16 matrix pipe with every fp32 operand split EXACTLY into three bf16 pieces and fp32
# accumulation ("bf16x3", weight fragments split once per call) unless S3G_MLP_ARITHMETIC=f32 asks for the exact fp32 fma chains.  The
# three conditions round 4's review set for this default were met in round 5: BASELINE-size parity on the exact chain's
# bars in both arithmetics, PSNR at cfg2 size +0.03 / +0.007 dB against the reference's mean, the split kernels bit-reproducible over
# 200 / 1000 launches with the staging-store guard asserted on the built ISA.  The results are fp32 results (distance from fp64 no larger
# than the exact chain's); they are NOT bit-identical to the exact chain.  The C library's own default stays S3G_MLP_F32.
DEFAULT_ARITHMETIC = "bf16x3"
# S3G_MLP_ORDERED_WGRAD=0: the weight-gradient kernel's workgroups add their partial blocks with float atomics (rounds 1-5: the sum's
# order, hence its last bits, differed between runs); default: partial blocks summed in workgroup order by a second kernel
ORDERED_WGRAD_FLUSH = os.environ.get("S3G_MLP_ORDERED_WGRAD", "1") != "0"


def set_mlp_arithmetic(mode: str) -> None:
    """Arithmetic of the per-point GEMM chains of deform_mlp's forward and backward kernels (process-wide; environment:
    S3G_MLP_ARITHMETIC): "f32" = exact fp32 fma chains, "bf16x3" (DEFAULT_ARITHMETIC since round 6) = the bf16 matrix pipe on operands
    split exactly into three bf16 pieces (fp32 accuracy, not bit-identical to the exact chain).  The weight-gradient GEMMs are the exact chain in both modes."""
    if mode not in _ARITHMETIC:
        raise ValueError(f"set_mlp_arithmetic: mode must be one of {sorted(_ARITHMETIC)}, got {mode!r}")
    _lib.check(_bind().s3g_deform_mlp_set_arithmetic(_ARITHMETIC[mode]))


def get_mlp_arithmetic() -> str:
    v = _bind().s3g_deform_mlp_get_arithmetic()
    return next(k for k, x in _ARITHMETIC.items() if x == v)


_POS = slice(2, 6)     # P1, pb1, P2, pb2: the position head's slots in _NAMES
_SHS = slice(6, 10)    # S1, sb1, S2, sb2: the SH head's
_DINO = slice(10, 16)  # D0 .. db2: the feature (dino) head's


def _pack(tensors) -> _Params:
    p = _Params()
    for n, shape, t in zip(_NAMES, _SHAPES, tensors):
        if t is None:      # a gradient slot the library does not touch (a skipped head's): NULL
            continue
        if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError(f"deform MLP: parameter {n} must be contiguous float32 {shape}, got {tuple(t.shape)} {t.dtype}")
        setattr(p, n, t.data_ptr())
    return p


_zero_blocks = {}


def _zero_dino(dev):
    """The six weight slots of a network WITHOUT a dino_head module (feat_head=False): views of one shared block of 4096 zeros per
    device.  The pack kernels copy whole images whatever the heads, so the slots must point at readable memory."""
    z = _zero_blocks.get(dev)
    if z is None:
        z = _zero_blocks[dev] = torch.zeros(4096, dtype=torch.float32, device=dev)
    return tuple(z[:int(torch.Size(shape).numel())].view(shape) for shape in _SHAPES[_DINO])


class _DeformMLP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, need_feat, grad_mode, fill, *params):
        # fill is None: `params` are all 16 tensors.  Else `fill` has 16 entries: None for a slot that `params` supplies (in _NAMES order),
        # a detached tensor for a slot of a head that is skipped -- NOT an input of this node (the kernels skip the head but the pack
        # kernels still copy its weights into the LDS images): need_dx=False, need_dshs=False, dino_head=None
        if not features.is_cuda:
            raise RuntimeError(f"deform MLP: features must live on the GPU (got {features.device}); no CPU fallback")
        L = _bind()
        x = features.contiguous().float()
        P, dev = x.shape[0], x.device
        live = lambda sl: fill is None or fill[sl.start] is None
        has_dino = live(_DINO)
        dx = torch.empty((P, 3), dtype=torch.float32, device=dev) if live(_POS) else None
        dshs = torch.empty((P, 48), dtype=torch.float32, device=dev) if live(_SHS) else None
        # needs_input_grad is True for parameters even under torch.no_grad(); the caller's grad mode decides whether a
        # backward can follow (inside Function.forward grad mode is always off)
        need_bwd = bool(grad_mode) and any(ctx.needs_input_grad)
        need_feat = has_dino and (bool(need_feat) or need_bwd)   # the feature head is only skippable when no backward follows
        feat = torch.empty((P, 3), dtype=torch.float32, device=dev) if need_feat else None
        nbytes = L.s3g_deform_mlp_stash_bytes(P) if need_bwd else L.s3g_deform_mlp_pack_bytes()
        stash = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
        w = _pack(_all16(fill, [p.detach() for p in params]))
        ptr = lambda t: t.data_ptr() if t is not None else None
        with _lib.on_device(dev):
            _lib.check(L.s3g_deform_mlp_forward(C.byref(w), P, x.data_ptr(), ptr(dx), ptr(dshs), ptr(feat),
                                                stash.data_ptr(), int(need_bwd), _lib.stream_ptr()))
        if need_bwd:
            ctx.save_for_backward(x, stash, *params)
            ctx.fill = fill
            ctx.set_materialize_grads(False)   # an output the loss never touched must arrive as None, not as zeros
        return dx, dshs, feat     # feat is None when the head was skipped (need_feat=False under no_grad) or does not exist

    @staticmethod
    def backward(ctx, g_dx, g_dshs, g_feat):
        x, stash, *params = ctx.saved_tensors
        L = _bind()
        P, dev = x.shape[0], x.device
        z = lambda g, n: (torch.zeros((P, n), dtype=torch.float32, device=dev) if g is None else g.contiguous().float())
        fill = ctx.fill    # a skipped head: NULL for its upstream gradient, no gradient slots for its parameters
        live = lambda sl: fill is None or fill[sl.start] is None
        g_dx = z(g_dx, 3) if live(_POS) else None
        g_dshs = z(g_dshs, 48) if live(_SHS) else None
        # no gradient on the feature output (feature image not in the loss): like the reference, the dino head's parameters
        # then get grad None -- Adam skips them (no moment decay, no step count) -- and its part of the backward is skipped
        # (a node whose ONLY head is the feature head differentiates it against zeros instead: the library needs one head)
        has_dino = live(_DINO)
        no_feat = not has_dino or (g_feat is None and (g_dx is not None or g_dshs is not None))
        g_feat = None if no_feat else z(g_feat, 3)
        ptr = lambda t: t.data_ptr() if t is not None else None
        gx = torch.empty_like(x)
        flat = torch.zeros(sum(p.numel() for p in params), dtype=torch.float32, device=dev)  # one fill, up to 16 views
        grads, off = [], 0
        for p in params:
            grads.append(flat[off:off + p.numel()].view(p.shape))
            off += p.numel()
        ws = torch.empty((5, P, 64), dtype=torch.float32, device=dev)
        w, gw = _pack(_all16(fill, [p.detach() for p in params])), _pack(_all16(fill, grads, grad_slots=True))
        with _lib.on_device(dev):
            if ORDERED_WGRAD_FLUSH:     # bit-reproducible weight gradients (include/s3g_mlp.h::s3g_deform_mlp_backward_ordered)
                part = torch.empty(L.s3g_deform_mlp_wgrad_partial_bytes() // 4, dtype=torch.float32, device=dev)
                _lib.check(L.s3g_deform_mlp_backward_ordered(C.byref(w), P, x.data_ptr(), stash.data_ptr(), ptr(g_dx),
                                                             ptr(g_dshs), ptr(g_feat), gx.data_ptr(),
                                                             C.byref(gw), ws.data_ptr(), part.data_ptr(), _lib.stream_ptr()))
            else:
                _lib.check(L.s3g_deform_mlp_backward(C.byref(w), P, x.data_ptr(), stash.data_ptr(), ptr(g_dx),
                                                     ptr(g_dshs), ptr(g_feat), gx.data_ptr(),
                                                     C.byref(gw), ws.data_ptr(), _lib.stream_ptr()))
        if no_feat and has_dino:
            names = [n for i, n in enumerate(_NAMES) if fill is None or fill[i] is None]
            grads = [None if n.startswith(("D", "db")) else g for n, g in zip(names, grads)]
        return (gx, None, None, None, *grads)


def _all16(fill, rest, grad_slots=False):
    """The 16 slots of _NAMES: slot i is fill[i] where that is not None (a skipped head's weight; with grad_slots=True: None, its
    gradient slot is NULL), else the next tensor of `rest`; fill is None: `rest` already has all 16."""
    if fill is None:
        return list(rest)
    it = iter(rest)
    return [next(it) if f is None else (None if grad_slots else f) for f in fill]


def _head_params(feature_out, pos_deform, shs_deform, dino_head):
    """The 16 tensors in _NAMES order; the six of a network without a dino_head module (feat_head=False) are None."""
    dino = [None] * 6 if dino_head is None else [dino_head[0].weight, dino_head[0].bias, dino_head[2].weight, dino_head[2].bias,
                                                  dino_head[4].weight, dino_head[4].bias]
    return [feature_out[0].weight, feature_out[0].bias, pos_deform[1].weight, pos_deform[1].bias, pos_deform[3].weight,
            pos_deform[3].bias, shs_deform[1].weight, shs_deform[1].bias, shs_deform[3].weight, shs_deform[3].bias] + dino


@torch.no_grad()
def deform_infer(grid, xyz, time, feature_out, pos_deform, shs_deform, dino_head, uniform_time=None, arithmetic="f32"):
    """Inference only: HexPlane sampler (+) feature_out + position / SH heads in ONE kernel (include/s3g_mlp.h::s3g_deform_infer).
    xyz [P,3], time [P,1] -> (dx [P,3], dshs [P,48]); bit-identical to `deform_mlp(grid(xyz, time), ..., need_feat=False)[:2]`
    without ever materialising the [P,128] features.  `grid` is the HexPlaneField (4 levels x 32 channels).
    arithmetic="bf16x3": the three GEMM layers on the bf16 matrix pipe with every fp32 operand split exactly into three bf16 pieces
    (s3g_deform_infer_split: fp32 accuracy, not bit-identical; the sampler half is unchanged)."""
    if arithmetic not in ("f32", "bf16x3"):
        raise ValueError(f"deform_infer: arithmetic must be 'f32' or 'bf16x3', got {arithmetic!r}")
    from .hexplane import _make_desc
    if not xyz.is_cuda:
        raise RuntimeError(f"deform_infer: xyz must live on the GPU (got {xyz.device}); no CPU fallback")
    L = _bind()
    P, dev = xyz.shape[0], xyz.device
    xyz_c = xyz.detach().contiguous().float()
    t_c = time.detach().reshape(-1).contiguous().float()
    if t_c.numel() != P and not (uniform_time is True and t_c.numel() == 1):   # uniform time: one shared timestamp is enough
        raise RuntimeError("time must have one value per point")
    if uniform_time is None:
        uniform_time = bool(P > 0 and (t_c == t_c[0]).all().item())
    d = _make_desc(grid._planes(), grid.resolutions, grid._host_aabb(), bool(uniform_time) and P > 0)
    order = grid._order_cache.get("order")
    if order is not None and (order.numel() != P or order.device != dev):
        order = None
    dx = torch.empty((P, 3), dtype=torch.float32, device=dev)
    dshs = torch.empty((P, 48), dtype=torch.float32, device=dev)
    ws = torch.empty(max(L.s3g_deform_infer_workspace_bytes(C.byref(d)), 4) // 4, dtype=torch.float32, device=dev)
    ps = _head_params(feature_out, pos_deform, shs_deform, dino_head)
    if dino_head is None:      # feat_head=False: the kernel never reads the dino slabs' values, the pack kernel copies them
        ps[_DINO] = _zero_dino(dev)
    w = _pack([p.detach() for p in ps])
    with _lib.on_device(dev):
        fn = L.s3g_deform_infer_split if arithmetic == "bf16x3" else L.s3g_deform_infer
        _lib.check(fn(C.byref(d), C.byref(w), P, xyz_c.data_ptr(), t_c.data_ptr(), order.data_ptr() if order is not None else None,
                      dx.data_ptr(), dshs.data_ptr(), ws.data_ptr(), _lib.stream_ptr()))
    return dx, dshs


_HEAD_BITS = (1, 2, 4, 8, 16)     # dx, ds, dr, do, dshs: the head mask of include/s3g_mlp.h::s3g_deform_infer_heads_lds_bytes


def infer_heads_lds_bytes(need_dx, need_dshs, need_ds, need_dr, need_do) -> int:
    """Dynamic LDS of the one-kernel inference route for this head set, 0 for a set it does not serve (host code: no GPU needed)."""
    mask = sum(b for b, on in zip(_HEAD_BITS, (need_dx, need_ds, need_dr, need_do, need_dshs)) if on)
    return int(_bind().s3g_deform_infer_heads_lds_bytes(mask))


def infer_heads_served(need_dx, need_dshs, need_ds, need_dr, need_do) -> bool:
    """Does deform_infer_heads serve this head set?  (Every non-empty subset of dx / ds / dr / do with at most three heads, dshs alone,
    dshs with one of ds / dr / do; not the empty set, not dx + dshs alone -- deform_infer's -- and no set whose weights do not fit.)"""
    return infer_heads_lds_bytes(need_dx, need_dshs, need_ds, need_dr, need_do) > 0


@torch.no_grad()
def deform_infer_heads(grid, xyz, time, feature_out, pos_deform, shs_deform, geometry=(None, None, None), uniform_time=None):
    """Inference only: HexPlane sampler (+) feature_out (+) the heads given, in ONE kernel (include/s3g_mlp.h::s3g_deform_infer_heads).
    pos_deform / shs_deform / the three entries of geometry = (scales_deform, rotations_deform, opacity_deform): a module given as None
    is an absent head.  xyz [P,3], time [P,1] -> (dx [P,3], dshs [P,48], ds [P,3], dr [P,4], do [P,1]) with None for absent heads;
    bit-identical to `deform_mlp(grid(xyz, time), ..., need_feat=False, need_dx=..., need_dshs=...)` (with shs_deform: in the "f32"
    arithmetic, which is this kernel's only one) and `geometry_heads(grid(xyz, time), ...)` without ever materialising the [P,128]
    features.  A head set the kernel does not serve (infer_heads_served) is an error, not a fall-back."""
    from .hexplane import _make_desc
    from .mlp_geom import _GeomParams
    if not xyz.is_cuda:
        raise RuntimeError(f"deform_infer_heads: xyz must live on the GPU (got {xyz.device}); no CPU fallback")
    L = _bind()
    P, dev = xyz.shape[0], xyz.device
    xyz_c = xyz.detach().contiguous().float()
    t_c = time.detach().reshape(-1).contiguous().float()
    if t_c.numel() != P and not (uniform_time is True and t_c.numel() == 1):   # uniform time: one shared timestamp is enough
        raise RuntimeError("time must have one value per point")
    if uniform_time is None:
        uniform_time = bool(P > 0 and (t_c == t_c[0]).all().item())
    d = _make_desc(grid._planes(), grid.resolutions, grid._host_aabb(), bool(uniform_time) and P > 0)
    order = grid._order_cache.get("order")
    if order is not None and (order.numel() != P or order.device != dev):
        order = None
    heads = (pos_deform, shs_deform) + tuple(geometry)
    outs = [torch.empty((P, n), dtype=torch.float32, device=dev) if m is not None else None for m, n in zip(heads, (3, 48, 3, 4, 1))]
    ws = torch.empty(max(L.s3g_deform_infer_workspace_bytes(C.byref(d)), 4) // 4, dtype=torch.float32, device=dev)

    # (host time counts here: a render is a dozen launches long.  Parameters are read where they are -- no detach(), one check each)
    w, gw = _Params(), _GeomParams()
    lin = feature_out[0]
    if tuple(lin.weight.shape) != (64, 128):
        raise RuntimeError(f"deform_infer_heads: feature_out must be Linear(128, 64), got weight {tuple(lin.weight.shape)}")
    slots = [(w, "W0", lin.weight), (w, "b0", lin.bias)]
    for struct, names, m in ((w, ("P1", "pb1", "P2", "pb2"), pos_deform), (w, ("S1", "sb1", "S2", "sb2"), shs_deform),
                             (gw, ("C1", "cb1", "C2", "cb2"), geometry[0]), (gw, ("R1", "rb1", "R2", "rb2"), geometry[1]),
                             (gw, ("O1", "ob1", "O2", "ob2"), geometry[2])):
        if m is not None:      # the four tensors of a present head; an absent head's slots stay NULL (never read)
            l1, l2 = m[1], m[3]
            slots += [(struct, names[0], l1.weight), (struct, names[1], l1.bias), (struct, names[2], l2.weight), (struct, names[3], l2.bias)]
    for struct, n, t in slots:
        if t.dtype != torch.float32 or t.device != dev or not t.is_contiguous():
            raise RuntimeError(f"deform_infer_heads: parameter {n} must be a contiguous float32 tensor on {dev}, got {t.dtype} on {t.device}")
        setattr(struct, n, t.data_ptr())
    ptr = lambda t: t.data_ptr() if t is not None else None
    with _lib.on_device(dev):
        _lib.check(L.s3g_deform_infer_heads(C.byref(d), C.byref(w), C.byref(gw), P, xyz_c.data_ptr(), t_c.data_ptr(), ptr(order),
                                            ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), ptr(outs[3]), ptr(outs[4]), ws.data_ptr(),
                                            _lib.stream_ptr()))
    return tuple(outs)


def deform_mlp(features, feature_out, pos_deform, shs_deform, dino_head, need_feat=True, need_dx=True, need_dshs=True):
    """features [P,128] -> (dx [P,3], dshs [P,48], feat [P,3]) with the reference's Sequential modules as parameter
    holders (feature_out = Sequential(Linear); heads = Sequential(ReLU, Linear, ReLU, Linear); dino = Sequential(Linear,
    ReLU, Linear, ReLU, Linear)).
    need_dx=False (static scenes, ModelHiddenParams no_dx=True): the position head is skipped in every kernel, dx is None, and
    pos_deform's parameters are not inputs of the autograd node -- their .grad stays None, as the reference's autograd leaves it
    when scene/deformation.py:119-121 never calls the head (Adam then neither decays their moments nor counts a step).
    need_dshs=False (no_dshs=True): the same for the SH head -- dshs is None, shs_deform's four parameters are not inputs of the node.
    These calls run the chain kernels without the SH head (exact fp32 in every arithmetic mode, csrc/mlp_heads.hip).
    dino_head=None (feat_head=False: the network has no such module): feat is None under autograd too; the library is handed one shared
    zero block for the head's weight slots and NULL for their gradients.
    need_feat=False is honoured only when no backward follows.  Nothing to compute -- no dx, no dshs and no feat wanted or possible --
    means no launch: (None, None, None)."""
    ps = _head_params(feature_out, pos_deform, shs_deform, dino_head)
    grad_mode = torch.is_grad_enabled()
    if need_dx and need_dshs and dino_head is not None:
        return _DeformMLP.apply(features, need_feat, grad_mode, None, *ps)
    will_feat = dino_head is not None and (bool(need_feat) or (grad_mode and (features.requires_grad or any(p.requires_grad for p in ps if p is not None))))
    if not (need_dx or need_dshs or will_feat):
        return None, None, None
    fill = [None] * 16
    for sl, skipped in ((_POS, not need_dx), (_SHS, not need_dshs)):
        if skipped:
            fill[sl] = [p.detach() for p in ps[sl]]
    if dino_head is None:
        fill[_DINO] = _zero_dino(features.device)
    return _DeformMLP.apply(features, need_feat, grad_mode, tuple(fill), *(p for p, f in zip(ps, fill) if f is None))
