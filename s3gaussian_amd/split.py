"""The dynamic / static point-cloud split on the MI355X library (include/s3g_split.h): the motion classification of the reference's
`GaussianModel.save_ply_split` (scene/gaussian_model.py:277-348) and of its "dynamic point" counter (train.py:445-452), and the PLY
vertex table of `save_ply` / `save_ply_split` (:258-275, :304-348) built in one launch.

    motion_classify(dx)        mask = max|dx| > mean(max|dx|), the threshold and the count, all left on the device
    pack_ply_rows(...)         [x y z | 0 0 0 | f_dc | f_rest channel-major | opacity | scale | rot] rows: the whole table, or the
                               dynamic and the static table of a mask, each in source order (np.where(mask) / np.where(~mask))
    export_split(pc, dx, ...)  both files of save_ply_split through plyio.write_vertices

The threshold is the float64 sum of the fp32 maxima divided by P and rounded to fp32 once, in an order fixed by P alone; destination
rows come from an exclusive scan, never from atomic counters: every output is bit-reproducible.  GPU only: CPU tensors are refused
(no fallback on the product path)."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib

BLOCK = 256
SH_REST = (0, 3, 8, 15)      # rows of f_rest at SH degree 0..3

calls = 0                    # classify / pack calls that reached the library (tests, tools/split_ab.py)


class _Stats(C.Structure):
    """struct s3g_split_stats (include/s3g_split.h)."""
    _fields_ = [("thre", C.c_float), ("n_dynamic", C.c_uint32)]


class _PackPlan(C.Structure):
    """struct s3g_split_pack_plan (include/s3g_split.h)."""
    _fields_ = [("P", C.c_int), ("sh_rest", C.c_int), ("rows_a", C.c_int), ("rows_b", C.c_int), ("xyz", C.c_void_p),
                ("dx", C.c_void_p), ("f_dc", C.c_void_p), ("f_rest", C.c_void_p), ("opacity", C.c_void_p), ("scaling", C.c_void_p),
                ("rotation", C.c_void_p), ("mask", C.c_void_p), ("block_offsets", C.c_void_p), ("out_a", C.c_void_p),
                ("out_b", C.c_void_p)]


_L = None


def _bind():
    global _L
    if _L is None:
        L = _lib.lib()
        if not hasattr(L, "s3g_split_pack_rows"):
            raise ImportError(f"{_lib.LIB_PATH} has no s3g_split_pack_rows: it was built from an older tree: rebuild")
        vp, i = C.c_void_p, C.c_int
        L.s3g_split_count_words.restype = C.c_size_t
        L.s3g_split_count_words.argtypes = [i]
        L.s3g_split_workspace_bytes.restype = C.c_size_t
        L.s3g_split_workspace_bytes.argtypes = [i]
        L.s3g_split_classify.restype = i
        L.s3g_split_classify.argtypes = [i, vp, vp, vp, vp, vp, vp]
        L.s3g_split_mask_offsets.restype = i
        L.s3g_split_mask_offsets.argtypes = [i, vp, vp, vp, vp]
        L.s3g_split_pack_rows.restype = i
        L.s3g_split_pack_rows.argtypes = [C.POINTER(_PackPlan), vp]
        _L = L
    return _L


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def _dense(t: torch.Tensor) -> torch.Tensor:
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    return t if t.is_contiguous() else t.contiguous()


def row_width(sh_rest: int) -> int:
    """Floats per vertex row: 17 + 3 R (62 at SH degree 3)."""
    if sh_rest not in SH_REST:
        raise ValueError(f"split.row_width: f_rest has {sh_rest} rows per Gaussian; SH degrees 0..3 have {SH_REST}")
    return 17 + 3 * sh_rest


@torch.no_grad()
def motion_classify(dx: torch.Tensor, return_offsets: bool = False):
    """-> (mask bool [P], thre 0-dim float32 tensor, n_dynamic 0-dim int32 tensor), all on dx's device; nothing here waits for it.
    mask[i] = max(|dx[i]|) > thre, thre = mean_i max(|dx[i]|) (float64 sum rounded to fp32 once).
    return_offsets: also the scanned per-block counts pack_ply_rows takes as `offsets` (int32 [ceil(P / 256) + 1]: word b = dynamic
    Gaussians in front of block b, the last word = n_dynamic).
    P = 0 gives an empty mask, a NaN threshold (the mean of nothing) and 0."""
    global calls
    if not (torch.is_tensor(dx) and dx.is_cuda):
        where = dx.device if torch.is_tensor(dx) else type(dx).__name__
        raise RuntimeError(f"split.motion_classify: dx must live on the GPU (got {where}); no CPU fallback")
    if dx.dim() != 2 or dx.shape[1] != 3:
        raise RuntimeError("split.motion_classify expects dx of shape [P,3]")
    L = _bind()
    dev = dx.device
    d = _dense(dx)
    P = d.shape[0]
    mask = torch.empty(P, dtype=torch.uint8, device=dev)
    offsets = torch.zeros(int(L.s3g_split_count_words(P)), dtype=torch.int32, device=dev) if P == 0 else \
        torch.empty(int(L.s3g_split_count_words(P)), dtype=torch.int32, device=dev)
    stats = torch.zeros(2, dtype=torch.int32, device=dev)
    if P == 0:
        stats[:1].view(torch.float32).fill_(float("nan"))
    else:
        work = torch.empty(int(L.s3g_split_workspace_bytes(P)), dtype=torch.uint8, device=dev)
        with _lib.on_device(dev):
            _lib.check(L.s3g_split_classify(P, d.data_ptr(), mask.data_ptr(), offsets.data_ptr(), stats.data_ptr(), work.data_ptr(),
                                            _lib.stream_ptr()))
        calls += 1
    out = (mask.view(torch.bool), stats[:1].view(torch.float32)[0], stats[1])
    return out + (offsets,) if return_offsets else out


def _mask_offsets(L, mask_u8: torch.Tensor) -> torch.Tensor:
    P, dev = mask_u8.shape[0], mask_u8.device
    offsets = torch.empty(int(L.s3g_split_count_words(P)), dtype=torch.int32, device=dev)
    with _lib.on_device(dev):
        _lib.check(L.s3g_split_mask_offsets(P, mask_u8.data_ptr(), offsets.data_ptr(), None, _lib.stream_ptr()))
    return offsets


@torch.no_grad()
def pack_ply_rows(xyz, f_dc, f_rest, opacity, scaling, rotation, dx=None, mask=None, offsets=None, out=None):
    """The reference's vertex table, rows of W = 17 + 3 R floats: [x y z | 0 0 0 | f_dc | f_rest [3,R] | opacity | scale | rot].

    xyz [P,3], f_dc [P,1,3], f_rest [P,R,3] (R = 0, 3, 8, 15), opacity [P,1], scaling [P,3], rotation [P,4]: float tensors on the GPU
    (made contiguous fp32 here).  dx [P,3] or None: x y z = xyz + dx.
    mask None -> rows [P, W] in source order.
    mask bool / uint8 [P] -> (dynamic_rows [n_dynamic, W], static_rows [P - n_dynamic, W]), each in source order.  offsets: the
    fourth value of motion_classify(dx, return_offsets=True) FOR THIS MASK (computed from the mask here when None).  The mask case
    reads n_dynamic back once, 4 bytes, to size the two tables.
    out: the output tensor (no mask) or pair of tensors (mask) to write into: contiguous fp32 on the same device with at least the
    rows needed; views of their leading rows are returned."""
    global calls
    named = (("xyz", xyz, 3), ("f_dc", f_dc, 3), ("f_rest", f_rest, None), ("opacity", opacity, 1), ("scaling", scaling, 3),
             ("rotation", rotation, 4))
    for name, t, _ in named:
        if not (torch.is_tensor(t) and t.is_cuda):
            where = t.device if torch.is_tensor(t) else type(t).__name__
            raise RuntimeError(f"split.pack_ply_rows: {name} must live on the GPU (got {where}); no CPU fallback")
    dev = xyz.device
    P = int(xyz.shape[0])
    if f_rest.dim() != 3 or (f_rest.shape[1] != 0 and f_rest.shape[2] != 3):
        raise RuntimeError("split.pack_ply_rows: f_rest must be [P,R,3]")
    R = int(f_rest.shape[1])
    W = row_width(R)
    dense = {}
    for name, t, width in named:
        width = 3 * R if width is None else width
        if t.device != dev or t.shape[0] != P or t.numel() != P * width:
            raise RuntimeError(f"split.pack_ply_rows: {name} has shape {tuple(t.shape)}; expected {P} rows of {width} floats on {dev}")
        dense[name] = _dense(t)
    if dx is not None:
        if not (torch.is_tensor(dx) and dx.is_cuda and dx.device == dev and tuple(dx.shape) == (P, 3)):
            raise RuntimeError(f"split.pack_ply_rows: dx must be a [{P},3] tensor on {dev}")
        dx = _dense(dx)
    L = _bind()
    n_dynamic = None
    mask_u8 = None
    if mask is not None:
        if not (torch.is_tensor(mask) and mask.is_cuda and mask.device == dev and tuple(mask.shape) == (P,)
                and mask.dtype in (torch.bool, torch.uint8)):
            raise RuntimeError(f"split.pack_ply_rows: mask must be a bool or uint8 [{P}] tensor on {dev}")
        mask_u8 = mask.contiguous()
        mask_u8 = mask_u8.view(torch.uint8) if mask_u8.dtype == torch.bool else mask_u8
        words = int(L.s3g_split_count_words(P))
        if offsets is None:
            offsets = _mask_offsets(L, mask_u8) if P > 0 else torch.zeros(words, dtype=torch.int32, device=dev)
        elif not (torch.is_tensor(offsets) and offsets.is_cuda and offsets.device == dev and offsets.dtype == torch.int32
                  and tuple(offsets.shape) == (words,) and offsets.is_contiguous()):
            raise RuntimeError(f"split.pack_ply_rows: offsets must be the contiguous int32 [{words}] tensor of motion_classify")
        n_dynamic = int(offsets[-1].item())              # the one host read: sizes the two tables
        if not 0 <= n_dynamic <= P:
            raise RuntimeError(f"split.pack_ply_rows: the offsets count {n_dynamic} dynamic rows of {P}")
    elif offsets is not None:
        raise RuntimeError("split.pack_ply_rows: offsets without a mask")
    need = (P,) if mask is None else (n_dynamic, P - n_dynamic)
    if out is None:
        outs = [torch.empty((n, W), dtype=torch.float32, device=dev) for n in need]
    else:
        outs = [out] if mask is None else list(out)
        if len(outs) != len(need):
            raise RuntimeError("split.pack_ply_rows: out must be one tensor without a mask and a pair with one")
        for o, n in zip(outs, need):
            if not (torch.is_tensor(o) and o.is_cuda and o.device == dev and o.dtype == torch.float32 and o.dim() == 2
                    and o.shape[1] == W and o.shape[0] >= n and o.is_contiguous()):
                raise RuntimeError(f"split.pack_ply_rows: out must hold contiguous fp32 [>= {n}, {W}] on {dev}")
        outs = [o[:n] for o, n in zip(outs, need)]
    if P > 0:
        plan = _PackPlan(P, R, need[0], need[1] if mask is not None else 0, _ptr(dense["xyz"]), _ptr(dx), _ptr(dense["f_dc"]), _ptr(dense["f_rest"]), _ptr(dense["opacity"]),
                         _ptr(dense["scaling"]), _ptr(dense["rotation"]), _ptr(mask_u8), _ptr(offsets) if mask is not None else None,
                         _ptr(outs[0]), _ptr(outs[1]) if mask is not None else None)
        with _lib.on_device(dev):
            _lib.check(L.s3g_split_pack_rows(C.byref(plan), _lib.stream_ptr()))
        calls += 1
    return outs[0] if mask is None else (outs[0], outs[1])


def model_rows(pc, dx=None, mask=None, offsets=None):
    """pack_ply_rows on a model's tensors (GaussianParams or the reference's GaussianModel: the attribute names are the same)."""
    return pack_ply_rows(pc._xyz, pc._features_dc, pc._features_rest, pc._opacity, pc._scaling, pc._rotation, dx=dx, mask=mask,
                         offsets=offsets)


@torch.no_grad()
def export_split(pc, dx: torch.Tensor, dynamic_pcd_path: str, static_pcd_path: str):
    """Both files of save_ply_split for the displacement dx [P,3]: classify -> one host read -> pack -> two device-to-host copies.
    The model is not modified.  -> {"n_dynamic", "n_static", "thre": 0-dim device tensor}."""
    from .plyio import write_vertices
    if not (torch.is_tensor(dx) and dx.is_cuda and pc._xyz.is_cuda):
        raise RuntimeError("split.export_split: the model and dx must live on the GPU; no CPU fallback")
    if tuple(dx.shape) != tuple(pc._xyz.shape):
        raise RuntimeError(f"split.export_split: dx has shape {tuple(dx.shape)}, the model has {tuple(pc._xyz.shape)}")
    dx = _dense(dx.to(pc._xyz.device))
    mask, thre, _, offsets = motion_classify(dx, return_offsets=True)
    dynamic, static = model_rows(pc, dx=dx, mask=mask, offsets=offsets)
    names = pc.construct_list_of_attributes()
    write_vertices(dynamic_pcd_path, names, dynamic.cpu().numpy())
    write_vertices(static_pcd_path, names, static.cpu().numpy())
    return {"n_dynamic": int(dynamic.shape[0]), "n_static": int(static.shape[0]), "thre": thre}
