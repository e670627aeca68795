"""Coloured depth frames on the MI355X: the reference's depth_visualizer (utils/video_utils.py:27-33) --
`visualize_depth(frame, opacity, lo, hi, depth_curve_fn=-log(x + 1e-6))` of utils/visualization_tools.py:117-194: turbo map, log curve,
opacity weighting -- written as uint8 into one camera's tile of a strip (frames.py), and the opacity-weighted 0.5 / 99.5 percentiles
visualize_cmap takes its bounds from when lo or hi is None, selected on the device (include/s3g_depthvis.h).  The reference carries
the call commented out in both of its video writers because its renderer returns no opacity image; render(..., return_alpha=True)
does.  pipeline.evaluate_video(depth_keys=("depth_colors",)) puts this behind one render per camera."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib

MAX_PIXELS = 1 << 23     # S3G_DEPTHVIS_MAX_PIXELS: the weight sums stay exact in a double up to there
LAUNCHES_PERCENTILES = 10  # four digit passes of two kernels each, the last pass, the interpolation
LAUNCHES_COLORS = 1

calls = 0                # depth_colors calls that reached the library (tests, tools/depthvis_ab.py)

_bound = False
_table = None


def _bind():
    global _bound
    L = _lib.lib()
    if not _bound:
        vp = C.c_void_p
        L.s3g_depthvis_workspace_bytes.restype = C.c_size_t
        L.s3g_depthvis_workspace_bytes.argtypes = [C.c_int, C.c_int]
        L.s3g_depth_percentiles.restype = C.c_int
        L.s3g_depth_percentiles.argtypes = [C.c_int, C.c_int, vp, vp, vp, vp, vp]
        L.s3g_depth_colors.restype = C.c_int
        L.s3g_depth_colors.argtypes = [C.c_int, C.c_int, vp, vp, C.c_double, C.c_double, vp, vp, C.c_longlong, C.c_int, vp]
        L.s3g_depth_turbo_table.restype = C.POINTER(C.c_ubyte * 768)
        L.s3g_depth_turbo_table.argtypes = []
        _bound = True
    return L


def __getattr__(name):
    """TABLE: the library's [256, 3] uint8 turbo table (matplotlib's, through to8b) as a numpy array, read on first use; no GPU."""
    global _table
    if name == "TABLE":
        if _table is None:
            import numpy as np
            _table = np.array(_bind().s3g_depth_turbo_table().contents, dtype=np.uint8).reshape(256, 3)
            _table.setflags(write=False)
        return _table
    raise AttributeError(name)


def _plane(name, t, like=None):
    if not (torch.is_tensor(t) and t.is_cuda):
        where = t.device if torch.is_tensor(t) else type(t).__name__
        raise RuntimeError(f"depthvis: {name} must live on the GPU (got {where}); no CPU fallback")
    if not (t.dim() == 2 or (t.dim() == 3 and t.shape[0] == 1)) or t.numel() < 1:
        raise RuntimeError(f"depthvis: {name} must have shape [H,W] or [1,H,W] (got {tuple(t.shape)})")
    if like is not None and (tuple(t.shape[-2:]) != tuple(like.shape[-2:]) or t.device != like.device):
        raise RuntimeError(f"depthvis: {name} has shape {tuple(t.shape)} on {t.device}; the depth has {tuple(like.shape)} on {like.device}")
    return t.detach().float().contiguous()


def _percentiles(L, d, a, H, W):
    if H * W > MAX_PIXELS:
        raise RuntimeError(f"depthvis: {H} x {W} pixels; the weighted percentiles take at most 2^23 (exact integer sums in a double)")
    out = torch.empty(2, dtype=torch.float64, device=d.device)
    work = torch.empty(max(int(L.s3g_depthvis_workspace_bytes(H, W)), 8) // 8, dtype=torch.int64, device=d.device)
    with _lib.on_device(d.device):
        _lib.check(L.s3g_depth_percentiles(H, W, d.data_ptr(), a.data_ptr(), out.data_ptr(), work.data_ptr(), _lib.stream_ptr()))
    return out


def weighted_percentiles(depth: torch.Tensor, alpha: torch.Tensor) -> torch.Tensor:
    """The opacity-weighted 0.5 and 99.5 percentiles of a depth image as a float64 [2] tensor on the device: np.interp over the exact
    integer prefix sums of the weights llrint(clip(alpha, 0, 1) * 2^30) in ascending (depth, pixel index) order; NaN depths take no part
    (tests/depthvis_ref.py::weighted_percentiles, equal to the last bit).  Ten launches, nothing here waits for the device."""
    d = _plane("depth", depth)
    a = _plane("alpha", alpha, d)
    return _percentiles(_bind(), d, a, int(d.shape[-2]), int(d.shape[-1]))


def depth_colors(depth: torch.Tensor, alpha: Optional[torch.Tensor] = None, lo: Optional[float] = 4.0, hi: Optional[float] = 120.0,
                 out: Optional[torch.Tensor] = None, cam: int = 0, num_cams: int = 1) -> torch.Tensor:
    """out[:, cam * W:(cam + 1) * W, :] = to8b(visualize_depth(depth, alpha, lo, hi, depth_curve_fn=-log(x + 1e-6))) with the turbo map;
    every other byte of `out` is left alone.  depth: [H,W] or [1,H,W] on the GPU; alpha: the same shape, or None (no weighting; only
    with both bounds given).  lo / hi: a float, or None for the automatic bound -- the weighted 0.5 percentile minus 2^-23, the 99.5
    one plus 2^-23 -- which stays on the device (unlike the reference's `lo or ...`, a given 0.0 is a bound).  out: a contiguous uint8
    [H, num_cams * W, 3] tensor on the depth's device, or None for a new one (its other tiles uninitialised).  One launch, eleven
    with an automatic bound.  Returns `out`."""
    global calls
    d = _plane("depth", depth)
    a = None if alpha is None else _plane("alpha", alpha, d)
    H, W = int(d.shape[-2]), int(d.shape[-1])
    cam, num_cams = int(cam), int(num_cams)
    automatic = lo is None or hi is None
    if automatic and a is None:
        raise RuntimeError("depth_colors: an automatic bound is an opacity-weighted percentile: alpha=None needs both lo and hi")
    lo_v, hi_v = (float("nan") if v is None else float(v) for v in (lo, hi))
    if (lo is not None and lo_v != lo_v) or (hi is not None and hi_v != hi_v):
        raise RuntimeError("depth_colors: a NaN bound (None selects the automatic one)")
    if num_cams < 1 or not 0 <= cam < num_cams:
        raise RuntimeError(f"depth_colors: cam = {cam}, num_cams = {num_cams}")
    if out is None:
        out = torch.empty((H, num_cams * W, 3), dtype=torch.uint8, device=d.device)
    elif not (torch.is_tensor(out) and out.is_cuda and out.device == d.device and out.dtype == torch.uint8 and out.is_contiguous()
              and tuple(out.shape) == (H, num_cams * W, 3)):
        raise RuntimeError(f"depth_colors: out must be a contiguous uint8 [{H}, {num_cams * W}, 3] tensor on the depth's device")
    L = _bind()
    bounds = _percentiles(L, d, a, H, W) if automatic else None
    with _lib.on_device(d.device):
        _lib.check(L.s3g_depth_colors(H, W, d.data_ptr(), None if a is None else a.data_ptr(), lo_v, hi_v,
                                      None if bounds is None else bounds.data_ptr(), out.data_ptr(), num_cams * W * 3, cam * W,
                                      _lib.stream_ptr()))
    calls += 1
    return out
