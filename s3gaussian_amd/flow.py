"""Scene-flow colours on the MI355X: the per-Gaussian RGB of the reference's forward / backward flow images
(utils/video_utils.py:252-299: `flow_visualizer(dx_b - dx_a)` = utils/visualization_tools.py::scene_flow_to_rgb with the bright
background and radius 1) from a min / max reduction and one per-Gaussian kernel (include/s3g_flow.h), and the order in which that loop
pairs the frames (`frame_plan`).  pipeline.render_flows puts the two together."""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Tuple

import torch

from . import _lib

evaluations = 0      # scene_flow_colors calls that reached the library (tests, tools/flow_ab.py)

_bound = False


def _bind():
    global _bound
    L = _lib.lib()
    if not _bound:
        vp = C.c_void_p
        L.s3g_scene_flow_workspace_bytes.restype = C.c_size_t
        L.s3g_scene_flow_workspace_bytes.argtypes = [C.c_int]
        L.s3g_scene_flow_colors.restype = C.c_int
        L.s3g_scene_flow_colors.argtypes = [C.c_int, vp, vp, vp, vp, vp, vp]
        _bound = True
    return L


def scene_flow_colors(dx_a: torch.Tensor, dx_b: torch.Tensor, out=None, return_range: bool = False):
    """Colours [P,3] (fp32, in [0,1]) of the flow dx_b - dx_a, the reference's `flow_visualizer(dx_b - dx_a)` without its trip
    through the host.

    dx_a, dx_b: [P,3] on the GPU, any strides and float dtype (made contiguous fp32 here).
    out: a contiguous fp32 [P,3] tensor on the same device, written in place and returned.
    return_range: also return a 2-element device tensor {min, max} of the fp32 difference (what step 1 normalises with).
    P = 0 gives an empty tensor (and a NaN range).  Nothing here waits for the device."""
    global evaluations
    if not (torch.is_tensor(dx_a) and dx_a.is_cuda and torch.is_tensor(dx_b) and dx_b.is_cuda):
        where = dx_a.device if torch.is_tensor(dx_a) else type(dx_a).__name__
        raise RuntimeError(f"scene_flow_colors: dx_a and dx_b must live on the GPU (got {where}); no CPU fallback")
    if dx_a.dim() != 2 or dx_a.shape[1] != 3 or dx_b.shape != dx_a.shape:
        raise RuntimeError("scene_flow_colors expects dx_a and dx_b of shape [P,3]")
    L = _bind()
    dev = dx_a.device
    a, b = dx_a.detach().float().contiguous(), dx_b.detach().to(dev).float().contiguous()
    P = a.shape[0]
    if out is None:
        out = torch.empty((P, 3), dtype=torch.float32, device=dev)
    elif not (out.is_cuda and out.device == dev and out.dtype == torch.float32 and tuple(out.shape) == (P, 3) and out.is_contiguous()):
        raise RuntimeError("scene_flow_colors: out must be a contiguous fp32 [P,3] tensor on the inputs' device")
    rng = None
    if return_range:
        rng = (torch.full((2,), float("nan"), dtype=torch.float32, device=dev) if P == 0
               else torch.empty(2, dtype=torch.float32, device=dev))
    if P != 0:
        work = torch.empty(max(int(L.s3g_scene_flow_workspace_bytes(P)), 1), dtype=torch.uint8, device=dev)
        with _lib.on_device(dev):
            _lib.check(L.s3g_scene_flow_colors(P, a.data_ptr(), b.data_ptr(), out.data_ptr(), None if rng is None else rng.data_ptr(),
                                               work.data_ptr(), _lib.stream_ptr()))
        evaluations += 1
    return (out, rng) if return_range else out


class FlowFrame(NamedTuple):
    """One image of the forward or backward list: painted with C(dx[to_frame] - dx[from_frame]), rendered at its own frame.
    edge_copy: the reference fills this slot with the other list's image of the same frame (the first `num_cams` backward and the
    last `num_cams` forward images), which is what the pair says, too."""
    from_frame: int
    to_frame: int
    edge_copy: bool


def frame_plan(n_frames: int, num_cams: int = 3) -> Tuple[List[FlowFrame], List[FlowFrame]]:
    """(forward, backward): for each of the n_frames frames, in dataset order (num_cams cameras per timestamp), the pair of frames
    whose dx difference colours its forward and its backward flow image (utils/video_utils.py:252-299):

      forward[t]  = (t, t + n)   for t <  N - n        backward[t] = (t - n, t)   for t >= n
      forward[t]  = backward[t]  for t >= N - n        backward[t] = forward[t]   for t <  n      (edge copies)

    At num_cams = 3 -- the only value at which the reference's own loop is self-consistent: its fix-ups for the first and last three
    frames are hard-coded -- this is the reference's result list for list; other values follow the same formulas.
    N < 2 * num_cams (no frame would have both neighbours' worth of pairs) and num_cams < 1 raise ValueError."""
    N, n = int(n_frames), int(num_cams)
    if n < 1:
        raise ValueError(f"frame_plan: num_cams = {num_cams}")
    if N < 2 * n:
        raise ValueError(f"frame_plan: {N} frames are fewer than 2 * num_cams = {2 * n}")
    forward = [FlowFrame(t, t + n, False) if t < N - n else FlowFrame(t - n, t, True) for t in range(N)]
    backward = [FlowFrame(t - n, t, False) if t >= n else FlowFrame(t, t + n, True) for t in range(N)]
    return forward, backward
