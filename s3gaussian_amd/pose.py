"""Camera pose refinement: a six-parameter correction per camera in front of the rasterizer's camera gradients
(include/s3g_camera.h).

delta = (omega, tau) is a left perturbation in the camera frame, x_cam' = Exp(omega) x_cam + tau.  `apply_pose_delta` maps it
onto the camera's three tensors (viewmatrix, projmatrix, campos) with one single-workgroup kernel each way; the rasterizer nodes
(rasterizer.py) and the render glue (glue.py) return gradients for those tensors when they require one, so a loss on a render
back-propagates to delta.  `PoseRefiner` keeps one delta per camera and its optimizer.

A batch of cameras (a rig's cameras of one timestamp) is served too: `PoseRefiner.corrected_views` maps V corrections onto V
cameras with one launch each way (s3g_pose_apply_views / _backward_views, bit-identical per camera to the single-camera map),
pipeline.render_views / training_step_views take `pose=` and `cam_indices=`, and the shared glue pass returns every view's own
camera-centre gradient (glue.activations_and_colors_views(campos_grad=True)).  A camera whose tensors the CALLER made require a
gradient is still refused by the multi-view routes, by name.

Not served, and refused by name: pose refinement together with a sky model (skymodel: its directions take host camera values)
and under the data-parallel wrapper (dp).
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import torch
from torch import nn

from . import _lib


def _f32_16(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"pose: {name} must live on the GPU (got {t.device}); no CPU fallback")
    if t.dtype != torch.float32 or t.numel() != 16:
        raise RuntimeError(f"pose: {name} must be a float32 4 x 4 matrix, got {t.dtype} {tuple(t.shape)}")
    return t.detach().contiguous()


class _ApplyPose(torch.autograd.Function):
    @staticmethod
    def forward(ctx, delta6, view0, proj0):
        if delta6.dtype != torch.float64 or delta6.numel() != 6:
            raise RuntimeError(f"apply_pose_delta: delta6 must be six float64 values, got {delta6.dtype} {tuple(delta6.shape)}")
        view0, proj0 = _f32_16(view0, "viewmatrix"), _f32_16(proj0, "projmatrix")
        if delta6.device != view0.device:
            raise RuntimeError(f"apply_pose_delta: delta6 is on {delta6.device}, the camera on {view0.device}")
        d = delta6.detach().contiguous()
        dev = view0.device
        view = torch.empty((4, 4), dtype=torch.float32, device=dev)
        proj = torch.empty((4, 4), dtype=torch.float32, device=dev)
        campos = torch.empty(3, dtype=torch.float32, device=dev)
        L = _lib.lib()
        with _lib.on_device(dev):
            _lib.check(L.s3g_pose_apply(d.data_ptr(), view0.data_ptr(), proj0.data_ptr(), view.data_ptr(), proj.data_ptr(),
                                        campos.data_ptr(), _lib.stream_ptr()))
        ctx.save_for_backward(d, view0, proj0)
        ctx.delta_shape = delta6.shape
        ctx.set_materialize_grads(False)
        return view, proj, campos

    @staticmethod
    def backward(ctx, g_view, g_proj, g_campos):
        d, view0, proj0 = ctx.saved_tensors
        dev = d.device
        g35 = torch.zeros(35, dtype=torch.float64, device=dev)
        for lo, hi, g in ((0, 16, g_view), (16, 32, g_proj), (32, 35, g_campos)):
            if g is not None:
                g35[lo:hi] = g.reshape(-1)
        out = torch.empty(6, dtype=torch.float64, device=dev)
        L = _lib.lib()
        with _lib.on_device(dev):
            _lib.check(L.s3g_pose_apply_backward(d.data_ptr(), view0.data_ptr(), proj0.data_ptr(), g35.data_ptr(), out.data_ptr(),
                                                 _lib.stream_ptr()))
        return out.view(ctx.delta_shape), None, None


class _ApplyPoseViews(torch.autograd.Function):
    """_ApplyPose for V cameras in one launch each way: delta [N,6], rows [V] int32 (distinct), view0s / proj0s [V,4,4] ->
    views [V,4,4], projs [V,4,4], camposs [V,3].  The gradient of delta has rows `rows` filled and exact zeros elsewhere."""

    @staticmethod
    def forward(ctx, delta, rows, view0s, proj0s):
        d = delta.detach().contiguous()
        V, dev = rows.shape[0], d.device
        views = torch.empty((V, 4, 4), dtype=torch.float32, device=dev)
        projs = torch.empty((V, 4, 4), dtype=torch.float32, device=dev)
        camposs = torch.empty((V, 3), dtype=torch.float32, device=dev)
        L = _lib.lib()
        with _lib.on_device(dev):
            _lib.check(L.s3g_pose_apply_views(V, d.data_ptr(), rows.data_ptr(), view0s.data_ptr(), proj0s.data_ptr(), views.data_ptr(),
                                              projs.data_ptr(), camposs.data_ptr(), _lib.stream_ptr()))
        ctx.save_for_backward(d, rows, view0s, proj0s)
        ctx.set_materialize_grads(False)
        return views, projs, camposs

    @staticmethod
    def backward(ctx, g_views, g_projs, g_camposs):
        d, rows, view0s, proj0s = ctx.saved_tensors
        V, dev = rows.shape[0], d.device
        g35 = torch.zeros((V, 35), dtype=torch.float64, device=dev)
        for lo, hi, g in ((0, 16, g_views), (16, 32, g_projs), (32, 35, g_camposs)):
            if g is not None:
                g35[:, lo:hi] = g.reshape(V, hi - lo)
        g_rows = torch.empty((V, 6), dtype=torch.float64, device=dev)
        L = _lib.lib()
        with _lib.on_device(dev):
            _lib.check(L.s3g_pose_apply_backward_views(V, d.data_ptr(), rows.data_ptr(), view0s.data_ptr(), proj0s.data_ptr(),
                                                       g35.data_ptr(), g_rows.data_ptr(), _lib.stream_ptr()))
        out = torch.zeros_like(d)
        out.index_copy_(0, rows.long(), g_rows)     # rows are distinct (corrected_views refuses repeats): a copy, no sum, no order
        return out, None, None, None


def apply_pose_delta(delta6: torch.Tensor, cam: Dict) -> Dict:
    """-> a copy of the camera dict `cam` whose viewmatrix, projmatrix and campos are those of the camera moved by
    delta6 = (omega, tau) (float64 [6], on the camera's device); the other fields are shared.  Differentiable in delta6."""
    view, proj, campos = _ApplyPose.apply(delta6, cam["viewmatrix"], cam["projmatrix"])
    out = dict(cam)
    out.update(viewmatrix=view, projmatrix=proj, campos=campos)
    return out


def camera_requires_grad(cam: Dict) -> bool:
    return any(torch.is_tensor(cam.get(k)) and cam[k].requires_grad for k in ("viewmatrix", "projmatrix", "campos"))


class PoseRefiner:
    """One correction per camera: `delta` [N,6] float64, zeros at the start (every camera where its calibration put it).
    The optimizer is torch.optim.Adam: the project's optim.Adam handles float32 parameters only.  `lr` has no default.
    Adam is dense over the whole [N,6] parameter: a step taken for camera j also moves every camera i that still carries momentum
    from its earlier views (by lr * m_i / sqrt(v_i), with m_i and v_i decaying), as torch's Adam does for any row without a
    gradient.  With a learning-rate schedule or many cameras per log, keep that in mind when reading a trajectory.
    A plain object, not an nn.Module: it owns its optimizer, and state_dict() / load_state_dict() carry both in one format."""

    def __init__(self, n_cameras: int, device, lr: float):
        from . import dp
        if dp.active():
            raise RuntimeError("PoseRefiner: pose refinement under the data-parallel wrapper (dp) is not served")
        self.delta = nn.Parameter(torch.zeros((int(n_cameras), 6), dtype=torch.float64, device=device))
        self.optimizer = torch.optim.Adam([self.delta], lr=float(lr))

    def corrected(self, cam: Dict, i: int) -> Dict:
        """The camera dict of camera `i` at its refined pose (differentiable in delta[i] under autograd)."""
        return apply_pose_delta(self.delta[int(i)], cam)

    def corrected_views(self, cams: Sequence[Dict], indices: Sequence[int]) -> List[Dict]:
        """corrected() for a batch: camera dicts `cams` as cameras `indices` of this refiner -> their dicts at the refined poses, in
        order.  One autograd node over one launch each way whatever the number of cameras; each camera's tensors are bit-identical
        to corrected(cam, i)'s, and so is the gradient that reaches delta: rows `indices` of delta.grad, exact zeros in every other
        row.  An index may appear once per call: two cameras on one row would have to be summed, in an order nothing fixes."""
        cams, idx = list(cams), [int(i) for i in indices]
        if len(cams) != len(idx):
            raise RuntimeError(f"PoseRefiner.corrected_views: {len(cams)} cameras, {len(idx)} indices")
        if len(set(idx)) != len(idx):
            raise RuntimeError(f"PoseRefiner.corrected_views: repeated camera indices {sorted(i for i in set(idx) if idx.count(i) > 1)} "
                               "in one call (their gradients would be summed in no fixed order); render such cameras in separate calls")
        N = self.delta.shape[0]
        if any(i < 0 or i >= N for i in idx):
            raise RuntimeError(f"PoseRefiner.corrected_views: camera indices {idx} outside 0 .. {N - 1}")
        if not cams:
            return []
        dev = self.delta.device
        view0s = torch.stack([_f32_16(cam["viewmatrix"], "viewmatrix").reshape(4, 4) for cam in cams])
        proj0s = torch.stack([_f32_16(cam["projmatrix"], "projmatrix").reshape(4, 4) for cam in cams])
        if view0s.device != dev:
            raise RuntimeError(f"PoseRefiner.corrected_views: delta is on {dev}, the cameras on {view0s.device}")
        rows = torch.tensor(idx, dtype=torch.int32, device=dev)
        views, projs, camposs = _ApplyPoseViews.apply(self.delta, rows, view0s, proj0s)
        out = []
        for v, cam in enumerate(cams):
            c = dict(cam)
            c.update(viewmatrix=views[v], projmatrix=projs[v], campos=camposs[v])
            out.append(c)
        return out

    def step(self) -> None:
        """Optimizer step and gradients cleared: what pipeline.training_step does beside the model's own step."""
        if self.delta.grad is not None:
            self.optimizer.step()
        self.optimizer.zero_grad(set_to_none=True)

    @torch.no_grad()
    def poses(self, cameras) -> torch.Tensor:
        """-> [N,4,4] float32: the corrected world-to-camera matrices (column-vector convention, x_cam = M x_world) of
        `cameras`, one dict per refined camera, for export."""
        if len(cameras) != self.delta.shape[0]:
            raise RuntimeError(f"PoseRefiner.poses: {len(cameras)} cameras for {self.delta.shape[0]} corrections")
        return torch.stack([self.corrected(cam, i)["viewmatrix"].t() for i, cam in enumerate(cameras)])

    def state_dict(self) -> Dict:
        """{"delta": [N,6] float64 copy, "optimizer": the Adam state}."""
        return {"delta": self.delta.detach().clone(), "optimizer": self.optimizer.state_dict()}

    def load_state_dict(self, state: Dict) -> None:
        """Takes what state_dict() returned; a missing key or another number of cameras is an error."""
        delta = state["delta"]
        if tuple(delta.shape) != tuple(self.delta.shape):
            raise RuntimeError(f"PoseRefiner.load_state_dict: delta is {tuple(delta.shape)}, this refiner holds {tuple(self.delta.shape)}")
        with torch.no_grad():
            self.delta.copy_(delta.to(self.delta.device, torch.float64))
        self.optimizer.load_state_dict(state["optimizer"])
