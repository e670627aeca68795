"""The LiDAR scene set-up on the MI355X library (include/s3g_lidar.h): what the reference's `readWaymoInfo` does with its sweeps before
the first iteration (scene/dataset_readers.py:824-977) and its `GridSample3D` (:1102-1144).

    depth_maps(rows, l2w, w2c, K, H, W)   the [V,H,W] fp32 depth maps of one sweep for the V <= 8 cameras of its timestamp (:838-887):
                                          a pixel holds pix.z of the counted point with the highest source row, 0 where none lands
    LidarCloud(aabb, capacity, device)    .add(rows, l2w) appends the world points inside the aabb (:843-856, 909-911), no host read;
                                          .finish(voxel_size) is GridSample3D: one point per voxel label, ascending label order
    read_sweep, frustum_aabb, init_colors host helpers (:830-834, :752-779, :907 + 967)

The sweep stays the raw [N,10] fp32 table of the .bin file (the point in columns 3:6): uploaded once, used as it is.  Poses and
intrinsics are float64 HOST arrays and travel as kernel arguments.  All arithmetic is float64 in a fixed order without contraction;
the winner of a pixel is an integer atomicMax of the source row, destination rows come from scans: every output is bit-reproducible.

Two documented differences from the reference: the representative of a voxel label is its row with the lowest position in the
accumulated cloud (the reference: whichever row numpy's unstable argsort puts first), and the `num_pts` subset is drawn with
torch.randperm (the reference: np.random.choice; another stream).  GPU only: CPU tensors are refused (no fallback)."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib

MAX_CAMS = 8
BLOCK = 256
LABEL_LIMIT = 1 << 53        # labels are exact integers in the reference's float64 below this
SH_C0 = 0.28209479177387814

calls = 0                    # calls that reached the library (tests, tools/lidar_ab.py)


class _Sweep(C.Structure):
    """struct s3g_lidar_sweep (include/s3g_lidar.h)."""
    _fields_ = [("rows", C.c_void_p), ("N", C.c_int), ("row_stride", C.c_int), ("point_offset", C.c_int), ("reserved", C.c_int),
                ("x_min", C.c_double), ("x_max", C.c_double), ("l2w", C.c_double * 12)]


class _Cams(C.Structure):
    """struct s3g_lidar_cams (include/s3g_lidar.h)."""
    _fields_ = [("V", C.c_int), ("H", C.c_int), ("W", C.c_int), ("reserved", C.c_int), ("w2c", (C.c_double * 12) * MAX_CAMS),
                ("K", (C.c_double * 9) * MAX_CAMS)]


class _GridStats(C.Structure):
    """struct s3g_lidar_grid_stats (include/s3g_lidar.h)."""
    _fields_ = [("qmin", C.c_int64 * 3), ("b", C.c_int64 * 3)]


_L = None


def _bind():
    global _L
    if _L is None:
        L = _lib.lib()
        if not hasattr(L, "s3g_lidar_depth_maps"):
            raise ImportError(f"{_lib.LIB_PATH} has no s3g_lidar_depth_maps: it was built from an older tree: rebuild")
        vp, i, d = C.c_void_p, C.c_int, C.c_double
        L.s3g_lidar_depth_workspace_bytes.restype = C.c_size_t
        L.s3g_lidar_depth_workspace_bytes.argtypes = [i, i, i]
        L.s3g_lidar_depth_maps.restype = i
        L.s3g_lidar_depth_maps.argtypes = [C.POINTER(_Sweep), C.POINTER(_Cams), vp, vp, vp]
        L.s3g_lidar_count_words.restype = C.c_size_t
        L.s3g_lidar_count_words.argtypes = [i]
        L.s3g_lidar_cloud_add.restype = i
        L.s3g_lidar_cloud_add.argtypes = [C.POINTER(_Sweep), C.POINTER(d), vp, i, vp, vp, vp]
        L.s3g_lidar_grid_workspace_bytes.restype = C.c_size_t
        L.s3g_lidar_grid_workspace_bytes.argtypes = [i]
        L.s3g_lidar_grid_range.restype = i
        L.s3g_lidar_grid_range.argtypes = [i, vp, d, vp, vp, vp]
        L.s3g_lidar_grid_keys.restype = i
        L.s3g_lidar_grid_keys.argtypes = [i, vp, d, vp, vp, vp]
        L.s3g_lidar_grid_heads.restype = i
        L.s3g_lidar_grid_heads.argtypes = [i, vp, vp, vp]
        L.s3g_lidar_grid_gather.restype = i
        L.s3g_lidar_grid_gather.argtypes = [i, vp, vp, vp, vp, vp, i, vp]
        _L = L
    return _L


def _rigid(m, what: str) -> np.ndarray:
    """Rows 0..2 of a [4,4] or [3,4] transform as 12 float64, row-major."""
    a = np.asarray(m.detach().cpu().numpy() if torch.is_tensor(m) else m, dtype=np.float64)
    if a.shape not in ((4, 4), (3, 4)):
        raise ValueError(f"lidar: {what} must be a [4,4] or [3,4] matrix, got shape {a.shape}")
    return np.ascontiguousarray(a[:3]).reshape(12)


def _sweep(who: str, rows: torch.Tensor, l2w, x_range, point_offset: int) -> _Sweep:
    if not (torch.is_tensor(rows) and rows.is_cuda):
        where = rows.device if torch.is_tensor(rows) else type(rows).__name__
        raise RuntimeError(f"lidar.{who}: rows must live on the GPU (got {where}); no CPU fallback")
    if rows.dim() != 2 or rows.dtype != torch.float32 or not rows.is_contiguous():
        raise RuntimeError(f"lidar.{who}: rows must be a contiguous fp32 [N,stride] table (the raw sweep file, or [N,3] with point_offset=0)")
    N, stride = int(rows.shape[0]), int(rows.shape[1])
    if N >= 1 << 31:
        raise RuntimeError(f"lidar.{who}: {N} rows (< 2^31)")
    if point_offset < 0 or stride < point_offset + 3:
        raise RuntimeError(f"lidar.{who}: rows of {stride} floats cannot hold a point at columns {point_offset}:{point_offset + 3}")
    s = _Sweep(rows.data_ptr() if N > 0 else None, N, stride, int(point_offset), 0, float(x_range[0]), float(x_range[1]))
    s.l2w[:] = _rigid(l2w, "l2w").tolist()
    return s


@torch.no_grad()
def depth_maps(rows: torch.Tensor, l2w, w2c, K, H: int, W: int, x_range=(-2.0, 80.0), point_offset: int = 3,
               out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> [V,H,W] fp32 on rows' device: the depth maps of one sweep for the V cameras of its timestamp; nothing here waits for it.

    rows [N,stride] fp32 on the GPU, the point in columns point_offset:point_offset + 3.  l2w [4,4] (or [3,4]), w2c [V,4,4] (or
    [V,3,4]) = np.linalg.inv(c2w), K [V,3,3]: float64 host arrays.  A point counts iff x_range[0] < p.x < x_range[1], pix.z > 0 and
    0 <= u < W, 0 <= v < H; the pixel (int(v), int(u)) takes pix.z of the counted point with the highest row, rounded to fp32 once.
    out: a contiguous fp32 [V,H,W] tensor to write into; workspace: a contiguous int32 tensor of at least V H W words."""
    global calls
    s = _sweep("depth_maps", rows, l2w, x_range, point_offset)
    dev = rows.device
    w2c = np.asarray(w2c, dtype=np.float64)
    K = np.asarray(K, dtype=np.float64)
    if w2c.ndim != 3 or K.shape != (w2c.shape[0], 3, 3):
        raise ValueError(f"lidar.depth_maps: w2c must be [V,4,4] and K [V,3,3]; got {w2c.shape} and {K.shape}")
    V, H, W = int(w2c.shape[0]), int(H), int(W)
    if not 1 <= V <= MAX_CAMS:
        raise RuntimeError(f"lidar.depth_maps: {V} cameras; one call takes 1..{MAX_CAMS} (S3G_LIDAR_MAX_CAMS)")
    if H < 1 or W < 1 or V * H * W >= 1 << 31:
        raise RuntimeError(f"lidar.depth_maps: H = {H}, W = {W} (>= 1, V H W < 2^31)")
    c = _Cams(V, H, W, 0)
    for v in range(V):
        c.w2c[v][:] = _rigid(w2c[v], "w2c[v]").tolist()
        c.K[v][:] = np.ascontiguousarray(K[v]).reshape(9).tolist()
    if out is None:
        out = torch.empty((V, H, W), dtype=torch.float32, device=dev)
    elif not (torch.is_tensor(out) and out.is_cuda and out.device == dev and out.dtype == torch.float32
              and tuple(out.shape) == (V, H, W) and out.is_contiguous()):
        raise RuntimeError(f"lidar.depth_maps: out must be a contiguous fp32 [{V},{H},{W}] tensor on {dev}")
    if workspace is None:
        workspace = torch.empty(V * H * W, dtype=torch.int32, device=dev)
    elif not (torch.is_tensor(workspace) and workspace.is_cuda and workspace.device == dev and workspace.dtype == torch.int32
              and workspace.numel() >= V * H * W and workspace.is_contiguous()):
        raise RuntimeError(f"lidar.depth_maps: workspace must be a contiguous int32 tensor of at least {V * H * W} words on {dev}")
    L = _bind()
    with _lib.on_device(dev):
        _lib.check(L.s3g_lidar_depth_maps(C.byref(s), C.byref(c), out.data_ptr(), workspace.data_ptr(), _lib.stream_ptr()))
    calls += 1
    return out


class LidarCloud:
    """The initial point cloud: the union of the sweeps' world points inside the camera-frustum aabb, then one point per voxel.

    capacity: the sum of the sweeps' row counts (known from the file sizes); the float64 buffer [capacity,3] lives on `device`."""

    def __init__(self, aabb, capacity: int, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"lidar.LidarCloud: the cloud must live on the GPU (got {device}); no CPU fallback")
        aabb = np.ascontiguousarray(np.asarray(aabb.detach().cpu().numpy() if torch.is_tensor(aabb) else aabb, dtype=np.float64))
        if aabb.shape != (2, 3) or not np.isfinite(aabb).all():
            raise ValueError(f"lidar.LidarCloud: aabb must be a finite [2,3] array (min, max), got shape {aabb.shape}")
        capacity = int(capacity)
        if not 0 <= capacity < 1 << 31:
            raise ValueError(f"lidar.LidarCloud: capacity = {capacity} (0 <= capacity < 2^31)")
        self.aabb, self.capacity, self.device = aabb, capacity, device
        self.rows_offered = 0        # host-side: the rows of every sweep added so far, kept or not
        self.points = torch.empty((capacity, 3), dtype=torch.float64, device=device)
        self.total = torch.zeros(1, dtype=torch.int32, device=device)      # kept rows so far; stays on the device

    @torch.no_grad()
    def add(self, rows: torch.Tensor, l2w, x_range=(-2.0, 80.0), point_offset: int = 3) -> None:
        """Appends the sweep's world points with x_range[0] < p.x < x_range[1] and aabb_min <= world <= aabb_max, in source order.
        Three launches, no host read; a sweep whose rows do not fit the capacity is refused here, on the host."""
        global calls
        s = _sweep("LidarCloud.add", rows, l2w, x_range, point_offset)
        if rows.device != self.device:
            raise RuntimeError(f"lidar.LidarCloud.add: rows are on {rows.device}, the cloud on {self.device}")
        if self.rows_offered + s.N > self.capacity:
            raise RuntimeError(f"lidar.LidarCloud.add: a sweep of {s.N} rows after {self.rows_offered} does not fit the capacity "
                               f"{self.capacity} (the sum of the sweeps' row counts)")
        self.rows_offered += s.N
        if s.N == 0:
            return
        L = _bind()
        offsets = torch.empty(int(L.s3g_lidar_count_words(s.N)), dtype=torch.int32, device=self.device)
        box = (C.c_double * 6)(*self.aabb.reshape(6).tolist())
        with _lib.on_device(self.device):
            _lib.check(L.s3g_lidar_cloud_add(C.byref(s), box, self.points.data_ptr(), self.capacity, self.total.data_ptr(),
                                             offsets.data_ptr(), _lib.stream_ptr()))
        calls += 1

    def kept(self) -> torch.Tensor:
        """The accumulated float64 world points [n,3] (a view); reads the kept count back (4 bytes)."""
        n = int(self.total.item())
        if not 0 <= n <= self.rows_offered:
            raise RuntimeError(f"lidar.LidarCloud: the device counts {n} kept rows of {self.rows_offered} offered")
        return self.points[:n]

    @torch.no_grad()
    def finish(self, voxel_size: float = 0.013, num_pts: Optional[int] = None, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """GridSample3D: -> xyz [M,3] fp32, one point per distinct label, ascending label order; the representative of a label is its
        row with the lowest position in the cloud.  label = q.x b.y b.z + q.y b.z + q.z with q = rint(p / voxel_size) - min and
        b = max(q): b is the maximum, not the extent + 1, so two voxels can share a label (the reference's behaviour, kept).
        num_pts: when M exceeds it, a torch.randperm(M, generator=generator)[:num_pts] subset of the rows.
        Three host reads: the kept count, the grid range (the 2^53 guard) and M."""
        return grid_sample(self.kept(), voxel_size, num_pts, generator)


@torch.no_grad()
def grid_sample(points: torch.Tensor, voxel_size: float = 0.013, num_pts: Optional[int] = None,
                generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """LidarCloud.finish on any contiguous float64 [n,3] device tensor (two host reads: the grid range and M)."""
    global calls
    if not (torch.is_tensor(points) and points.is_cuda):
        where = points.device if torch.is_tensor(points) else type(points).__name__
        raise RuntimeError(f"lidar.grid_sample: points must live on the GPU (got {where}); no CPU fallback")
    if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float64 or not points.is_contiguous():
        raise RuntimeError("lidar.grid_sample: points must be a contiguous float64 [n,3] tensor")
    voxel_size = float(voxel_size)
    if not voxel_size > 0.0:
        raise ValueError(f"lidar.grid_sample: voxel_size = {voxel_size} (> 0)")
    dev, n = points.device, int(points.shape[0])
    if n >= 1 << 31:
        raise RuntimeError(f"lidar.grid_sample: {n} points (< 2^31)")
    if n == 0:
        return torch.empty((0, 3), dtype=torch.float32, device=dev)
    L = _bind()
    stats = torch.empty(6, dtype=torch.int64, device=dev)
    work = torch.empty(int(L.s3g_lidar_grid_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    offsets = torch.empty(int(L.s3g_lidar_count_words(n)), dtype=torch.int32, device=dev)
    with _lib.on_device(dev):
        stream = _lib.stream_ptr()
        _lib.check(L.s3g_lidar_grid_range(n, points.data_ptr(), voxel_size, stats.data_ptr(), work.data_ptr(), stream))
        check_label_range(stats.tolist())                                   # host read: 48 bytes
        _lib.check(L.s3g_lidar_grid_keys(n, points.data_ptr(), voxel_size, stats.data_ptr(), keys.data_ptr(), stream))
        sorted_keys, perm = torch.sort(keys, stable=True)                   # plumbing: a stable sort keeps the lowest row in front
        _lib.check(L.s3g_lidar_grid_heads(n, sorted_keys.data_ptr(), offsets.data_ptr(), stream))
        M = int(offsets[-1].item())                                         # host read: 4 bytes, sizes the output
        if not 1 <= M <= n:
            raise RuntimeError(f"lidar.grid_sample: the scan counts {M} labels among {n} points")
        out = torch.empty((M, 3), dtype=torch.float32, device=dev)
        _lib.check(L.s3g_lidar_grid_gather(n, sorted_keys.data_ptr(), perm.data_ptr(), points.data_ptr(), offsets.data_ptr(),
                                           out.data_ptr(), M, stream))
    calls += 1
    if num_pts is not None and M > int(num_pts):
        gdev = generator.device if generator is not None else dev
        out = out[torch.randperm(M, generator=generator, device=gdev)[:int(num_pts)].to(dev)]
    return out


def check_label_range(stats: Sequence[int]) -> int:
    """stats = qmin x y z, b x y z (struct s3g_lidar_grid_stats).  -> b.x b.y b.z; a cloud whose product reaches 2^53 is refused: the
    reference's float64 labels would no longer be exact integers there, and no int64 key could stand for them."""
    b = [int(v) for v in stats[3:6]]
    if any(q > LABEL_LIMIT or q < -LABEL_LIMIT for q in [int(v) for v in stats[:3]]) or any(v < 0 or v > LABEL_LIMIT for v in b):
        raise RuntimeError(f"lidar.grid_sample: the quantized cloud spans {stats}: coordinates / voxel_size reach 2^53, beyond the exact integers of float64")
    product = b[0] * b[1] * b[2]
    if product >= LABEL_LIMIT:
        raise RuntimeError(f"lidar.grid_sample: the grid spans b = {b} voxels, b.x b.y b.z = {product} >= 2^53: the voxel labels are "
                           "no longer exact in float64; use a larger voxel_size or a smaller aabb")
    return product


# ---- host helpers ---------------------------------------------------------------------------------------------------------------------
def read_sweep(path: str) -> torch.Tensor:
    """The raw sweep file as a [N,10] fp32 host tensor (scene/dataset_readers.py:830-834): origin 0:3, point 3:6, ..., laser id 9."""
    a = np.fromfile(path, dtype=np.float32)
    if a.size % 10 != 0:
        raise ValueError(f"lidar.read_sweep: {path} holds {a.size} floats, not a multiple of 10")
    return torch.from_numpy(a.reshape(-1, 10))


def frustum_aabb(c2w, K, H: int, W: int, depth_range=(0.01, 80.0)) -> np.ndarray:
    """The aabb of every camera's frustum between the two depths (scene/dataset_readers.py:752-779), numpy float64 on the host.
    c2w [n,4,4], K [n,3,3] -> [2,3] (min, max)."""
    c2w = np.asarray(c2w, dtype=np.float64)
    K = np.asarray(K, dtype=np.float64)
    corners = np.array([[0, 0], [0, H], [W, H], [W, 0]])
    homog = np.concatenate([corners, np.ones((4, 1))], axis=-1).T
    lo, hi = [], []
    for pose, intri in zip(c2w, K):
        for extent in depth_range:
            cam = np.linalg.inv(intri) @ homog * extent
            world = pose[:3, :3] @ cam + pose[:3, 3:4]
            lo.append(world.min(axis=1))
            hi.append(world.max(axis=1))
    return np.stack([np.min(lo, axis=0), np.max(hi, axis=0)], axis=0)


def sh2rgb(sh):
    """utils/sh_utils.py SH2RGB: sh * C0 + 0.5."""
    return sh * SH_C0 + 0.5


def init_colors(n: int, generator: Optional[torch.Generator] = None, device="cpu") -> torch.Tensor:
    """SH2RGB(rand(n,3) / 255) (scene/dataset_readers.py:907, 967) as float64 [n,3]: the colours create_from_points turns back into
    the DC coefficient.  The uniform numbers come from torch's generator (the reference: np.random; another stream)."""
    gdev = generator.device if generator is not None else torch.device(device)
    u = torch.rand((int(n), 3), generator=generator, dtype=torch.float64, device=gdev)
    return sh2rgb(u / 255.0).to(device)
