"""numpy float64 restatement of the LiDAR scene set-up (readWaymoInfo, scene/dataset_readers.py:838-911, and GridSample3D, :1102-1144,
of the reference) IN THE KERNELS' ARITHMETIC ORDER (include/s3g_lidar.h): the yardstick of tests/test_lidar_cpu.py (against what the
reference's own readWaymoInfo and GridSample3D recorded, tests/golden/lidar.npz) and of tests/test_lidar_gpu.py.

    world_points(rows, l2w)        the x-range mask and world = ((R0 p0 + R1 p1) + R2 p2) + t per row, float64, no contraction
    depth_maps(rows, l2w, ...)     per camera: the pixel takes pix.z of the counted point with the HIGHEST source row (np.maximum.at
                                   on the row index = numpy's last assignment), returned as float64 [V,H,W]; fp32 is one .astype
    cloud_rows(rows, l2w, aabb)    the kept world rows in source order
    grid_labels / grid_sample      q = np.around(p / voxel), q -= min, b = max(q), label = q.x b.y b.z + q.y b.z + q.z in int64; the
                                   representative of a label is its LOWEST row (stable argsort), output in ascending label order
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lidar.npz")
X_RANGE = (-2.0, 80.0)
VOXEL = 0.013
LABEL_LIMIT = 1 << 53


def load_fixture():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _row34(M, r, v):
    """Row r of a [3,4] (or [4,4]) transform applied to the columns v[:, 0..2]: ordered sum, translation last."""
    return ((M[r, 0] * v[:, 0] + M[r, 1] * v[:, 1]) + M[r, 2] * v[:, 2]) + M[r, 3]


def world_points(rows, l2w, x_range=X_RANGE, point_offset=3):
    """-> (mask [N] of x_min < p.x < x_max on the fp32 value, world [N,3] float64 of EVERY row)."""
    rows = np.asarray(rows, dtype=np.float32)
    p = rows[:, point_offset:point_offset + 3].astype(np.float64)
    mask = (p[:, 0] > float(x_range[0])) & (p[:, 0] < float(x_range[1]))
    l2w = np.asarray(l2w, dtype=np.float64)
    world = np.stack([_row34(l2w, r, p) for r in range(3)], axis=1) if len(p) else np.zeros((0, 3))
    return mask, world


def project(world, w2c, K):
    """-> (u, v, z) float64 per row (u, v meaningless where z <= 0)."""
    cam = np.stack([_row34(w2c, r, world) for r in range(3)], axis=1)
    pix = np.stack([(K[r, 0] * cam[:, 0] + K[r, 1] * cam[:, 1]) + K[r, 2] * cam[:, 2] for r in range(3)], axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return pix[:, 0] / pix[:, 2], pix[:, 1] / pix[:, 2], pix[:, 2]


def winners(rows, l2w, w2c, K, H, W, x_range=X_RANGE, point_offset=3):
    """-> (winner [V,H,W] int64: the highest counted row per pixel or -1, z [V,N] float64, counted [V,N] bool, pixel [V,N] int64)."""
    mask, world = world_points(rows, l2w, x_range, point_offset)
    w2c, K = np.asarray(w2c, dtype=np.float64), np.asarray(K, dtype=np.float64)
    V, N = len(w2c), len(world)
    winner = np.full((V, H * W), -1, dtype=np.int64)
    zs, counted, pixel = np.zeros((V, N)), np.zeros((V, N), dtype=bool), np.zeros((V, N), dtype=np.int64)
    for v in range(V):
        if N == 0:
            continue
        u, vv, z = project(world, w2c[v], K[v])
        with np.errstate(invalid="ignore"):
            ok = mask & (z > 0) & (u >= 0) & (u < W) & (vv >= 0) & (vv < H)
        idx = np.where(ok)[0]
        pix = vv[idx].astype(np.int64) * W + u[idx].astype(np.int64)
        np.maximum.at(winner[v], pix, idx)
        zs[v], counted[v] = z, ok
        pixel[v, idx] = pix
    return winner.reshape(V, H, W), zs, counted, pixel


def depth_maps(rows, l2w, w2c, K, H, W, x_range=X_RANGE, point_offset=3):
    """-> [V,H,W] float64; .astype(np.float32) is what the kernels write."""
    winner, zs, _, _ = winners(rows, l2w, w2c, K, H, W, x_range, point_offset)
    out = np.zeros(winner.shape)
    for v in range(winner.shape[0]):
        hit = winner[v] >= 0
        out[v][hit] = zs[v][winner[v][hit]]
    return out


def cloud_rows(rows, l2w, aabb, x_range=X_RANGE, point_offset=3):
    """The world rows inside the x range and the (inclusive) aabb, in source order: float64 [n,3]."""
    mask, world = world_points(rows, l2w, x_range, point_offset)
    aabb = np.asarray(aabb, dtype=np.float64)
    keep = mask & np.all((world >= aabb[0]) & (world <= aabb[1]), axis=-1)
    return world[keep]


def grid_labels(points, voxel=VOXEL):
    """-> (labels [n] int64, b [3] int64).  The reference's float64 label as exact integers; refuses b.x b.y b.z >= 2^53."""
    q = np.around(np.asarray(points, dtype=np.float64) / voxel)
    q = (q - q.min(axis=0)).astype(np.int64)
    b = q.max(axis=0)
    if int(b[0]) * int(b[1]) * int(b[2]) >= LABEL_LIMIT:
        raise ValueError("grid_labels: b.x b.y b.z >= 2^53")
    return q[:, 0] * b[1] * b[2] + q[:, 1] * b[2] + q[:, 2], b


def grid_sample(points, voxel=VOXEL):
    """-> (xyz [M,3] fp32 in ascending label order, rows [M]: the lowest row of every label, labels [M] ascending)."""
    points = np.asarray(points, dtype=np.float64)
    if len(points) == 0:
        return np.zeros((0, 3), np.float32), np.zeros(0, np.int64), np.zeros(0, np.int64)
    labels, _ = grid_labels(points, voxel)
    order = np.argsort(labels, kind="stable")
    s = labels[order]
    head = np.ones(len(s), dtype=bool)
    head[1:] = s[1:] != s[:-1]
    rows = order[head]
    return points[rows].astype(np.float32), rows, s[head]


def sparse_map(flat_index, values, H, W):
    """A recorded map (flat index, float64 value of its non-zeros) back as float64 [H,W]."""
    m = np.zeros(H * W)
    m[flat_index] = values
    return m.reshape(H, W)
