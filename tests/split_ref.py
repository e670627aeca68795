"""numpy restatement of the dynamic / static point-cloud split (scene/gaussian_model.py:258-348 of the reference), the yardstick of
tests/test_split_cpu.py (against the tables the reference's own save_ply_split recorded) and tests/test_split_gpu.py (for the
kernels of include/s3g_split.h):

    motion_mask(dx)      m_i = max|dx_i| in fp32, thre = fp32(float64 mean of m), mask = m > thre
    table(...)           [x y z | 0 0 0 | f_dc | f_rest channel-major | opacity | scale | rot] rows, x y z = xyz (+ dx, one fp32 add)
    split_tables(...)    the rows of np.where(mask)[0] and of np.where(~mask)[0], each in source order
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "split_pcd.npz")
TIE_GAP = 1e-5          # no m_i within this relative distance of the threshold: a last-bit difference in thre then moves no point
INPUTS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")


def load_fixture():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def max_abs(dx):
    return np.abs(np.asarray(dx, dtype=np.float32)).max(axis=1) if len(dx) else np.zeros(0, np.float32)


def threshold(m):
    """fp32(float64 mean): the sum in float64, one rounding to fp32."""
    return np.float32(np.asarray(m, dtype=np.float64).sum() / max(len(m), 1)) if len(m) else np.float32("nan")


def motion_mask(dx):
    """-> (mask bool [P], thre fp32, m fp32 [P])."""
    m = max_abs(dx)
    thre = threshold(m)
    return m > thre, thre, m


def no_near_tie(m, thre, gap=TIE_GAP) -> bool:
    """No m_i lies within a relative `gap` of thre."""
    m = np.asarray(m, dtype=np.float64)
    return bool(np.all(np.abs(m - float(thre)) > gap * abs(float(thre)))) if len(m) else True


def tie_free(m, thre) -> bool:
    """no_near_tie, or P == 1: the one value then IS the mean in every arithmetic (a float64 sum of one fp32 number, divided by 1, is
    that number; so is torch's fp32 mean), and the strict comparison is False on every side."""
    return (len(m) == 1 and np.float32(thre) == np.float32(m[0])) or no_near_tie(m, thre)


def table(xyz, f_dc, f_rest, opacity, scaling, rotation, dx=None):
    """-> float32 [P, 17 + 3 R]."""
    f32 = lambda a: np.asarray(a, dtype=np.float32)
    xyz = f32(xyz)
    P = xyz.shape[0]
    pos = xyz if dx is None else xyz + f32(dx)
    cols = [pos, np.zeros_like(pos), f32(f_dc).transpose(0, 2, 1).reshape(P, -1), f32(f_rest).transpose(0, 2, 1).reshape(P, -1),
            f32(opacity).reshape(P, 1), f32(scaling).reshape(P, 3), f32(rotation).reshape(P, 4)]
    return np.ascontiguousarray(np.concatenate(cols, axis=1), dtype=np.float32)


def split_tables(mask, full):
    """-> (dynamic rows, static rows) of the full table, stable."""
    mask = np.asarray(mask, dtype=bool)
    return full[np.where(mask)[0]], full[np.where(~mask)[0]]


def block_offsets(mask, block=256):
    """int32 [ceil(P / block) + 1]: dynamic Gaussians in front of each block, then the total."""
    mask = np.asarray(mask, dtype=bool)
    nb = max((len(mask) + block - 1) // block, 1)
    counts = np.array([int(mask[b * block:(b + 1) * block].sum()) for b in range(nb)], dtype=np.int64)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def structured(rows, names):
    """The rows as the structured array the reference hands to PlyElement.describe."""
    out = np.empty(rows.shape[0], dtype=[(n, "f4") for n in names])
    for k, n in enumerate(names):
        out[n] = rows[:, k]
    return out


def attribute_names(sh_rest):
    return (["x", "y", "z", "nx", "ny", "nz"] + [f"f_dc_{i}" for i in range(3)] + [f"f_rest_{i}" for i in range(3 * sh_rest)]
            + ["opacity"] + [f"scale_{i}" for i in range(3)] + [f"rot_{i}" for i in range(4)])


def random_model(P, R, seed, sigma=1.5):
    """Seeded inputs of P Gaussians with R rows of f_rest and a heavy-tailed (log-normal) dx without a near tie at its threshold.
    -> dict of float32 arrays (INPUTS + "dx")."""
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    out = dict(xyz=f(P, 3) * 10, f_dc=f(P, 1, 3), f_rest=f(P, R, 3), opacity=f(P, 1), scaling=f(P, 3) - 3, rotation=f(P, 4))
    for _ in range(64):
        mag = np.exp(sigma * rng.standard_normal((P, 1))).astype(np.float32) * 0.01
        dx = (mag * rng.uniform(-1, 1, (P, 3))).astype(np.float32)
        mask, thre, m = motion_mask(dx)
        if tie_free(m, thre):
            out["dx"] = dx
            return out
    raise AssertionError("no tie-free dx found")
