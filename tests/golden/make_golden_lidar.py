"""Generate tests/golden/lidar.npz by RUNNING THE REFERENCE'S OWN `readWaymoInfo` (scene/dataset_readers.py:597-1093) and `GridSample3D`
(:1102-1144) in the build container.  /root/reference is only ever imported here, never copied; without it this script refuses to run.

    python tests/golden/make_golden_lidar.py        # rewrites lidar.npz next to this file

How the reference's reader runs without a dataset, a GPU, `cv2` or `plyfile`:
  1. `scene.dataset_readers` is imported with the stub finder of oracle/ref_py.py standing in for the packages the image lacks;
  2. a throw-away Waymo-layout directory is written into a temporary directory: 2 timestamps (10 empty files under images/, so that
     the reader's listing gives num_seqs = 2), intrinsics/0..2.txt, extrinsics/0..4.txt (real rotations), ego_pose/000.txt (identity)
     and 001.txt (a real rigid motion), lidar/000.bin and 001.bin ([N,10] fp32, zeros outside columns 3:6);
  3. four names inside `scene.dataset_readers` are stand-ins while it runs:
       constructCameras_waymo -> a recorder that keeps each frame's transform_matrix, intrinsic and depth_map and ends the call by
                                 raising a private exception once it has seen the full list (images are never opened)
       storePly               -> a recorder of the down-sampled cloud
       get_OccGrid            -> a recorder of the accumulated cloud and of the camera-frustum aabb (save_occ_grid=True hands both over)
       get_split_point        -> the reference's own function, wrapped: the labels it is handed are kept
  4. GridSample3D is then called directly on a second cloud.

Stored: the two sweeps' points [N,3] fp32, l2w [2,4,4], per frame c2w, K and the map as (flat index, float64 value) of its non-zeros,
the aabb, the sorted distinct labels and the count of the reader's own cloud, the second cloud with its labels, and for the host
helpers a block of uniform numbers with the reference's SH2RGB of them.

The generator ASSERTS, and reseeds until all hold (sizes and margins below):
  (a) over the six maps >= 300 pixels receive >= 2 points, and in >= 100 of them the last point is neither the first nor the nearest;
  (b) no counted u or v within 1e-9 of an integer;  (c) no pix.z within 1e-9 of 0, no x within 1e-6 of a range bound;
  (d) no winning z within a relative 1e-12 of an fp32 rounding boundary;
  (e) no p / voxel_size within 1e-9 of a half-integer, no world coordinate within 1e-9 of the aabb;
  (f) >= 20 % of the cloud's labels hold >= 2 points.
Under (b)-(e) the summation order and FMA use of numpy's matmul cannot change a decision of the ordered restatement.
"""
import importlib
import os
import sys
import tempfile
import types

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "lidar.npz")

H, W = 640, 960                  # the reference's hard-coded load_size
ORIGINAL = (1280, 1920)          # its ORIGINAL_SIZE of cameras 0..2
BASE_POINTS = 2000               # per sweep; every base point comes with COPIES jittered copies: N = 8000
COPIES = 3
JITTER = 0.002                   # metres
VOXEL = 0.013
SECOND_CLOUD = 6000
N_COLORS = 64
FIRST_SEED = 20241021


class _Done(Exception):
    pass


def reference_present() -> bool:
    return os.path.isfile(os.path.join(REF, "scene", "dataset_readers.py"))


def _import_reference():
    """-> (scene.dataset_readers module, cleanup()).  Nothing of what is imported here stays in sys.modules afterwards."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import ref_py
    before = set(sys.modules)
    finder = ref_py._StubFinder([n for n in ref_py.STUBBED if ref_py._missing(n)])
    sys.meta_path.append(finder)
    for pkg in ("scene", "utils"):       # package objects that do not execute the reference's __init__.py
        m = types.ModuleType(pkg)
        m.__path__ = [os.path.join(REF, pkg)]
        sys.modules[pkg] = m
    sys.path.insert(0, REF)

    def cleanup():
        for name in set(sys.modules) - before:
            del sys.modules[name]
        if finder in sys.meta_path:
            sys.meta_path.remove(finder)
        if REF in sys.path:
            sys.path.remove(REF)

    try:
        dr = importlib.import_module("scene.dataset_readers")
    except Exception:
        cleanup()
        raise
    return dr, cleanup


def _rot(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    Ry = np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
    Rx = np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]])
    return Rz @ Ry @ Rx


def _pose(yaw, pitch, roll, t):
    m = np.eye(4)
    m[:3, :3] = _rot(yaw, pitch, roll)
    m[:3, 3] = t
    return m


def make_inputs(seed):
    rng = np.random.default_rng(seed)
    yaws = np.deg2rad([0.7, 44.3, -45.1, 89.0, -91.0])
    extr = [_pose(yaws[i], np.deg2rad(rng.uniform(-2, 2)), np.deg2rad(rng.uniform(-1, 1)),
                  [1.5 + 0.1 * i, 0.2 * (i % 3) - 0.2, 2.1 + 0.01 * i]) for i in range(5)]
    intr = [np.array([2050.0 + 7.3 * i, 2047.0 - 5.1 * i, 960.0 + 3.7 * i, 640.0 - 2.9 * i, 0.01, -0.02, 0.0, 0.0, 0.0]) for i in range(3)]
    ego = [np.eye(4), _pose(np.deg2rad(2.3), np.deg2rad(0.4), np.deg2rad(-0.3), [1.37, 0.061, 0.013])]
    sweeps = []
    for t in range(2):
        az = rng.uniform(-np.deg2rad(80), np.deg2rad(80), BASE_POINTS)
        rg = rng.uniform(2.5, 92.0, BASE_POINTS) ** 1.0
        z = rng.uniform(-2.0, 7.0, BASE_POINTS)
        base = np.stack([rg * np.cos(az) - 4.0, rg * np.sin(az), z], axis=1)       # some x below -2, some above 80
        pts = np.concatenate([base] + [base + rng.normal(0.0, JITTER, base.shape) for _ in range(COPIES)], axis=0)
        pts = pts[rng.permutation(len(pts))].astype(np.float32)
        rows = np.zeros((len(pts), 10), dtype=np.float32)
        rows[:, 3:6] = pts
        sweeps.append(rows)
    second = rng.uniform(-3.0, 3.0, (SECOND_CLOUD // 3, 3)) * np.array([4.0, 2.0, 0.5])
    second = np.concatenate([second, second + rng.normal(0, 0.004, second.shape), second + rng.normal(0, 0.004, second.shape)], axis=0)
    second = second[rng.permutation(len(second))]
    uniform = rng.random((N_COLORS, 3))
    return dict(extr=extr, intr=intr, ego=ego, sweeps=sweeps, second=second, uniform=uniform)


def write_dataset(root, inp):
    for d in ("images", "intrinsics", "extrinsics", "ego_pose", "lidar"):
        os.makedirs(os.path.join(root, d))
    for t in range(2):
        for cam in range(5):
            open(os.path.join(root, "images", f"{t:03d}_{cam}.jpg"), "w").close()
        np.savetxt(os.path.join(root, "ego_pose", f"{t:03d}.txt"), inp["ego"][t], fmt="%.17g")
        inp["sweeps"][t].tofile(os.path.join(root, "lidar", f"{t:03d}.bin"))
    for i, a in enumerate(inp["intr"]):
        np.savetxt(os.path.join(root, "intrinsics", f"{i}.txt"), a, fmt="%.17g")
    for i, a in enumerate(inp["extr"]):
        np.savetxt(os.path.join(root, "extrinsics", f"{i}.txt"), a, fmt="%.17g")


def run_reference(dr, inp):
    """-> dict with what the reference's readWaymoInfo and GridSample3D computed."""
    rec = {"frames": None, "ply": None, "occ": None, "labels": []}
    real_split = dr.get_split_point

    def cameras(frames_list, *a, **k):
        rec["frames"] = [dict(c2w=np.array(f["transform_matrix"], dtype=np.float64), K=np.array(f["intrinsic"], dtype=np.float64),
                              depth_map=np.array(f["depth_map"], dtype=np.float64)) for f in frames_list]
        if len(rec["frames"]) == 6:
            raise _Done()
        return []

    def store_ply(path, xyz, rgb):
        rec["ply"] = np.array(xyz, dtype=np.float64)

    def occ_grid(points, aabb, voxel):
        rec["occ"] = (np.array(points, dtype=np.float64), np.array(aabb, dtype=np.float64))
        return np.zeros((1, 1, 1), dtype=bool)

    def split_point(labels):
        rec["labels"].append(np.array(labels, dtype=np.float64))
        return real_split(labels)

    dr.constructCameras_waymo, dr.storePly, dr.get_OccGrid, dr.get_split_point = cameras, store_ply, occ_grid, split_point
    with tempfile.TemporaryDirectory() as tmp:
        write_dataset(tmp, inp)
        try:
            dr.readWaymoInfo(tmp, False, False, num_pts=10 ** 9, save_occ_grid=True)
            raise AssertionError("the camera recorder never saw the full list")
        except _Done:
            pass
    assert rec["ply"] is not None and rec["occ"] is not None and len(rec["labels"]) == 1 and len(rec["frames"]) == 6
    second_out, _ = dr.GridSample3D(inp["second"].copy(), np.zeros((len(inp["second"]), 3)))
    assert len(rec["labels"]) == 2
    colors = dr.SH2RGB(inp["uniform"] / 255.0)
    return dict(frames=rec["frames"], cloud_out=rec["ply"], cloud_in=rec["occ"][0], aabb=rec["occ"][1], labels=rec["labels"][0],
                second_out=np.array(second_out, dtype=np.float64), second_labels=rec["labels"][1], colors=np.array(colors, dtype=np.float64))


def _far_from_integer(x, gap):
    return bool((np.abs(x - np.round(x)) > gap).all())


def _far_from_f32_boundary(z, rel):
    f = z.astype(np.float32)
    lo, hi = np.nextafter(f, np.float32(-np.inf)).astype(np.float64), np.nextafter(f, np.float32(np.inf)).astype(np.float64)
    f = f.astype(np.float64)
    d = np.minimum(np.abs(z - (f + lo) / 2), np.abs(z - (f + hi) / 2))
    return bool((d > rel * np.abs(z)).all())


def conditions(inp, ref):
    """-> (ok, report).  Uses the ordered restatement for the per-point quantities, the reference's results for the rest."""
    from tests import lidar_ref as lr
    l2w = [np.linalg.inv(inp["ego"][0]) @ e for e in inp["ego"]]
    contended = neither = 0
    ok = True
    for t in range(2):
        rows = inp["sweeps"][t]
        x = rows[:, 3].astype(np.float64)
        ok &= bool((np.abs(x + 2.0) > 1e-6).all() and (np.abs(x - 80.0) > 1e-6).all())                              # (c)
        fr = ref["frames"][3 * t:3 * t + 3]
        w2c = np.stack([np.linalg.inv(f["c2w"]) for f in fr])
        K = np.stack([f["K"] for f in fr])
        mask, world = lr.world_points(rows, l2w[t])
        ok &= bool((np.abs(world[mask] - ref["aabb"][0]) > 1e-9).all() and (np.abs(world[mask] - ref["aabb"][1]) > 1e-9).all())   # (e)
        winner, zs, counted, pixel = lr.winners(rows, l2w[t], w2c, K, H, W)
        for v in range(3):
            u, vv, z = lr.project(world, w2c[v], K[v])
            ok &= bool((np.abs(z[mask]) > 1e-9).all())                                                               # (c)
            c = counted[v]
            ok &= _far_from_integer(u[c], 1e-9) and _far_from_integer(vv[c], 1e-9)                                   # (b)
            # points that fall just outside the image must not sit on its border either
            near = mask & (z > 0)
            ok &= _far_from_integer(u[near & (np.abs(u) < 4 * W)], 1e-9) and _far_from_integer(vv[near & (np.abs(vv) < 4 * H)], 1e-9)
            hit = winner[v] >= 0
            ok &= _far_from_f32_boundary(zs[v][winner[v][hit]], 1e-12)                                               # (d)
            idx = np.where(c)[0]
            order = np.argsort(pixel[v, idx], kind="stable")
            pix_sorted, idx_sorted = pixel[v, idx][order], idx[order]
            starts = np.flatnonzero(np.r_[True, pix_sorted[1:] != pix_sorted[:-1]])
            ends = np.r_[starts[1:], len(pix_sorted)]
            for s, e in zip(starts, ends):
                if e - s >= 2:
                    contended += 1
                    members = idx_sorted[s:e]                      # ascending rows
                    last = members[-1]
                    if last != members[0] and zs[v][last] != zs[v][members].min():
                        neither += 1
    ok &= contended >= 300 and neither >= 100                                                                        # (a)
    shares = []
    for cloud, labels in ((ref["cloud_in"], ref["labels"]), (inp["second"], ref["second_labels"])):
        frac = cloud / VOXEL
        ok &= bool((np.abs(np.abs(frac - np.floor(frac)) - 0.5) > 1e-9).all())                                      # (e)
        _, counts = np.unique(labels, return_counts=True)
        shares.append(float((counts >= 2).mean()))
        ok &= shares[-1] >= 0.20                                                                                     # (f)
    return bool(ok), dict(contended=contended, neither=neither, shares=shares)


def generate():
    """-> dict of numpy arrays (what lidar.npz holds)."""
    if not reference_present():
        raise SystemExit(f"{REF} is not here: this generator runs the reference's own code and cannot run without it")
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    dr, cleanup = _import_reference()
    try:
        seed = FIRST_SEED
        while True:
            inp = make_inputs(seed)
            ref = run_reference(dr, inp)
            ok, report = conditions(inp, ref)
            if ok:
                break
            print(f"seed {seed}: conditions not met ({report}); reseeding")
            seed += 1
    finally:
        cleanup()
    out = dict(seed=np.int64(seed), H=np.int64(H), W=np.int64(W), voxel=np.float64(VOXEL),
               points0=inp["sweeps"][0][:, 3:6].copy(), points1=inp["sweeps"][1][:, 3:6].copy(),
               l2w=np.stack([np.linalg.inv(inp["ego"][0]) @ e for e in inp["ego"]]),
               c2w=np.stack([f["c2w"] for f in ref["frames"]]), K=np.stack([f["K"] for f in ref["frames"]]),
               aabb=ref["aabb"], cloud_count_in=np.int64(len(ref["cloud_in"])), cloud_count=np.int64(len(ref["cloud_out"])),
               cloud_labels=np.unique(ref["labels"]).astype(np.int64),
               second=inp["second"], second_labels=ref["second_labels"].astype(np.int64), second_count=np.int64(len(ref["second_out"])),
               uniform=inp["uniform"], colors=ref["colors"],
               contended=np.int64(report["contended"]), neither=np.int64(report["neither"]), shares=np.array(report["shares"]))
    assert np.array_equal(ref["labels"], ref["labels"].astype(np.int64)) and np.array_equal(ref["second_labels"], out["second_labels"])
    for i, f in enumerate(ref["frames"]):
        assert f["depth_map"].shape == (H, W)
        flat = np.flatnonzero(f["depth_map"].reshape(-1))
        out[f"map{i}_index"] = flat.astype(np.int32)
        out[f"map{i}_value"] = f["depth_map"].reshape(-1)[flat]
    return out


if __name__ == "__main__":
    arrays = generate()
    np.savez_compressed(OUT, **arrays)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes; seed {int(arrays['seed'])}, {len(arrays['points0'])} + {len(arrays['points1'])} points, "
          f"{sum(len(arrays[f'map{i}_index']) for i in range(6))} map entries, {int(arrays['contended'])} contended pixels "
          f"({int(arrays['neither'])} where the last point is neither the first nor the nearest), cloud {int(arrays['cloud_count_in'])} -> "
          f"{int(arrays['cloud_count'])} labels, second cloud {len(arrays['second'])} -> {int(arrays['second_count'])}, "
          f"label shares with >= 2 points {arrays['shares']}")
