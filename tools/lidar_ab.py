#!/usr/bin/env python
"""LiDAR scene set-up: the kernel route against the numpy route a user had before it existed, at the reference's own workload.

  workload  50 sweeps of 170 000 rows ([N,10] fp32, the raw file layout), 3 cameras per timestamp, at 640 x 960 (the only size the
            reference's loader can produce) and at 1066 x 1600 (the size this project benchmarks).
  numpy     readWaymoInfo's arithmetic restated in its own BLAS form on the host, float64: per sweep the x-range mask, the world
            transform, per camera w2c / K matmuls, the image mask and `depth_map[iy, ix] = z`; every float64 map is uploaded and cast to
            fp32 as it is made (train.py uploads and casts them one by one); then the aabb filter over the concatenated cloud,
            GridSample3D (np.around, labels, np.argsort, run heads) and the upload of the fp32 cloud.
  kernels   starts from the same raw tables on the host: per sweep one upload of the table as it is, lidar.depth_maps into a slice of
            the [150,H,W] output, LidarCloud.add; then LidarCloud.finish.
  Both routes end with the fp32 maps and the cloud on the device; host wall clock around the whole route, device idle before and after.

    python tools/lidar_ab.py [--reps 5] [--warmup 1] [--out profiles/lidar_ab.txt] [--sweeps 50] [--rows 170000] [--step-timeout 420]

The parent process never touches the GPU: every image size is measured by a child process of its own under its own time limit, the
two routes alternated inside it; a child that fails or runs out of time ends the run (nothing else is started).  The routes' results
are compared as well (maps: pixels that differ; cloud: label count).  There is no speed gate."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = ((640, 960), (1066, 1600))
X_RANGE = (-2.0, 80.0)
VOXEL = 0.013


def _rot(yaw, pitch):
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    return np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]]) @ np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])


def workload(T, N, H, W, seed=0):
    """-> (sweeps: T arrays [N,10] fp32, l2ws [T,4,4], c2ws [3T,4,4], Ks [3T,3,3]): a vehicle driving forward 1.1 m per sweep, a
    360-degree scan of 2..75 m around it, three cameras fanned out 45 degrees with the focal length of the Waymo front cameras."""
    rng = np.random.default_rng(seed)
    to_cv = np.array([[0, 0, 1, 0], [-1, 0, 0, 0], [0, -1, 0, 0], [0, 0, 0, 1.0]])
    c2e = []
    for yaw in (45.0, 0.0, -45.0):
        m = np.eye(4)
        m[:3, :3] = _rot(np.deg2rad(yaw + 0.3), np.deg2rad(0.4))
        m[:3, 3] = [1.5, 0.0, 2.1]
        c2e.append(m @ to_cv)
    K = np.array([[2050.0 * W / 1920.0, 0, W / 2 + 1.3], [0, 2050.0 * H / 1280.0, H / 2 - 0.7], [0, 0, 1.0]])
    sweeps, l2ws, c2ws, Ks = [], [], [], []
    for t in range(T):
        l2w = np.eye(4)
        l2w[:3, :3] = _rot(np.deg2rad(0.05 * t), 0.0)
        l2w[:3, 3] = [1.1 * t, 0.01 * t, 0.0]
        az, rg = rng.uniform(-np.pi, np.pi, N), rng.uniform(2.0, 75.0, N)
        rows = np.zeros((N, 10), dtype=np.float32)
        rows[:, 3], rows[:, 4], rows[:, 5] = rg * np.cos(az), rg * np.sin(az), rng.uniform(-2.0, 4.0, N)
        sweeps.append(rows)
        l2ws.append(l2w)
        for m in c2e:
            c2ws.append(l2w @ m)
            Ks.append(K)
    return sweeps, np.stack(l2ws), np.stack(c2ws), np.stack(Ks)


def numpy_route(sweeps, l2ws, c2ws, Ks, H, W, aabb, dev):
    """scene/dataset_readers.py:838-911, 927 in the reference's own (BLAS) form; the maps go up one by one as train.py:392 does."""
    import torch
    V = len(c2ws) // len(sweeps)
    maps, points = torch.empty((len(c2ws), H, W), dtype=torch.float32, device=dev), []
    for t, rows in enumerate(sweeps):
        p = rows[:, 3:6]
        valid = (p[:, 0] < X_RANGE[1]) & (p[:, 0] > X_RANGE[0])
        p = p[valid]
        world = (l2ws[t][:3, :3] @ p.T + l2ws[t][:3, 3:4]).T
        for v in range(V):
            w2c = np.linalg.inv(c2ws[t * V + v])
            cam = (w2c[:3, :3] @ world.T + w2c[:3, 3:4]).T
            pix = (Ks[t * V + v] @ cam.T).T
            pix = pix[pix[:, 2] > 0]
            img = pix[:, :2] / pix[:, 2:]
            ok = (img[:, 0] >= 0) & (img[:, 0] < W) & (img[:, 1] >= 0) & (img[:, 1] < H)
            pix, img = pix[ok], img[ok]
            depth = np.zeros((H, W))
            depth[img[:, 1].astype(np.int32), img[:, 0].astype(np.int32)] = pix[:, 2]
            maps[t * V + v].copy_(torch.from_numpy(depth).to(dev))           # the float64 map goes up, the cast happens there
        points.append(world)
    points = np.concatenate(points, axis=0)
    points = points[np.all((points >= aabb[0]) & (points <= aabb[1]), axis=-1)]
    q = np.around(points / VOXEL)
    q -= np.min(q, axis=0)
    b = np.max(q, axis=0)
    labels = q[:, 0] * b[1] * b[2] + q[:, 1] * b[2] + q[:, 2]
    index = np.argsort(labels)
    s = labels[index]
    head = np.ones(len(s), dtype=bool)
    head[1:] = s[1:] != s[:-1]
    xyz = torch.from_numpy(points[index[head]]).to(dev).float()
    return maps, xyz


def kernel_route(sweeps_host, l2ws, c2ws, Ks, H, W, aabb, dev):
    import torch
    from s3gaussian_amd import lidar
    T = len(sweeps_host)
    V = len(c2ws) // T
    maps = torch.empty((T * V, H, W), dtype=torch.float32, device=dev)
    work = torch.empty(V * H * W, dtype=torch.int32, device=dev)
    cloud = lidar.LidarCloud(aabb, sum(int(s.shape[0]) for s in sweeps_host), dev)
    for t, rows in enumerate(sweeps_host):
        table = rows.to(dev)
        w2c = np.stack([np.linalg.inv(c2ws[t * V + v]) for v in range(V)])
        lidar.depth_maps(table, l2ws[t], w2c, Ks[t * V:(t + 1) * V], H, W, X_RANGE, 3, out=maps[t * V:(t + 1) * V], workspace=work)
        cloud.add(table, l2ws[t], X_RANGE, 3)
    return maps, cloud.finish(VOXEL)


def child(args):
    """One image size: the routes alternated in this process; prints one JSON line."""
    import torch
    from s3gaussian_amd import lidar
    H, W = args.size
    dev = torch.device("cuda:0")
    sweeps, l2ws, c2ws, Ks = workload(args.sweeps, args.rows, H, W)
    aabb = lidar.frustum_aabb(c2ws, Ks, H, W)
    hosts = [torch.from_numpy(s) for s in sweeps]
    routes = {"kernels": lambda: kernel_route(hosts, l2ws, c2ws, Ks, H, W, aabb, dev),
              "numpy": lambda: numpy_route(sweeps, l2ws, c2ws, Ks, H, W, aabb, dev)}
    times, res = {k: [] for k in routes}, {}
    for rep in range(args.warmup + args.reps):
        for k, fn in routes.items():
            res.pop(k, None)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res[k] = fn()
            torch.cuda.synchronize()
            if rep >= args.warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
    mk, mn = res["kernels"][0], res["numpy"][0]
    differ = int((mk != mn).sum())
    occupied = int((mn != 0).sum())
    print(json.dumps(dict(H=H, W=W, times=times, differ=differ, occupied=occupied, pixels=mk.numel(), cloud_kernels=int(res["kernels"][1].shape[0]),
                          cloud_numpy=int(res["numpy"][1].shape[0]), device=torch.cuda.get_device_name(0), threads=torch.get_num_threads())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sweeps", type=int, default=50)
    ap.add_argument("--rows", type=int, default=170_000)
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds one image size may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lidar_ab.txt"))
    ap.add_argument("--size", type=lambda s: tuple(int(x) for x in s.split("x")), default=None, help="(child) HxW")
    args = ap.parse_args()
    if args.size is not None:
        return child(args)
    if args.reps < 3:
        raise SystemExit("lidar_ab.py reports medians of at least 3 repetitions")
    lines = [f"# tools/lidar_ab.py --reps {args.reps} --warmup {args.warmup} --sweeps {args.sweeps} --rows {args.rows}: LiDAR set-up of a scene "
             f"({args.sweeps} sweeps x {args.rows} rows, 3 cameras each),",
             "# kernel route vs the numpy route a user had before, alternated in one process per image size, host wall clock, ms."]
    for H, W in SIZES:
        cmd = [sys.executable, os.path.abspath(__file__), "--size", f"{H}x{W}", "--reps", str(args.reps), "--warmup", str(args.warmup),
               "--sweeps", str(args.sweeps), "--rows", str(args.rows)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"lidar_ab.py: {H} x {W} did not finish within {args.step_timeout} s; nothing else is started")
        if done.returncode != 0:
            sys.stderr.write(done.stderr[-4000:])
            raise SystemExit(f"lidar_ab.py: {H} x {W} ended with status {done.returncode}; nothing else is started")
        r = json.loads(done.stdout.strip().splitlines()[-1])
        if len(lines) == 2:
            lines.append(f"# {r['device']}; {r['threads']} torch threads")
        lines.append(f"{H} x {W}: {args.sweeps * 3} maps ({args.sweeps * 3 * H * W * 4 / 1e6:.0f} MB fp32 on the device) + the initial cloud")
        med = {}
        for k, v in r["times"].items():
            med[k] = statistics.median(v)
            lines.append(f"  {k:8s} ms per scene: median {med[k]:.1f}  min {min(v):.1f}  max {max(v):.1f}")
        lines.append(f"  numpy / kernels (medians): {med['numpy'] / med['kernels']:.2f} x;  pixels that differ between the routes: {r['differ']} of "
                     f"{r['pixels']} ({r['occupied']} occupied);  cloud: {r['cloud_kernels']} labels (kernels), {r['cloud_numpy']} (numpy)")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
