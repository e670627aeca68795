"""The LiDAR scene set-up on the GPU (s3gaussian_amd/lidar.py, include/s3g_lidar.h) against the fixture recorded from the reference's
own readWaymoInfo / GridSample3D (tests/golden/make_golden_lidar.py) and against the numpy restatement tests/lidar_ref.py.

Bounds.  Every comparison is EXACT, with zero excluded pixels or rows.  Against the restatement: both sides evaluate the same float64
expressions in the same order without contraction (IEEE add, multiply, divide, round-to-nearest-even), the winner is an integer
maximum and the destination rows are integer scans, so the bits agree for any input.  Against the reference's recorded maps: numpy's
matmul sums in another order, which moves a world coordinate by a float64 ulp or so (1.4e-14 below 100 m); the fixture's generator
asserts margins of 1e-9 (pixel edges, pix.z, the aabb, half-integers of p / voxel), 1e-6 (range bounds) and a relative 1e-12 (fp32
rounding boundaries of the winning z), so no decision and no fp32 value can differ."""
import numpy as np
import pytest
import torch

from tests import lidar_ref as lr

pytestmark = pytest.mark.gpu

SENTINEL = -77777.0
ISENTINEL = -77777


@pytest.fixture(scope="module")
def fixture():
    return lr.load_fixture()


def _rot(yaw, pitch):
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    return np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]]) @ np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])


def _rig(V, H, W, seed, away=False):
    """-> (l2w [4,4], w2c [V,4,4], K [V,3,3]) float64: cameras that look along the ego x axis (opencv axes), fanned out in yaw; a
    focal length of 0.6 W keeps a good share of the points inside even a 1 x 1 image.  away=True: they look backwards."""
    rng = np.random.default_rng(seed)
    l2w = np.eye(4)
    l2w[:3, :3] = _rot(np.deg2rad(3.1), np.deg2rad(-0.7))
    l2w[:3, 3] = [0.8, -0.3, 0.05]
    to_cv = np.array([[0, 0, 1, 0], [-1, 0, 0, 0], [0, -1, 0, 0], [0, 0, 0, 1.0]])
    w2c, K = [], []
    for v in range(V):
        c2e = np.eye(4)
        yaw = np.deg2rad((v - (V - 1) / 2) * 25.0 + rng.uniform(-3, 3)) + (np.pi if away else 0.0)
        c2e[:3, :3] = _rot(yaw, np.deg2rad(rng.uniform(-2, 2)))
        c2e[:3, 3] = [1.5, 0.1 * v, 1.9]
        w2c.append(np.linalg.inv(l2w @ c2e @ to_cv))
        f = 0.6 * W + rng.uniform(0, 0.1)
        K.append(np.array([[f, 0.013, W / 2 + rng.uniform(-0.2, 0.2)], [0, f * 1.01, H / 2 + rng.uniform(-0.2, 0.2)], [0, 0, 1.0]]))
    return l2w, np.stack(w2c), np.stack(K)


def _points(N, seed, x_lo=-6.0, x_hi=90.0):
    """[N,3] fp32 in the ego frame, x on both sides of both range bounds; a third are near copies of earlier points (they contend)."""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(x_lo, x_hi, N), rng.uniform(-25, 25, N), rng.uniform(-3, 6, N)], axis=1)
    n3 = N // 3
    if n3:
        p[N - n3:] = p[:n3] + rng.normal(0, 0.002, (n3, 3))
    return p.astype(np.float32)


def _table(points, stride, offset, dev, shift=0):
    """The points inside a [N,stride] fp32 device table of other numbers; shift = 1: it starts 4 bytes past a 16-byte boundary."""
    N = len(points)
    rows = np.random.default_rng(N + stride).uniform(-500, 500, (N, stride)).astype(np.float32)
    rows[:, offset:offset + 3] = points
    flat = torch.full((N * stride + shift,), SENTINEL, dtype=torch.float32, device=dev)
    flat[shift:] = torch.from_numpy(rows).reshape(-1).to(dev)
    t = flat[shift:].view(N, stride)
    assert t.is_contiguous() and (N == 0 or t.data_ptr() % 16 == 4 * shift)
    return t, rows


def _guarded_call(rows_dev, l2w, w2c, K, H, W, offset, **kw):
    """lidar.depth_maps into sentinel-filled buffers with one canary row behind the output and behind the workspace."""
    from s3gaussian_amd import lidar
    V, dev = len(w2c), rows_dev.device
    out = torch.full((V * H + 1, W), SENTINEL, dtype=torch.float32, device=dev)
    work = torch.full((V * H * W + W,), ISENTINEL, dtype=torch.int32, device=dev)
    got = lidar.depth_maps(rows_dev, l2w, w2c, K, H, W, point_offset=offset, out=out[:V * H].view(V, H, W), workspace=work, **kw)
    assert got.data_ptr() == out.data_ptr()
    assert bool((out[V * H] == SENTINEL).all()) and bool((work[V * H * W:] == ISENTINEL).all())
    return got


def test_fixture_maps_are_the_reference_maps_bit_for_bit(fixture, gpu_device):
    f, dev = fixture, gpu_device
    H, W = int(f["H"]), int(f["W"])
    for t, (stride, offset) in enumerate(((3, 0), (10, 3))):
        pts = f[f"points{t}"]
        rows = np.zeros((len(pts), stride), dtype=np.float32)
        rows[:, offset:offset + 3] = pts
        w2c = np.stack([np.linalg.inv(c) for c in f["c2w"][3 * t:3 * t + 3]])
        got = _guarded_call(torch.from_numpy(rows).to(dev), f["l2w"][t], w2c, f["K"][3 * t:3 * t + 3], H, W, offset).cpu().numpy()
        for v in range(3):
            want = lr.sparse_map(f[f"map{3 * t + v}_index"], f[f"map{3 * t + v}_value"], H, W)
            assert np.array_equal(got[v] != 0, want != 0), (t, v)
            assert got[v].tobytes() == want.astype(np.float32).tobytes(), (t, v)


SHAPES = ((1, 1), (7, 5), (37, 53), (64, 64), (641, 97))


@pytest.mark.parametrize("N", [0, 1, 63, 64, 65, 257, 5000])
def test_depth_maps_equal_the_restatement(N, gpu_device):
    dev = gpu_device
    pts = _points(N, 100 + N)
    tables = {(3, 0): _table(pts, 3, 0, dev), (10, 3): _table(pts, 10, 3, dev)}
    hits = 0
    for (H, W) in SHAPES:
        for V in (1, 3, 5):
            l2w, w2c, K = _rig(V, H, W, seed=H * 7 + V)
            want = lr.depth_maps(pts, l2w, w2c, K, H, W, point_offset=0).astype(np.float32)
            hits += int((want != 0).sum())
            for (stride, offset), (dev_rows, _) in tables.items():
                got = _guarded_call(dev_rows, l2w, w2c, K, H, W, offset)
                assert got.dtype == torch.float32 and tuple(got.shape) == (V, H, W)
                assert got.cpu().numpy().tobytes() == want.tobytes(), (N, H, W, V, stride)
    assert hits > 0 or N <= 1      # (a single point may miss every camera)


def test_depth_maps_contended_misaligned_empty_and_repeatable(gpu_device):
    from s3gaussian_amd import lidar
    dev = gpu_device
    N = 5000
    l2w, w2c, K = _rig(3, 8, 8, seed=4)
    # 5 000 points back-projected from random positions inside camera 0's 8 x 8 image: every pixel of it is contended
    rng = np.random.default_rng(9)
    pix = np.stack([rng.uniform(0, 8, N), rng.uniform(0, 8, N), np.ones(N)]) * rng.uniform(3.0, 60.0, N)
    world = np.linalg.inv(w2c[0]) @ np.concatenate([np.linalg.inv(K[0]) @ pix, np.ones((1, N))])
    pts = (np.linalg.inv(l2w) @ world)[:3].T.astype(np.float32)
    want = lr.depth_maps(pts, l2w, w2c, K, 8, 8, point_offset=0).astype(np.float32)
    winner, _, counted, pixel = lr.winners(pts, l2w, w2c, K, 8, 8, point_offset=0)
    assert (winner[0] >= 0).all() and np.bincount(pixel[0][counted[0]], minlength=64).min() >= 20 and (winner[1:] >= 0).any()
    rows, _ = _table(pts, 10, 3, dev, shift=1)                             # 4 bytes past a 16-byte boundary
    a = _guarded_call(rows, l2w, w2c, K, 8, 8, 3)
    b = _guarded_call(rows, l2w, w2c, K, 8, 8, 3)
    assert a.cpu().numpy().tobytes() == want.tobytes() and torch.equal(a, b)
    rows3, _ = _table(pts, 3, 0, dev, shift=1)
    assert torch.equal(lidar.depth_maps(rows3, l2w, w2c, K, 8, 8, point_offset=0), a)
    # a rig that looks backwards sees nothing; neither does any rig when every point is outside the x range
    _, w2c_away, K_away = _rig(3, 37, 53, seed=5, away=True)
    assert int(lr.winners(pts, l2w, w2c_away, K_away, 37, 53, point_offset=0)[2].sum()) == 0
    assert not bool(_guarded_call(rows, l2w, w2c_away, K_away, 37, 53, 3).any())
    l2w, w2c, K = _rig(3, 37, 53, seed=5)
    assert bool(_guarded_call(rows, l2w, w2c, K, 37, 53, 3).any())
    assert not bool(_guarded_call(rows, l2w, w2c, K, 37, 53, 3, x_range=(80.0, 90.0)).any())
    far = _points(300, 11, x_lo=80.5, x_hi=95.0)
    far[:100, 0] = np.linspace(-9, -2.5, 100, dtype=np.float32)
    assert not bool(_guarded_call(_table(far, 10, 3, dev)[0], l2w, w2c, K, 37, 53, 3).any())
    # the bounds are strict, on the fp32 value
    edge = np.array([[-2.0, 0, 1], [80.0, 0.5, 1], [np.nextafter(np.float32(80), np.float32(0)), 0.1, 1]], dtype=np.float32)
    want = lr.depth_maps(edge, l2w, w2c, K, 37, 53, point_offset=0).astype(np.float32)
    assert (want != 0).sum() >= 1 and np.array_equal(want, lr.depth_maps(edge[2:], l2w, w2c, K, 37, 53, point_offset=0).astype(np.float32))
    assert _guarded_call(_table(edge, 3, 0, dev)[0], l2w, w2c, K, 37, 53, 0).cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(RuntimeError, match="S3G_LIDAR_MAX_CAMS"):
        lidar.depth_maps(rows, l2w, np.repeat(w2c, 3, axis=0), np.repeat(K, 3, axis=0), 8, 8)
    with pytest.raises(RuntimeError, match="cannot hold a point"):
        lidar.depth_maps(rows3, l2w, w2c, K, 8, 8, point_offset=3)


def _aabb_for(l2w):
    """A box in the world frame that cuts into the cloud of _points on every side."""
    c = l2w[:3, :3] @ np.array([40.0, 0, 1.5]) + l2w[:3, 3]
    return np.stack([c - [35.0, 22.0, 4.0], c + [35.0, 22.0, 4.0]])


@pytest.mark.parametrize("sizes", [(1000,), (777, 0, 1301, 300)], ids=["one_sweep", "three_sweeps_one_empty_one_removed"])
def test_cloud_rows_and_grid_sample_equal_the_restatement(sizes, gpu_device):
    from s3gaussian_amd import lidar
    dev = gpu_device
    l2ws = [_rig(1, 8, 8, seed=20 + t)[0] for t in range(len(sizes))]
    for t in range(len(sizes)):
        l2ws[t][:3, 3] += [0.9 * t, 0.05 * t, 0.0]
    aabb = _aabb_for(l2ws[0])
    sweeps = [_points(n, 30 + t) for t, n in enumerate(sizes)]
    if len(sizes) == 4:
        sweeps[3][:, 1] += 400.0                                          # the aabb removes this sweep entirely
    cloud = lidar.LidarCloud(aabb, sum(sizes), dev)
    want = []
    for t, pts in enumerate(sweeps):
        stride, offset = ((10, 3), (3, 0))[t % 2]
        cloud.add(_table(pts, stride, offset, dev, shift=t % 2)[0], l2ws[t], point_offset=offset)
        want.append(lr.cloud_rows(pts, l2ws[t], aabb, point_offset=0))
    if len(sizes) == 4:
        assert len(want[1]) == 0 and len(want[3]) == 0 and len(want[2]) % 64 != 0
    want = np.concatenate(want)
    got = cloud.kept()
    assert 0 < len(want) < sum(sizes) and len(want) % 64 != 0 and got.dtype == torch.float64
    assert got.cpu().numpy().tobytes() == want.tobytes()                   # bit-equal float64 rows, in the restatement's order
    with pytest.raises(RuntimeError, match="does not fit the capacity"):
        cloud.add(_table(sweeps[0], 3, 0, dev)[0], l2ws[0], point_offset=0)
    # a voxel of 0.013 leaves almost every point alone; 0.5 merges many
    for voxel in (0.013, 0.5):
        xyz_want, rows_want, labels = lr.grid_sample(want, voxel)
        xyz = cloud.finish(voxel_size=voxel)
        assert xyz.dtype == torch.float32 and xyz.cpu().numpy().tobytes() == xyz_want.tobytes(), voxel
        assert torch.equal(cloud.finish(voxel_size=voxel), xyz)
    assert len(xyz_want) < len(want)
    k = len(xyz_want) // 3
    sub = cloud.finish(voxel_size=0.5, num_pts=k, generator=torch.Generator().manual_seed(3))
    assert tuple(sub.shape) == (k, 3)
    full = {r.tobytes() for r in xyz_want}
    picked = [r.tobytes() for r in sub.cpu().numpy()]
    assert len(set(picked)) == k and set(picked) <= full                   # k distinct rows of the full output
    assert torch.equal(cloud.finish(voxel_size=0.5, num_pts=len(xyz_want)), xyz)
    empty = lidar.LidarCloud(aabb, 0, dev)
    assert tuple(empty.finish().shape) == (0, 3)


def test_fixture_cloud_has_the_reference_count_and_labels(fixture, gpu_device):
    from s3gaussian_amd import lidar
    f, dev = fixture, gpu_device
    cloud = lidar.LidarCloud(f["aabb"], 16000, dev)
    for t in range(2):
        cloud.add(torch.from_numpy(f[f"points{t}"]).to(dev), f["l2w"][t], point_offset=0)
    rows = cloud.kept().cpu().numpy()
    want = np.concatenate([lr.cloud_rows(f[f"points{t}"], f["l2w"][t], f["aabb"], point_offset=0) for t in range(2)])
    assert len(rows) == int(f["cloud_count_in"]) and rows.tobytes() == want.tobytes()
    xyz = cloud.finish().cpu().numpy()
    xyz_want, rows_want, labels = lr.grid_sample(want)
    assert len(xyz) == int(f["cloud_count"]) and np.array_equal(labels, f["cloud_labels"]) and xyz.tobytes() == xyz_want.tobytes()
    second = lidar.grid_sample(torch.from_numpy(f["second"]).to(dev)).cpu().numpy()
    second_want, second_rows, second_labels = lr.grid_sample(f["second"])
    assert len(second) == int(f["second_count"]) and second.tobytes() == second_want.tobytes()
    assert np.array_equal(second_labels, np.unique(f["second_labels"]))


def test_scene_from_lidar_feeds_create_from_points_and_a_training_step(fixture, gpu_device):
    from s3gaussian_amd import synth
    from s3gaussian_amd.pipeline import GaussianParams, default_hyper, default_opt, scene_from_lidar, training_step
    f, dev = fixture, gpu_device
    H, W = 208, 320                                                        # a third of the reference's load size
    Ks = f["K"].copy()
    Ks[:, :2] /= 3.0
    sweeps = []
    for t in range(2):
        rows = torch.zeros((len(f[f"points{t}"]), 10))
        rows[:, 3:6] = torch.from_numpy(f[f"points{t}"])
        sweeps.append(rows)
    hyper, opt = default_hyper(), default_opt()
    scene = scene_from_lidar(sweeps, f["l2w"], f["c2w"], Ks, H, W, 3, hyper, device=dev, generator=torch.Generator().manual_seed(0))
    maps, xyz, colors, aabb = scene["depth_maps"], scene["xyz"], scene["colors"], scene["aabb"]
    assert tuple(maps.shape) == (6, H, W) and maps.dtype == torch.float32 and maps.is_cuda
    w2c = np.stack([np.linalg.inv(c) for c in f["c2w"][3:6]])
    want = lr.depth_maps(f["points1"], f["l2w"][1], w2c, Ks[3:6], H, W, point_offset=0).astype(np.float32)
    assert maps[3:6].cpu().numpy().tobytes() == want.tobytes() and (want != 0).sum() > 100
    M = xyz.shape[0]
    assert M > 1000 and tuple(colors.shape) == (M, 3) and aabb.shape == (2, 3)
    pc = GaussianParams(3, hyper).create_from_points(xyz, colors, dev)
    assert pc._xyz.shape[0] == M == scene["gaussians"]._xyz.shape[0] and bool(torch.isfinite(pc._scaling).all())
    # one training step of a synthetic scene supervised with a map from depth_maps as gt_depth
    scn = synth.street_scene(P=5000, seed=0, width=W, height=H, n_frames=2)
    pc = GaussianParams(3, hyper)
    gs = scn["gaussians"]
    pc.init_from_tensors(gs["xyz"], gs["log_scales"], gs["rotations_raw"], gs["opacity_logit"], gs["shs"], dev)
    pc._deformation.deformation_net.set_aabb(*scn["aabb"])
    pc.training_setup(opt)
    cam = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in scn["cameras"][0].items()}
    g = torch.Generator().manual_seed(1)
    loss, pkg = training_step(pc, cam, torch.rand(3, H, W, generator=g).to(dev), maps[4][None], torch.rand(3, H, W, generator=g).to(dev),
                              hyper, opt, scn["bg"].to(dev))
    assert bool(torch.isfinite(loss)), loss
