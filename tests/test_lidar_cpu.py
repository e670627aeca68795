"""CPU-only: the restatement tests/lidar_ref.py against what the reference's own readWaymoInfo and GridSample3D computed
(tests/golden/lidar.npz, written by tests/golden/make_golden_lidar.py), the host helpers of s3gaussian_amd.lidar, and the parts of the
s3g_lidar_* entry points that answer before any device call.

Bounds.  Everything compared here is EXACT.  The restatement sums in the kernels' order, numpy's matmul in BLAS's; the two world
coordinates differ by a float64 ulp or so.  The fixture's generator asserts that no counted u or v lies within 1e-9 of an integer, no
pix.z within 1e-9 of 0, no x within 1e-6 of a range bound, no winning z within a relative 1e-12 of an fp32 rounding boundary, no
p / voxel within 1e-9 of a half-integer and no world coordinate within 1e-9 of the aabb: five orders of magnitude and more above such
a difference (coordinates below 100 m: an ulp is 1.4e-14), so no decision and no fp32 value can differ."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import lidar_ref as lr


@pytest.fixture(scope="module")
def fixture():
    return lr.load_fixture()


def _sweeps(f):
    return [f["points0"], f["points1"]]


def _cams(f, t):
    w2c = np.stack([np.linalg.inv(c) for c in f["c2w"][3 * t:3 * t + 3]])
    return w2c, f["K"][3 * t:3 * t + 3]


def test_fixture_holds_what_its_generator_promises(fixture):
    f = fixture
    assert (int(f["H"]), int(f["W"])) == (640, 960) and float(f["voxel"]) == lr.VOXEL
    assert f["points0"].shape == (8000, 3) and f["points1"].shape == (8000, 3) and f["points0"].dtype == np.float32
    assert f["l2w"].shape == (2, 4, 4) and np.array_equal(f["l2w"][0], np.eye(4)) and not np.allclose(f["l2w"][1], np.eye(4))
    assert f["c2w"].shape == (6, 4, 4) and f["K"].shape == (6, 3, 3)
    assert int(f["contended"]) >= 300 and int(f["neither"]) >= 100 and (f["shares"] >= 0.2).all()
    # points on both sides of both range bounds, and points the aabb removes
    x = np.concatenate(_sweeps(f))[:, 0]
    assert (x < -2).any() and (x > 80).any() and int(f["cloud_count_in"]) < int(((x > -2) & (x < 80)).sum())


def test_restatement_reproduces_the_six_reference_maps_bit_for_bit(fixture):
    f = fixture
    H, W = int(f["H"]), int(f["W"])
    for t in range(2):
        w2c, K = _cams(f, t)
        maps = lr.depth_maps(_sweeps(f)[t], f["l2w"][t], w2c, K, H, W, point_offset=0)
        for v in range(3):
            want = lr.sparse_map(f[f"map{3 * t + v}_index"], f[f"map{3 * t + v}_value"], H, W)
            assert np.array_equal(maps[v] != 0, want != 0), (t, v)                                   # occupancy identical
            assert maps[v].astype(np.float32).tobytes() == want.astype(np.float32).tobytes(), (t, v)
            assert (want != 0).sum() > 100


def test_a_first_wins_or_nearest_wins_map_fails_the_fixture(fixture):
    """The collisions are there for a reason: the two wrong rules give other maps."""
    f = fixture
    H, W = int(f["H"]), int(f["W"])
    w2c, K = _cams(f, 0)
    winner, zs, counted, pixel = lr.winners(f["points0"], f["l2w"][0], w2c, K, H, W, point_offset=0)
    want = lr.sparse_map(f["map0_index"], f["map0_value"], H, W).reshape(-1)
    idx = np.where(counted[0])[0]
    first = np.zeros(H * W)
    first[pixel[0, idx[::-1]]] = zs[0][idx[::-1]]                # the lowest row assigned last
    nearest = np.full(H * W, np.inf)
    np.minimum.at(nearest, pixel[0, idx], zs[0][idx])
    nearest[np.isinf(nearest)] = 0
    assert (first != want).sum() > 50 and (nearest != want).sum() > 50


def test_restatement_reproduces_the_reference_cloud_and_its_labels(fixture):
    f = fixture
    cloud = np.concatenate([lr.cloud_rows(_sweeps(f)[t], f["l2w"][t], f["aabb"], point_offset=0) for t in range(2)])
    assert len(cloud) == int(f["cloud_count_in"])
    xyz, rows, labels = lr.grid_sample(cloud)
    assert len(xyz) == int(f["cloud_count"]) and np.array_equal(labels, f["cloud_labels"])      # labels sorted-equal, count equal
    # every output point is the fp32 of an input point carrying that label, and the lowest such row
    all_labels, _ = lr.grid_labels(cloud)
    assert np.array_equal(all_labels[rows], labels) and xyz.tobytes() == cloud[rows].astype(np.float32).tobytes()
    for m in (0, 1, len(rows) // 2, len(rows) - 1):
        assert rows[m] == np.flatnonzero(all_labels == labels[m])[0]
    assert (np.diff(labels) > 0).all()


def test_restatement_reproduces_the_labels_of_a_direct_grid_sample_call(fixture):
    f = fixture
    labels, b = lr.grid_labels(f["second"])
    assert np.array_equal(labels, f["second_labels"])
    xyz, rows, heads = lr.grid_sample(f["second"])
    assert len(xyz) == int(f["second_count"]) == len(np.unique(f["second_labels"]))
    # the quirk: b is the maximum, not the extent + 1, so (q.y, q.z = b.z) and (q.y + 1, q.z = 0) share a label
    q = np.around(f["second"] / lr.VOXEL)
    q = (q - q.min(axis=0)).astype(np.int64)
    assert np.array_equal(b, q.max(axis=0))
    voxels = len(np.unique(q, axis=0))
    assert voxels >= len(xyz)


def test_frustum_aabb_and_init_colors_against_the_recorded_values(fixture):
    from s3gaussian_amd import lidar
    f = fixture
    aabb = lidar.frustum_aabb(f["c2w"], f["K"], int(f["H"]), int(f["W"]))
    assert aabb.dtype == np.float64 and aabb.tobytes() == f["aabb"].tobytes()
    assert lidar.sh2rgb(f["uniform"] / 255.0).tobytes() == f["colors"].tobytes()
    g = torch.Generator().manual_seed(7)
    u = torch.rand((5, 3), generator=g, dtype=torch.float64)
    c = lidar.init_colors(5, torch.Generator().manual_seed(7))
    assert c.dtype == torch.float64 and torch.equal(c, lidar.sh2rgb(u / 255.0)) and float(c.min()) >= 0.5


def test_read_sweep_returns_the_raw_rows(tmp_path):
    from s3gaussian_amd import lidar
    rows = np.arange(70, dtype=np.float32).reshape(7, 10)
    rows.tofile(tmp_path / "000.bin")
    got = lidar.read_sweep(str(tmp_path / "000.bin"))
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), rows)
    np.arange(7, dtype=np.float32).tofile(tmp_path / "bad.bin")
    with pytest.raises(ValueError):
        lidar.read_sweep(str(tmp_path / "bad.bin"))


def test_library_exports_the_lidar_entry_points():
    from s3gaussian_amd import _lib, lidar
    L = lidar._bind()
    for name in ("s3g_lidar_depth_workspace_bytes", "s3g_lidar_depth_maps", "s3g_lidar_count_words", "s3g_lidar_cloud_add",
                 "s3g_lidar_grid_workspace_bytes", "s3g_lidar_grid_range", "s3g_lidar_grid_keys", "s3g_lidar_grid_heads",
                 "s3g_lidar_grid_gather"):
        assert hasattr(L, name) and name in _lib.EXPORTED_SYMBOLS
    assert L.s3g_abi_version() == _lib.ABI_VERSION


def test_structs_match_the_header():
    from s3gaussian_amd import lidar
    from tests.test_abi_cpu import _struct_fields
    assert _struct_fields("s3g_lidar.h", "s3g_lidar_sweep") == [f[0] for f in lidar._Sweep._fields_]
    assert _struct_fields("s3g_lidar.h", "s3g_lidar_cams") == [f[0] for f in lidar._Cams._fields_]
    assert _struct_fields("s3g_lidar.h", "s3g_lidar_grid_stats") == [f[0] for f in lidar._GridStats._fields_]
    assert C.sizeof(lidar._Sweep) == 8 + 4 * 4 + 2 * 8 + 12 * 8
    assert C.sizeof(lidar._Cams) == 4 * 4 + 8 * 12 * 8 + 8 * 9 * 8 and C.sizeof(lidar._GridStats) == 48
    header = open(os.path.join(os.path.dirname(lr.GOLDEN), "..", "..", "include", "s3g_lidar.h")).read()
    assert f"#define S3G_LIDAR_MAX_CAMS {lidar.MAX_CAMS}" in header and f"#define S3G_LIDAR_BLOCK {lidar.BLOCK}" in header


def test_sizes_and_refusals_before_any_device_call():
    """Argument validation only: every refused call returns S3G_ERR_INVALID_ARG (1) before the library touches a device; the pointers
    are made-up addresses that are never dereferenced."""
    from s3gaussian_amd import lidar
    L = lidar._bind()
    assert [L.s3g_lidar_count_words(n) for n in (0, 1, 256, 257, 170000)] == [2, 2, 2, 3, 666]
    assert L.s3g_lidar_depth_workspace_bytes(3, 640, 960) == 3 * 640 * 960 * 4
    assert [L.s3g_lidar_depth_workspace_bytes(*a) for a in ((0, 4, 4), (9, 4, 4), (1, 0, 4), (1, 4, 0), (8, 16384, 16384))] == [0] * 5
    assert L.s3g_lidar_grid_workspace_bytes(1) == L.s3g_lidar_grid_workspace_bytes(8_500_000) == 512 * 6 * 8
    a = 0x1000

    def sweep(N=5, stride=10, offset=3, rows=a):
        return lidar._Sweep(rows, N, stride, offset, 0, -2.0, 80.0)

    def cams(V=3, H=8, W=8):
        return lidar._Cams(V, H, W, 0)

    dm = lambda s, c, depth=a, ws=a: L.s3g_lidar_depth_maps(C.byref(s) if s is not None else None, C.byref(c) if c is not None else None,
                                                             depth, ws, None)
    refused = {
        "depth NULL sweep": dm(None, cams()),
        "depth NULL cams": dm(sweep(), None),
        "depth NULL depth": dm(sweep(), cams(), depth=None),
        "depth NULL workspace": dm(sweep(), cams(), ws=None),
        "depth NULL rows": dm(sweep(rows=None), cams()),
        "depth N < 0": dm(sweep(N=-1), cams()),
        "depth stride too small": dm(sweep(stride=5), cams()),
        "depth stride 3 with offset 3": dm(sweep(stride=3), cams()),
        "depth negative offset": dm(sweep(offset=-1), cams()),
        "depth V = 0": dm(sweep(), cams(V=0)),
        "depth V = 9": dm(sweep(), cams(V=9)),
        "depth H = 0": dm(sweep(), cams(H=0)),
        "depth W = 0": dm(sweep(), cams(W=0)),
        "depth V H W = 2^31": dm(sweep(), cams(V=8, H=16384, W=16384)),
    }
    box = (C.c_double * 6)(0, 0, 0, 1, 1, 1)
    add = lambda s, aabb=box, cloud=a, cap=10, total=a, off=a: L.s3g_lidar_cloud_add(C.byref(s) if s is not None else None, aabb, cloud,
                                                                                     cap, total, off, None)
    assert add(sweep(N=0, rows=None), aabb=None, cloud=None, total=None, off=None) == 0
    refused.update({
        "add NULL sweep": add(None),
        "add N < 0": add(sweep(N=-1)),
        "add stride too small": add(sweep(stride=4)),
        "add NULL rows": add(sweep(rows=None)),
        "add NULL aabb": add(sweep(), aabb=None),
        "add NULL cloud": add(sweep(), cloud=None),
        "add NULL total": add(sweep(), total=None),
        "add NULL offsets": add(sweep(), off=None),
        "add negative capacity": add(sweep(), cap=-1),
        "range n = 0": L.s3g_lidar_grid_range(0, a, 0.013, a, a, None),
        "range voxel = 0": L.s3g_lidar_grid_range(5, a, 0.0, a, a, None),
        "range voxel NaN": L.s3g_lidar_grid_range(5, a, float("nan"), a, a, None),
        "range NULL cloud": L.s3g_lidar_grid_range(5, None, 0.013, a, a, None),
        "range NULL stats": L.s3g_lidar_grid_range(5, a, 0.013, None, a, None),
        "range NULL workspace": L.s3g_lidar_grid_range(5, a, 0.013, a, None, None),
        "keys n < 0": L.s3g_lidar_grid_keys(-1, a, 0.013, a, a, None),
        "keys NULL keys": L.s3g_lidar_grid_keys(5, a, 0.013, a, None, None),
        "heads n = 0": L.s3g_lidar_grid_heads(0, a, a, None),
        "heads NULL keys": L.s3g_lidar_grid_heads(5, None, a, None),
        "heads NULL offsets": L.s3g_lidar_grid_heads(5, a, None, None),
        "gather n = 0": L.s3g_lidar_grid_gather(0, a, a, a, a, a, 5, None),
        "gather NULL perm": L.s3g_lidar_grid_gather(5, a, None, a, a, a, 5, None),
        "gather NULL out": L.s3g_lidar_grid_gather(5, a, a, a, a, None, 5, None),
        "gather negative rows": L.s3g_lidar_grid_gather(5, a, a, a, a, a, -1, None),
    })
    for what, rc in refused.items():
        assert rc == 1, (what, rc)
    assert b"s3g_lidar" in L.s3g_last_error()


def test_cpu_tensors_are_refused_by_name():
    from s3gaussian_amd import lidar
    before = lidar.calls
    eye = np.eye(4)
    with pytest.raises(RuntimeError, match="rows must live on the GPU.*no CPU fallback"):
        lidar.depth_maps(torch.zeros(4, 10), eye, eye[None], np.eye(3)[None], 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lidar.LidarCloud(np.array([[0.0, 0, 0], [1, 1, 1]]), 4, "cpu")
    with pytest.raises(RuntimeError, match="points must live on the GPU.*no CPU fallback"):
        lidar.grid_sample(torch.zeros(4, 3, dtype=torch.float64))
    assert lidar.calls == before


def test_the_label_guard_refuses_a_grid_of_two_to_the_53():
    from s3gaussian_amd import lidar
    assert lidar.check_label_range([0, 0, 0, 1 << 20, 1 << 20, (1 << 13) - 1]) == (1 << 40) * ((1 << 13) - 1)
    assert lidar.check_label_range([-5, 7, 0, 0, 0, 0]) == 0                       # a flat cloud: every label 0, as the reference's
    with pytest.raises(RuntimeError, match="2\\^53"):
        lidar.check_label_range([0, 0, 0, 1 << 20, 1 << 20, 1 << 13])
    with pytest.raises(RuntimeError, match="2\\^53"):
        lidar.check_label_range([0, 0, 0, 1 << 62, 4, 4])                          # would wrap an int64 product
    with pytest.raises(ValueError, match="2\\^53"):
        lr.grid_labels(np.array([[0.0, 0, 0], [1e9 * 0.013, 1e5 * 0.013, 1e3 * 0.013]]))
