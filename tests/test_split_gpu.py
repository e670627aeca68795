"""The dynamic / static point-cloud split on the GPU (s3gaussian_amd/split.py, include/s3g_split.h) against the fixture recorded from
the reference's own `GaussianModel.save_ply_split` (tests/golden/make_golden_split.py) and against the numpy restatement
tests/split_ref.py.

Bounds.  Masks, counts, offsets and both tables are EXACT, with zero excluded rows: every dx used here is checked (with numpy, inside
the test) to have no max|dx_i| within a relative 1e-5 of its mean, so a threshold that differs in its last bits moves no point; the
tables hold copied values and one fp32 add.  thre itself may differ from fp32(float64 mean) by 1 fp32 ulp: the kernel's float64 sum
runs in another order than numpy's, the two float64 sums differ by a few float64 ulp at most, and one rounding to fp32 of two such
neighbours lands on the same fp32 number or on adjacent ones."""
import math
import os

import numpy as np
import pytest
import torch

from tests import split_ref as sr

pytestmark = pytest.mark.gpu

SENTINEL = -77777.0


@pytest.fixture(scope="module")
def fixture():
    return sr.load_fixture()


def _dev(a, dev, shift=0):
    """The array on the device, contiguous; shift = 1 puts its first element one float past a 16-byte boundary."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not shift:
        return t.to(dev)
    flat = torch.full((t.numel() + shift,), SENTINEL, dtype=t.dtype, device=dev)
    flat[shift:] = t.reshape(-1).to(dev)
    v = flat[shift:].view(t.shape)
    assert v.is_contiguous() and (t.numel() == 0 or v.data_ptr() % 16 == 4 * shift)
    return v


def _guarded(rows, W, dev, shift=0):
    """-> (flat buffer, [rows + 1, W] view into it at `shift` floats): every float is the sentinel; the last row is the canary."""
    flat = torch.full((shift + (rows + 1) * W,), SENTINEL, dtype=torch.float32, device=dev)
    return flat, flat[shift:].view(rows + 1, W)


def _ulp_distance(a, b):
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def _model(f, dev):
    from s3gaussian_amd.pipeline import GaussianParams, default_hyper
    pc = GaussianParams(3, default_hyper())
    t = lambda k: torch.from_numpy(f[k])
    pc.init_from_tensors(t("xyz"), t("scaling"), t("rotation"), t("opacity"), torch.cat([t("f_dc"), t("f_rest")], dim=1), dev)
    return pc


def test_fixture_mask_threshold_count_and_tables(fixture, gpu_device):
    from s3gaussian_amd import split
    dev = gpu_device
    dx = _dev(fixture["dx"], dev)
    mask, thre, n_dynamic, offsets = split.motion_classify(dx, return_offsets=True)
    assert mask.dtype == torch.bool and thre.dim() == 0 and thre.dtype == torch.float32 and n_dynamic.dim() == 0 and thre.is_cuda and n_dynamic.is_cuda
    assert np.array_equal(mask.cpu().numpy(), fixture["mask"])
    assert int(n_dynamic) == int(fixture["mask"].sum())
    want = np.float32(fixture["mean_f64"])
    print(f"thre {float(thre):.9g}, fp32(float64 mean) {float(want):.9g}, torch's fp32 mean {float(fixture['thre']):.9g}")
    assert _ulp_distance(float(thre), want) <= 1
    assert np.array_equal(offsets.cpu().numpy(), sr.block_offsets(fixture["mask"]))
    inputs = [_dev(fixture[k], dev) for k in sr.INPUTS]
    dynamic, static = split.pack_ply_rows(*inputs, dx=dx, mask=mask, offsets=offsets)
    assert dynamic.cpu().numpy().tobytes() == fixture["dynamic_rows"].tobytes()
    assert static.cpu().numpy().tobytes() == fixture["static_rows"].tobytes()
    again = split.pack_ply_rows(*inputs, dx=dx, mask=mask)                    # offsets recomputed from the mask
    assert torch.equal(again[0], dynamic) and torch.equal(again[1], static)


def test_fixture_save_ply_split_writes_the_reference_files_and_leaves_the_model_alone(fixture, gpu_device, tmp_path):
    from s3gaussian_amd.plyio import read_vertices
    dev = gpu_device
    pc = _model(fixture, dev)
    xyz_object, xyz_before = pc._xyz, pc._xyz.detach().clone()
    g = torch.Generator().manual_seed(5)
    dx_list = [torch.randn(1000, 3, generator=g).to(dev) for _ in range(24)] + [_dev(fixture["dx"], dev)]
    paths = str(tmp_path / "pcd" / "dynamic.ply"), str(tmp_path / "pcd" / "static.ply")
    info = pc.save_ply_split(paths[0], paths[1], dx_list, None)
    assert info["n_dynamic"] == fixture["dynamic_rows"].shape[0] and info["n_static"] == fixture["static_rows"].shape[0]
    for path, rows in zip(paths, (fixture["dynamic_rows"], fixture["static_rows"])):
        names, cols = read_vertices(path)
        assert names == list(fixture["names"]) == pc.construct_list_of_attributes()
        got = np.stack([cols[n] for n in names], axis=1)
        assert got.dtype == np.float32 and got.tobytes() == rows.tobytes()
    assert pc._xyz is xyz_object and isinstance(pc._xyz, torch.nn.Parameter) and torch.equal(pc._xyz.detach(), xyz_before)
    with pytest.raises(IndexError):
        pc.save_ply_split(paths[0], paths[1], dx_list[:24], None)


@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 256, 257, 1000, 70001])
def test_shapes_against_the_restatement(P, gpu_device):
    """Wave and block seams, one multi-partial size; every SH degree; dx and mask present and absent; inputs and outputs aligned to 16
    bytes and one float past (the scalar head of a run); one canary row behind every output and one float in front of the shifted ones."""
    from s3gaussian_amd import split
    dev = gpu_device
    for R in (0, 3, 8, 15):
        W = 17 + 3 * R
        mdl = sr.random_model(P, R, seed=1000 * R + P)
        mask_ref, thre_ref, m = sr.motion_mask(mdl["dx"])
        assert sr.tie_free(m, thre_ref)
        nd = int(mask_ref.sum())
        full = {True: sr.table(*(mdl[k] for k in sr.INPUTS), dx=mdl["dx"]), False: sr.table(*(mdl[k] for k in sr.INPUTS))}
        for shift in (0, 1):
            inputs = [_dev(mdl[k], dev, shift) for k in sr.INPUTS]
            dx = _dev(mdl["dx"], dev, shift)
            mask, thre, n_dynamic, offsets = split.motion_classify(dx, return_offsets=True)
            assert np.array_equal(mask.cpu().numpy(), mask_ref), (P, R, shift)
            assert int(n_dynamic) == nd and _ulp_distance(float(thre), thre_ref) <= 1
            assert np.array_equal(offsets.cpu().numpy(), sr.block_offsets(mask_ref))
            for with_dx in (False, True):
                want = full[with_dx]
                flat, out = _guarded(P, W, dev, shift)
                rows = split.pack_ply_rows(*inputs, dx=dx if with_dx else None, out=out)
                assert rows.data_ptr() == out.data_ptr() and rows.shape == (P, W)
                assert rows.cpu().numpy().tobytes() == want.tobytes(), (P, R, shift, with_dx, "whole")
                assert bool((out[P] == SENTINEL).all()) and bool((flat[:shift] == SENTINEL).all())
                want_d, want_s = sr.split_tables(mask_ref, want)
                (flat_d, out_d), (flat_s, out_s) = _guarded(nd, W, dev, shift), _guarded(P - nd, W, dev, shift)
                got_d, got_s = split.pack_ply_rows(*inputs, dx=dx if with_dx else None, mask=mask, offsets=offsets, out=(out_d, out_s))
                assert got_d.shape == (nd, W) and got_s.shape == (P - nd, W)
                assert got_d.cpu().numpy().tobytes() == want_d.tobytes(), (P, R, shift, with_dx, "dynamic")
                assert got_s.cpu().numpy().tobytes() == want_s.tobytes(), (P, R, shift, with_dx, "static")
                assert bool((out_d[nd] == SENTINEL).all()) and bool((out_s[P - nd] == SENTINEL).all())
                assert bool((flat_d[:shift] == SENTINEL).all()) and bool((flat_s[:shift] == SENTINEL).all())


def test_degenerate_classes(gpu_device):
    from s3gaussian_amd import split
    dev = gpu_device
    P, R = 777, 15
    mdl = sr.random_model(P, R, seed=9)
    inputs = [_dev(mdl[k], dev) for k in sr.INPUTS]
    full = sr.table(*(mdl[k] for k in sr.INPUTS))
    # every max|dx_i| equal: the mean IS that value (P equal fp32 numbers sum exactly in float64), nothing exceeds it
    same = np.tile(np.array([[0.25, -0.3, 0.1]], dtype=np.float32), (P, 1))
    same[::2] = [-0.3, 0.2, 0.3]
    mask, thre, n_dynamic, offsets = split.motion_classify(_dev(same, dev), return_offsets=True)
    assert int(n_dynamic) == 0 and not bool(mask.any()) and float(thre) == float(np.float32(0.3)) and int(offsets.abs().sum()) == 0
    dynamic, static = split.pack_ply_rows(*inputs, mask=mask, offsets=offsets)
    assert dynamic.shape == (0, 62) and static.cpu().numpy().tobytes() == full.tobytes()
    # one outlier: exactly one dynamic row, the others keep their order
    one = np.full((P, 3), 0.01, dtype=np.float32)
    one[300] = [0.0, -5.0, 1.0]
    mask, thre, n_dynamic, offsets = split.motion_classify(_dev(one, dev), return_offsets=True)
    assert int(n_dynamic) == 1 and mask.nonzero().flatten().tolist() == [300] and offsets.tolist() == [0, 0, 1, 1, 1]
    dynamic, static = split.pack_ply_rows(*inputs, mask=mask, offsets=offsets)
    assert dynamic.cpu().numpy().tobytes() == full[300:301].tobytes()
    assert static.cpu().numpy().tobytes() == np.delete(full, 300, axis=0).tobytes()
    # everything but one dynamic
    most = np.full((P, 3), 1.0, dtype=np.float32)
    most[5] = 0.0
    mask, _, n_dynamic = split.motion_classify(_dev(most, dev))
    assert int(n_dynamic) == P - 1
    dynamic, static = split.pack_ply_rows(*inputs, mask=mask)
    assert static.cpu().numpy().tobytes() == full[5:6].tobytes() and dynamic.cpu().numpy().tobytes() == np.delete(full, 5, axis=0).tobytes()
    # nothing at all
    empty = [torch.zeros((0,) + tuple(t.shape[1:]), device=dev) for t in inputs]
    mask, thre, n_dynamic = split.motion_classify(torch.zeros(0, 3, device=dev))
    assert mask.shape == (0,) and math.isnan(float(thre)) and int(n_dynamic) == 0
    assert split.pack_ply_rows(*empty).shape == (0, 62)
    dynamic, static = split.pack_ply_rows(*empty, mask=mask)
    assert dynamic.shape == (0, 62) and static.shape == (0, 62)


def test_outputs_too_small_or_of_another_kind_are_refused(gpu_device):
    from s3gaussian_amd import split
    dev = gpu_device
    mdl = sr.random_model(100, 3, seed=2)
    inputs = [_dev(mdl[k], dev) for k in sr.INPUTS]
    before = split.calls
    with pytest.raises(RuntimeError, match="out must hold"):
        split.pack_ply_rows(*inputs, out=torch.empty(99, 26, device=dev))
    with pytest.raises(RuntimeError, match="out must hold"):
        split.pack_ply_rows(*inputs, out=torch.empty(100, 62, device=dev))
    with pytest.raises(RuntimeError, match="offsets without a mask"):
        split.pack_ply_rows(*inputs, offsets=torch.zeros(2, dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError, match="offsets must be"):
        split.pack_ply_rows(*inputs, mask=torch.zeros(100, dtype=torch.bool, device=dev), offsets=torch.zeros(7, dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError, match="mask must be"):
        split.pack_ply_rows(*inputs, mask=torch.zeros(99, dtype=torch.bool, device=dev))
    with pytest.raises(RuntimeError, match=r"dx must be"):
        split.pack_ply_rows(*inputs, dx=torch.zeros(99, 3, device=dev))
    assert split.calls == before


def test_two_runs_are_bit_identical(gpu_device):
    from s3gaussian_amd import split
    dev = gpu_device
    P = 70001
    mdl = sr.random_model(P, 15, seed=31)
    inputs = [_dev(mdl[k], dev) for k in sr.INPUTS]
    dx = _dev(mdl["dx"], dev)
    runs = []
    for _ in range(2):
        mask, thre, n_dynamic, offsets = split.motion_classify(dx, return_offsets=True)
        dynamic, static = split.pack_ply_rows(*inputs, dx=dx, mask=mask, offsets=offsets)
        runs.append((mask, thre.reshape(1).view(torch.int32), n_dynamic.reshape(1), offsets, dynamic.view(torch.int32), static.view(torch.int32)))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_save_ply_on_the_device_writes_the_bytes_of_the_numpy_route(fixture, gpu_device, tmp_path):
    from s3gaussian_amd import split
    from s3gaussian_amd.plyio import write_vertices
    pc = _model(fixture, gpu_device)
    before = split.calls
    pc.save_ply(str(tmp_path / "device.ply"))
    assert split.calls == before + 1
    n = lambda t_: t_.detach().cpu().numpy()                 # the route of GaussianParams.save_ply before the packer, restated
    xyz = n(pc._xyz)
    cols = [xyz, np.zeros_like(xyz), n(pc._features_dc.transpose(1, 2).flatten(start_dim=1).contiguous()),
            n(pc._features_rest.transpose(1, 2).flatten(start_dim=1).contiguous()), n(pc._opacity), n(pc._scaling), n(pc._rotation)]
    write_vertices(str(tmp_path / "numpy.ply"), pc.construct_list_of_attributes(), np.concatenate(cols, axis=1))
    a, b = open(tmp_path / "device.ply", "rb").read(), open(tmp_path / "numpy.ply", "rb").read()
    assert len(a) > 1000 * 62 * 4 and a == b
    cpu = _model(fixture, "cpu")                             # the CPU model keeps the numpy route: same file again
    cpu.save_ply(str(tmp_path / "cpu.ply"))
    assert open(tmp_path / "cpu.ply", "rb").read() == b and split.calls == before + 1


def test_dynamic_point_count_is_the_training_logs_number(fixture, gpu_device):
    from s3gaussian_amd.pipeline import dynamic_point_count
    dx = _dev(fixture["dx"], gpu_device).requires_grad_(True)          # the training loop's dx carries a graph
    n = dynamic_point_count(dx * 1.0)
    assert torch.is_tensor(n) and n.is_cuda and n.dim() == 0 and not n.requires_grad
    m = np.abs(fixture["dx"]).max(axis=1)
    assert int(n) == int((m > m.mean()).sum()) == int(fixture["mask"].sum())


def _deforming_model(dev, **hyper):
    from s3gaussian_amd.pipeline import GaussianParams, default_hyper
    P = 1500
    g = torch.Generator().manual_seed(11)
    r = lambda *s: torch.randn(*s, generator=g)
    torch.manual_seed(0)
    pc = GaussianParams(3, default_hyper(**hyper))
    pc.init_from_tensors(r(P, 3) * 0.6, r(P, 3) - 3, r(P, 4), r(P, 1), r(P, 16, 3) * 0.3, dev)
    net = pc._deformation.deformation_net
    with torch.no_grad():
        if not hyper.get("no_dx"):
            for p in net.pos_deform.parameters():
                p.add_(0.05 * torch.randn_like(p))
        for p in net.grid.grids.parameters():
            p.add_(0.2 * torch.randn_like(p))
    return pc


def test_save_split_point_clouds_exports_the_model_at_one_timestamp(gpu_device, tmp_path):
    from s3gaussian_amd import split
    from s3gaussian_amd.pipeline import _uniform_time, save_split_point_clouds
    from s3gaussian_amd.plyio import read_vertices
    pc = _deforming_model(gpu_device)
    paths = str(tmp_path / "dynamic.ply"), str(tmp_path / "static.ply")
    info = save_split_point_clouds(pc, 0.5, paths[0], paths[1])
    net = pc._deformation.deformation_net
    with torch.no_grad():
        dx = net.deform_heads(pc.get_xyz, _uniform_time(0.5, gpu_device), uniform_time=True, reg_weights=None, need_feat=False)[0]
    assert float(dx.abs().max()) > 0
    mask = split.motion_classify(dx)[0].cpu().numpy()
    assert info["n_dynamic"] == int(mask.sum()) and info["n_static"] == 1500 - int(mask.sum())
    n = lambda t_: t_.detach().cpu().numpy()
    full = sr.table(n(pc._xyz), n(pc._features_dc), n(pc._features_rest), n(pc._opacity), n(pc._scaling), n(pc._rotation), dx=n(dx))
    for path, rows in zip(paths, sr.split_tables(mask, full)):
        names, cols = read_vertices(path)
        assert names == pc.construct_list_of_attributes()
        assert np.stack([cols[k] for k in names], axis=1).tobytes() == rows.tobytes()


def test_a_static_model_is_refused_by_name(gpu_device, tmp_path):
    from s3gaussian_amd.pipeline import save_split_point_clouds
    pc = _deforming_model(gpu_device, no_dx=True)
    with pytest.raises(RuntimeError, match="no_dx"):
        save_split_point_clouds(pc, 0.5, str(tmp_path / "d.ply"), str(tmp_path / "s.ply"))
    assert not os.path.exists(tmp_path / "d.ply")
    with pytest.raises(RuntimeError, match="coarse"):
        save_split_point_clouds(_deforming_model(gpu_device), 0.5, str(tmp_path / "d.ply"), str(tmp_path / "s.ply"), stage="coarse")
