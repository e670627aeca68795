"""Scale / rotation / opacity deformation (no_ds / no_dr / no_do off) on the fused route, the part that needs no GPU: which switch
combinations `Deformation._fused_geometry_ok` admits, that `_fused_ok` keeps its value for all of them, the ctypes mirror of
s3g_geom_params, and the refusals that come before anything is launched."""
import ctypes as C
import itertools
from types import SimpleNamespace

import pytest
import torch

SMALL = dict(grid_dimensions=2, input_coordinate_dim=4, output_coordinate_dim=32, resolution=[8, 8, 8, 5])
SUBSETS = [s for s in itertools.product((True, False), repeat=3) if not all(s)]      # (no_ds, no_dr, no_do): the seven with a head on


def _net(**over):
    from s3gaussian_amd.deformation import deform_network
    from s3gaussian_amd.pipeline import default_hyper
    return deform_network(default_hyper(kplanes_config=SMALL, **over)).deformation_net


@pytest.mark.parametrize("no_dx", [False, True])
@pytest.mark.parametrize("no_ds,no_dr,no_do", SUBSETS)
def test_geometry_route_admits_every_head_subset(no_ds, no_dr, no_do, no_dx):
    net = _net(no_ds=no_ds, no_dr=no_dr, no_do=no_do, no_dx=no_dx)
    assert net._fused_geometry_ok()
    assert not net._fused_ok()                      # the MLP kernels' own predicate keeps its value
    mods = net._geometry_modules()
    assert [m is None for m in mods] == [no_ds, no_dr, no_do]


def test_geometry_route_is_off_for_the_default_and_the_static_configuration():
    for over in (dict(), dict(no_dx=True)):
        net = _net(**over)
        assert net._fused_ok() and not net._fused_geometry_ok()


@pytest.mark.parametrize("over", [dict(static_mlp=True), dict(empty_voxel=True), dict(grid_pe=2), dict(no_dshs=True), dict(feat_head=False)])
def test_geometry_route_refuses_the_other_switches(over):
    assert len(SUBSETS) == 7
    for no_ds, no_dr, no_do in SUBSETS:
        net = _net(no_ds=no_ds, no_dr=no_dr, no_do=no_do, **over)
        assert not net._fused_geometry_ok() and not net._fused_ok()
    assert not _net(**over)._fused_geometry_ok()   # and with every geometry head off


def test_flow_guard_admits_the_geometry_configuration_with_a_position_head():
    from s3gaussian_amd import pipeline
    stub = lambda net: SimpleNamespace(get_xyz=SimpleNamespace(is_cuda=True, device=torch.device("cpu")), max_sh_degree=3,
                                       _deformation=SimpleNamespace(deformation_net=net))
    pipe = SimpleNamespace(convert_SHs_python=True)
    assert pipeline._fused_route(stub(_net(no_ds=False, no_dr=False, no_do=False)), pipe)
    assert not pipeline._fused_route(stub(_net(no_ds=False, no_dr=False, no_do=False, no_dx=True)), pipe)
    assert not pipeline._fused_route(stub(_net(no_ds=False, static_mlp=True)), pipe)


def test_geom_params_struct_matches_the_header():
    from s3gaussian_amd import _lib, mlp_geom
    from tests.test_abi_cpu import _struct_fields
    want = ["W0", "b0", "C1", "cb1", "C2", "cb2", "R1", "rb1", "R2", "rb2", "O1", "ob1", "O2", "ob2"]
    assert _struct_fields("s3g_mlp_geom.h", "s3g_geom_params") == want == [f[0] for f in mlp_geom._GeomParams._fields_]
    assert C.sizeof(mlp_geom._GeomParams) == 14 * 8
    L = _lib.lib()
    for name in ("s3g_deform_geom_stash_bytes", "s3g_deform_geom_workspace_bytes", "s3g_deform_geom_forward", "s3g_deform_geom_backward"):
        assert hasattr(L, name) and name in _lib.EXPORTED_SYMBOLS
    assert L.s3g_abi_version() == _lib.ABI_VERSION == 16


def test_sizes_and_refusals_before_any_device_call():
    """Host code only: the two size functions, P == 0 returning at once, and S3G_ERR_INVALID_ARG (1) with the library's error text for
    a call without a head, without a requested head's weights, or with a negative P.  The pointers are made-up addresses that are never
    dereferenced."""
    from s3gaussian_amd import mlp_geom
    L = mlp_geom._bind()
    L.s3g_last_error.restype = C.c_char_p
    image = L.s3g_deform_geom_stash_bytes(0)
    assert image % 1024 == 0 and 100 * 1024 < image <= 160 * 1024             # the LDS image: whole 1 KiB rows, inside one CU's LDS
    assert L.s3g_deform_geom_stash_bytes(-5) == image
    for P in (1, 32, 33, 70_001):
        tiles = (P + 31) // 32
        assert L.s3g_deform_geom_stash_bytes(P) == image + 4 * P * 64 * 4 + tiles * 4 * 64 * 4
        assert L.s3g_deform_geom_workspace_bytes(P) == L.s3g_deform_geom_workspace_bytes(0) + 4 * P * 64 * 4
    assert L.s3g_deform_geom_workspace_bytes(0) == 256 * 8 * (64 * 64 + 2 * 64) * 4      # 256 workgroups x 8 GEMMs: block + bias pairs
    w = mlp_geom._GeomParams()
    fake = 0x1000
    w.W0 = w.b0 = fake
    w.R1 = w.rb1 = w.R2 = w.rb2 = fake               # the rotation head alone
    assert L.s3g_deform_geom_forward(C.byref(w), 0, None, None, fake, None, None, 0, None) == 0        # P == 0: nothing to do
    assert L.s3g_deform_geom_backward(C.byref(w), 0, None, None, None, fake, None, None, C.byref(w), None, None) == 0
    assert L.s3g_deform_geom_forward(C.byref(w), 0, None, None, None, None, None, 0, None) == 1          # no head asked for
    assert b"s3g_deform_geom_forward" in L.s3g_last_error()
    assert L.s3g_deform_geom_forward(C.byref(w), 0, None, fake, fake, None, None, 0, None) == 1          # ds asked for, C1..cb2 NULL
    assert L.s3g_deform_geom_forward(C.byref(w), -1, None, None, fake, None, None, 0, None) == 1
    assert L.s3g_deform_geom_forward(C.byref(w), 5, None, None, fake, None, None, 0, None) == 1          # P > 0 without features / stash
    assert L.s3g_deform_geom_backward(C.byref(w), 0, None, None, fake, None, None, None, C.byref(w), None, None) == 1   # g_ds without slots
    assert b"s3g_deform_geom_backward" in L.s3g_last_error()
    assert L.s3g_deform_geom_backward(C.byref(w), 0, None, None, None, fake, None, None, None, None, None) == 1         # gw NULL


def test_geometry_heads_refuses_cpu_tensors_and_an_empty_head_set():
    from s3gaussian_amd.mlp_geom import geometry_heads
    net = _net(no_ds=False, no_dr=False, no_do=False)
    x = torch.zeros(4, 128)
    with pytest.raises(RuntimeError, match="geometry heads: features must live on the GPU"):
        geometry_heads(x, net.feature_out, net.scales_deform, net.rotations_deform, net.opacity_deform)
    with pytest.raises(ValueError, match="at least one"):
        geometry_heads(x, net.feature_out, None, None, None)
