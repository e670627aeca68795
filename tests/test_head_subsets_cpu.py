"""Networks without the SH head or the feature head on the fused route, the part that needs no GPU: the truth table of the three
route predicates of `Deformation` over all 64 on/off combinations of the six heads, and the refusals of the C entry points that come
before anything is launched."""
import ctypes as C
import itertools

import pytest
import torch

SMALL = dict(grid_dimensions=2, input_coordinate_dim=4, output_coordinate_dim=32, resolution=[8, 8, 8, 5])
SWITCHES = ("no_dx", "no_ds", "no_dr", "no_do", "no_dshs", "feat_head")


def _net(**over):
    from s3gaussian_amd.deformation import deform_network
    from s3gaussian_amd.pipeline import default_hyper
    return deform_network(default_hyper(kplanes_config=SMALL, **over)).deformation_net


def test_the_three_predicates_over_all_64_head_combinations():
    seen = {"ok": 0, "geometry": 0, "heads": 0, "none": 0}
    for values in itertools.product((False, True), repeat=6):
        over = dict(zip(SWITCHES, values))
        net = _net(**over)
        geometry_off = over["no_ds"] and over["no_dr"] and over["no_do"]
        full_chain = not over["no_dshs"] and over["feat_head"]
        any_head = not (over["no_dx"] and geometry_off and over["no_dshs"]) or over["feat_head"]
        want = (full_chain and geometry_off, full_chain and not geometry_off, not full_chain and any_head)
        got = (net._fused_ok(), net._fused_geometry_ok(), net._fused_heads_ok())
        assert got == want, over
        assert sum(got) <= 1 and net._fused_any() == any(got), over
        assert net._fused_geometry_on() == (any(got) and not geometry_off), over
        assert hasattr(net, "dino_head") == over["feat_head"]
        seen["ok" if got[0] else "geometry" if got[1] else "heads" if got[2] else "none"] += 1
    # full chain: 2 (no_dx) x 8 geometry subsets; the other 48 lack the SH or the feature head, one of them has no head at all
    assert seen == {"ok": 2, "geometry": 14, "heads": 47, "none": 1}


@pytest.mark.parametrize("over", [dict(static_mlp=True), dict(empty_voxel=True), dict(grid_pe=2), dict(no_grid=True), dict(net_width=128),
                                  dict(defor_depth=2)])
@pytest.mark.parametrize("heads", [dict(feat_head=False), dict(no_dshs=True), dict(no_dshs=True, feat_head=False, no_ds=False, no_dr=False)])
def test_the_masked_and_embedded_family_stays_on_the_library_route(over, heads):
    net = _net(**over, **heads)
    assert not net._fused_heads_ok() and not net._fused_ok() and not net._fused_geometry_ok() and not net._fused_any()


def test_flow_guard_admits_every_fused_configuration_with_a_position_head():
    from types import SimpleNamespace
    from s3gaussian_amd import pipeline
    stub = lambda net: SimpleNamespace(get_xyz=SimpleNamespace(is_cuda=True, device=torch.device("cpu")), max_sh_degree=3,
                                       _deformation=SimpleNamespace(deformation_net=net))
    pipe = SimpleNamespace(convert_SHs_python=True)
    for heads in (dict(feat_head=False), dict(no_dshs=True), dict(no_dshs=True, feat_head=False, no_ds=False, no_dr=False)):
        assert pipeline._fused_route(stub(_net(**heads)), pipe)
        static = stub(_net(no_dx=True, **heads))
        assert not pipeline._fused_route(static, pipe)
        assert "no_dx" in pipeline._fused_route_missing(static, pipe)
        assert "grid_pe" in pipeline._fused_route_missing(stub(_net(grid_pe=2, **heads)), pipe)


def test_deform_mlp_refuses_cpu_tensors_for_the_new_head_sets():
    from s3gaussian_amd.mlp import deform_mlp
    net = _net(feat_head=False)
    x = torch.zeros(4, 128)
    with pytest.raises(RuntimeError, match="features must live on the GPU"):
        deform_mlp(x, net.feature_out, net.pos_deform, net.shs_deform, None)
    with pytest.raises(RuntimeError, match="features must live on the GPU"):
        deform_mlp(x, net.feature_out, net.pos_deform, net.shs_deform, None, need_dshs=False)
    with torch.no_grad():      # nothing to compute: no launch, whatever the device
        assert deform_mlp(x, net.feature_out, net.pos_deform, net.shs_deform, None, need_dx=False, need_dshs=False) == (None, None, None)


def test_refusals_before_any_device_call():
    """Host code only: S3G_ERR_INVALID_ARG (1) with the library's error text for a call without any head, for a gradient slot that a
    live head needs and does not get, and S3G_OK for P == 0.  The pointers are made-up addresses that are never dereferenced."""
    from s3gaussian_amd import _lib, mlp
    L = mlp._bind()
    L.s3g_last_error.restype = C.c_char_p
    assert L.s3g_abi_version() == _lib.ABI_VERSION == 16
    fake = 0x1000
    w = mlp._Params()
    for n in mlp._NAMES:
        setattr(w, n, fake)
    fwd, bwd, bwd_o = L.s3g_deform_mlp_forward, L.s3g_deform_mlp_backward, L.s3g_deform_mlp_backward_ordered
    # forward: P == 0 returns at once, whatever the outputs; all-NULL outputs are refused; save_activations with feat == NULL is not
    assert fwd(C.byref(w), 0, None, None, None, None, None, 0, None) == 0
    assert fwd(C.byref(w), 0, None, fake, None, None, None, 1, None) == 0
    assert fwd(C.byref(w), 5, fake, None, None, None, fake, 0, None) == 1
    assert b"s3g_deform_mlp_forward" in L.s3g_last_error() and b"all NULL" in L.s3g_last_error()
    assert fwd(C.byref(w), 5, fake, None, None, None, fake, 1, None) == 1
    assert fwd(C.byref(w), -1, fake, fake, None, None, fake, 0, None) == 1
    assert fwd(C.byref(w), 5, None, fake, None, None, fake, 0, None) == 1          # P > 0 without features
    assert fwd(C.byref(w), 5, fake, fake, None, None, None, 0, None) == 1          # ... without a stash
    assert fwd(None, 5, fake, fake, None, None, fake, 0, None) == 1
    # backward: the same for the three upstream gradients
    gw = mlp._Params()
    for n in mlp._NAMES:
        setattr(gw, n, fake)
    assert bwd(C.byref(w), 0, None, None, None, None, None, None, C.byref(gw), None, None) == 0
    assert bwd_o(C.byref(w), 0, None, None, None, None, None, None, C.byref(gw), None, None, None) == 0
    assert bwd(C.byref(w), 5, fake, fake, None, None, None, fake, C.byref(gw), fake, None) == 1
    assert b"s3g_deform_mlp_backward" in L.s3g_last_error() and b"all NULL" in L.s3g_last_error()
    assert bwd_o(C.byref(w), 5, fake, fake, None, None, None, fake, C.byref(gw), fake, fake, None) == 1
    assert bwd(C.byref(w), 5, fake, fake, fake, None, None, fake, None, fake, None) == 1                 # gw NULL
    # gw slots: a head with an upstream gradient needs all of its slots, feature_out always does; an absent head's may be NULL
    for g_index, names in ((0, ("P1", "pb1", "P2", "pb2")), (1, ("S1", "sb1", "S2", "sb2")), (2, ("D0", "db0", "D1", "db1", "D2", "db2"))):
        gs = [fake if k == g_index else None for k in range(3)]
        for missing in names + ("W0", "b0"):
            setattr(gw, missing, None)
            assert bwd(C.byref(w), 5, fake, fake, *gs, fake, C.byref(gw), fake, None) == 1, missing
            assert b"gw" in L.s3g_last_error()
            assert bwd_o(C.byref(w), 5, fake, fake, *gs, fake, C.byref(gw), fake, fake, None) == 1, missing
            setattr(gw, missing, fake)
    assert bwd_o(C.byref(w), 5, fake, fake, fake, None, None, fake, C.byref(gw), fake, None, None) == 1   # ordered flush without its scratch
