"""CPU-only: the host side of the sky colour model's device route (include/s3g_skymodel.h).  The exports exist, the one function
that decides every extent (s3g_skymodel_plan) agrees with a restatement of its formula, the public functions refuse CPU tensors by
name, GaussianParams.attach_sky_model adds the "sky_model" param group, and a state dict round-trips."""
from types import SimpleNamespace

import pytest
import torch

N_PARAMS = 83715
CHUNK = 256
DEFAULT_BAND = 16384


def _align(n):
    return (n + 127) // 128 * 128


def _plan_restated(n, band_pixels, T):
    """What include/s3g_skymodel.h says s3g_skymodel_plan decides."""
    tiles = -(-n // T)
    band = band_pixels if band_pixels > 0 else DEFAULT_BAND
    band = min(-(-band // T) * T, tiles * T)
    chunks = -(-band // CHUNK)
    # the band's scratch rows [h0, e, 0] (320), h1, dz1, dz0 (256 each), dz2 (32); the chunks' weight partials and double bias
    # partials; the double accumulator; every piece starts on a 128-byte boundary
    pieces = [band * 320 * 4, band * 256 * 4, band * 256 * 4, band * 256 * 4, band * 32 * 4, chunks * N_PARAMS * 4,
              chunks * 515 * 8, N_PARAMS * 8]
    off = 0
    for p in pieces:
        off = _align(off) + p
    return dict(tile_pixels=T, tiles=tiles, band_pixels=band, bands=-(-n // band), chunks=chunks, workspace_bytes=_align(off))


def test_the_new_exports_exist():
    from s3gaussian_amd import _lib
    L = _lib.lib()
    for name in ("s3g_skymodel_tile_pixels", "s3g_skymodel_plan", "s3g_skymodel_pack_bytes", "s3g_sky_pack", "s3g_sky_forward",
                 "s3g_sky_backward"):
        assert hasattr(L, name) and name in _lib.EXPORTED_SYMBOLS, name
    T = L.s3g_skymodel_tile_pixels()
    assert T > 0 and T % 32 == 0
    assert L.s3g_skymodel_pack_bytes() >= N_PARAMS * 4 and L.s3g_skymodel_pack_bytes() % 4 == 0


def test_plan_agrees_with_its_formula():
    from s3gaussian_amd import _lib, skymodel
    T = _lib.lib().s3g_skymodel_tile_pixels()
    for n in (1, T - 1, T, T + 1, 1961, 1066 * 1600):
        for band in (None, 0, 1, T, T + 1, 512, 1000, 1 << 20):
            e = skymodel.plan(n, band)
            got = {k: getattr(e, k) for k in ("tile_pixels", "tiles", "band_pixels", "bands", "chunks", "workspace_bytes")}
            assert got == _plan_restated(n, band or 0, T), (n, band, got)
            assert e.band_pixels % T == 0 and e.bands * e.band_pixels >= n > (e.bands - 1) * e.band_pixels
    assert skymodel.plan(1961, 512).bands == 4 and skymodel.plan(1961, 512).band_pixels == 512       # three full bands and 425 pixels
    for bad in (0, -5, 1 << 31):
        with pytest.raises(Exception, match="s3g_skymodel_plan"):
            skymodel.plan(bad)


def test_launchers_refuse_bad_arguments_before_any_device_call():
    from s3gaussian_amd import _lib
    L = _lib.lib()
    cam = _lib.SkyCamera()
    assert L.s3g_sky_forward(0, 4, cam, None, None, None, None, None) == 1 and b"s3g_sky_forward" in L.s3g_last_error()
    assert L.s3g_sky_forward(4, 4, cam, None, None, None, None, None) == 1
    assert L.s3g_sky_backward(4, 4, cam, None, None, None, 0, None, None, None, None) == 1 and b"s3g_sky_backward" in L.s3g_last_error()
    assert L.s3g_sky_pack(None, None, None, None, None, None, None, None) == 1 and b"s3g_sky_pack" in L.s3g_last_error()


def test_sky_image_and_composite_refuse_cpu_tensors_by_name():
    from s3gaussian_amd import skymodel
    m = skymodel.SkyModel()
    cam = (torch.eye(3), 20.0, 20.0, 12.0, 8.0)
    with pytest.raises(RuntimeError, match="the sky model must live on the GPU"):
        skymodel.sky_image(m, cam, H=16, W=24)
    with pytest.raises(RuntimeError, match="render must live on the GPU"):
        skymodel.sky_composite(m, cam, torch.zeros(3, 16, 24), None)


def _cpu_model(P=50):
    from s3gaussian_amd.pipeline import GaussianParams, default_hyper, default_opt
    torch.manual_seed(0)
    pc = GaussianParams(3, default_hyper(kplanes_config=dict(grid_dimensions=2, input_coordinate_dim=4, output_coordinate_dim=32,
                                                             resolution=[8, 8, 8, 5])))
    pc.init_from_tensors(torch.rand(P, 3), torch.rand(P, 3), torch.rand(P, 4), torch.rand(P, 1), torch.rand(P, 16, 3), torch.device("cpu"))
    return pc, default_opt()


def test_attach_sky_model_adds_the_group():
    from s3gaussian_amd import skymodel
    pc, opt = _cpu_model()
    m = skymodel.SkyModel()
    with pytest.raises(RuntimeError, match="training_setup"):
        pc.attach_sky_model(m)
    pc.training_setup(opt)
    keys = set(pc.state_dict())
    n_groups = len(pc.optimizer.param_groups)
    assert skymodel.attached_group(pc.optimizer, m) is None
    assert pc.attach_sky_model(m) is m
    g = pc.optimizer.param_groups[-1]
    assert len(pc.optimizer.param_groups) == n_groups + 1 and g["name"] == "sky_model" and g["lr"] == 0.0025
    assert [id(p) for p in g["params"]] == [id(p) for p in m.tensors()] and len(g["params"]) == 6
    assert skymodel.attached_group(pc.optimizer, m) is g and skymodel.attached_group(pc.optimizer, skymodel.SkyModel()) is None
    assert set(pc.state_dict()) == keys                          # not a submodule: the Gaussians' checkpoints keep their keys
    with pytest.raises(RuntimeError, match="already"):
        pc.attach_sky_model(skymodel.SkyModel())
    pc2, opt2 = _cpu_model()
    pc2.training_setup(opt2)
    pc2.attach_sky_model(skymodel.SkyModel(), lr=0.01)
    assert pc2.optimizer.param_groups[-1]["lr"] == 0.01


def test_unattached_models_and_bad_combinations_are_refused_by_name():
    from s3gaussian_amd import skymodel
    from s3gaussian_amd.pipeline import default_hyper, evaluate, render, training_step
    pc, opt = _cpu_model()
    pc.training_setup(opt)
    m = skymodel.SkyModel()
    pipe = SimpleNamespace(convert_SHs_python=True, compute_cov3D_python=False, debug=False)
    with pytest.raises(RuntimeError, match="not attached"):
        training_step(pc, {}, None, None, None, default_hyper(), opt, torch.zeros(3), sky_model=m)
    with pytest.raises(RuntimeError, match=r"render\(sky_model=..., pose=...\)"):
        render({}, pc, pipe, torch.zeros(3), sky_model=m, pose=object(), cam_index=0)
    with pytest.raises(RuntimeError, match=r"render\(sky_model=..., override_color=...\)"):
        render({}, pc, pipe, torch.zeros(3), sky_model=m, override_color=torch.zeros(50, 3))
    with pytest.raises(RuntimeError, match=r"evaluate\(sky_model=..., pose=...\)"):
        evaluate(pc, [], [], pipe, torch.zeros(3), sky_model=m, pose=object())


def test_a_state_dict_round_trips():
    from s3gaussian_amd import skymodel
    torch.manual_seed(3)
    a = skymodel.SkyModel()
    sd = a.state_dict()
    assert sum(v.numel() for k, v in sd.items() if "scales" not in k) == skymodel.N_PARAMS == N_PARAMS
    b = skymodel.SkyModel.from_state_dict({"sky_model." + k: v.clone() for k, v in sd.items()})
    for x, y in zip(a.tensors(), b.tensors()):
        assert torch.equal(x, y) and x.data_ptr() != y.data_ptr()
    assert [tuple(t.shape) for t in b.tensors()] == [(256, 33), (256,), (256, 289), (256,), (3, 256), (3,)]
