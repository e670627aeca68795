"""The blend backward's per-wave visit bounds (include/s3g_raster.h: s3g_raster_set_backward_wave_bounds) change no output bit.

With the bounds on, each wave of 64 pixels starts its walk at the deepest contributor of its own pixels instead of the tile's;
s3g_raster_set_backward_wave_bounds(0) restores the tile-wide schedule.  Images, depths, radii and every gradient must be equal
(torch.equal, not a tolerance) for the single-image and the two-image pass, with the host-asynchronous and the synchronous
forward, on the headline street scene, on the same scene with 3.5x scales, on an image whose sides are not multiples of 16 and on
a scene built so that the waves of one tile stop at very different depths."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def _set_wave_bounds(on: bool) -> bool:
    from s3gaussian_amd import _lib
    L = _lib.lib()
    L.s3g_raster_set_backward_wave_bounds.restype = ctypes.c_int
    L.s3g_raster_set_backward_wave_bounds.argtypes = [ctypes.c_int]
    return bool(L.s3g_raster_set_backward_wave_bounds(int(on)))


def _street(P, W, H, scale_mult, dev, seed=0):
    from s3gaussian_amd import synth
    sc = synth.street_scene(P=P, seed=seed, width=W, height=H, n_frames=1)
    gs = sc["gaussians"]
    g = torch.Generator().manual_seed(seed + 1)
    tensors = dict(means3D=gs["xyz"], scales=torch.exp(gs["log_scales"]) * scale_mult,
                   rotations=torch.nn.functional.normalize(gs["rotations_raw"], dim=1), opacities=torch.sigmoid(gs["opacity_logit"]),
                   colors_a=torch.rand(P, 3, generator=g), colors_b=torch.rand(P, 3, generator=g))
    return {k: v.float().contiguous().to(dev) for k, v in tensors.items()}, sc["cameras"][0], sc["bg"]


def _wall(dev, W=96, H=80, P=4000, seed=0):
    """Random Gaussians behind a few large, nearly opaque ones whose lower edge crosses the image in the middle of a tile row:
    pixels above the edge saturate after a handful of entries, pixels below walk the whole list."""
    from s3gaussian_amd import synth
    import numpy as np
    g = torch.Generator().manual_seed(seed)
    fov = math.radians(60)
    cam = synth.make_camera(np.eye(3), np.zeros(3), fov, 2 * math.atan(math.tan(fov / 2) * H / W), W, H)
    xyz = torch.rand(P, 3, generator=g) * 2 - 1
    xyz[:, :2] *= 2.2
    xyz[:, 2] = 4.0 + 2.0 * torch.rand(P, generator=g)
    scales = torch.exp(math.log(0.12) + 0.4 * torch.randn(P, 3, generator=g))
    op = torch.sigmoid(1.5 * torch.randn(P, 1, generator=g))
    wall = torch.tensor([[x, -1.2, 2.0] for x in (-1.2, -0.4, 0.4, 1.2) for _ in range(3)])   # y < 0: upper half of the image
    xyz = torch.cat([wall, xyz])
    scales = torch.cat([torch.tensor([[0.5, 0.6, 0.05]]).repeat(len(wall), 1), scales])
    op = torch.cat([torch.full((len(wall), 1), 0.995), op])
    n = xyz.shape[0]
    q = torch.randn(n, 4, generator=g)
    q[:len(wall)] = torch.tensor([1.0, 0.0, 0.0, 0.0])
    tensors = dict(means3D=xyz, scales=scales, rotations=torch.nn.functional.normalize(q, dim=1), opacities=op,
                   colors_a=torch.rand(n, 3, generator=g), colors_b=torch.rand(n, 3, generator=g))
    return {k: v.float().contiguous().to(dev) for k, v in tensors.items()}, cam, torch.tensor([0.2, 0.5, 0.7])


def _run(t, cam, bg, dev, pair):
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    rs = GaussianRasterizationSettings(
        image_height=cam["image_height"], image_width=cam["image_width"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
        bg=bg.to(dev), scale_modifier=1.0, viewmatrix=cam["viewmatrix"].to(dev), projmatrix=cam["projmatrix"].to(dev),
        sh_degree=0, campos=cam["campos"].to(dev), prefiltered=False, debug=False)
    rast = GaussianRasterizer(raster_settings=rs)
    leaf = {k: v.clone().requires_grad_(True) for k, v in t.items()}
    m2 = torch.zeros_like(leaf["means3D"], requires_grad=True)
    H, W = cam["image_height"], cam["image_width"]
    g = torch.Generator(device=dev).manual_seed(7)
    if pair:
        a, radii, depth, b = rast.forward_pair(leaf["means3D"], m2, leaf["opacities"], leaf["colors_a"], leaf["colors_b"],
                                               scales=leaf["scales"], rotations=leaf["rotations"])
        outs = [a, depth, b]
    else:
        a, radii, depth = rast(means3D=leaf["means3D"], means2D=m2, opacities=leaf["opacities"], colors_precomp=leaf["colors_a"],
                               scales=leaf["scales"], rotations=leaf["rotations"])
        outs = [a, depth]
    loss = sum((o * torch.randn(o.shape, generator=g, device=dev)).sum() for o in outs)
    loss.backward()
    res = [o.detach() for o in outs] + [radii, m2.grad]
    res += [leaf[k].grad for k in ("means3D", "scales", "rotations", "opacities", "colors_a")]
    if pair:
        res.append(leaf["colors_b"].grad)
    torch.cuda.synchronize()
    return res


def _compare(t, cam, bg, dev):
    from s3gaussian_amd import raster_C
    prev_async = raster_C.set_async(True)
    prev_bounds = _set_wave_bounds(True)
    try:
        for asynchronous in (True, False):
            raster_C.set_async(asynchronous)
            for pair in (False, True):
                _set_wave_bounds(False)
                want = _run(t, cam, bg, dev, pair)
                _set_wave_bounds(True)
                got = _run(t, cam, bg, dev, pair)
                assert float(want[0].abs().sum()) > 0
                for i, (x, y) in enumerate(zip(got, want)):
                    assert torch.equal(x, y), (asynchronous, pair, i)
    finally:
        _set_wave_bounds(prev_bounds)
        raster_C.set_async(prev_async)


def test_headline_street_scene(gpu_device):
    _compare(*_street(1_200_000, 1600, 1066, 1.0, gpu_device), gpu_device)


def test_street_scene_with_scales_x3_5(gpu_device):
    _compare(*_street(1_200_000, 1600, 1066, 3.5, gpu_device), gpu_device)


def test_image_sides_not_multiples_of_16(gpu_device):
    _compare(*_street(300_000, 1000, 613, 1.0, gpu_device), gpu_device)


def test_waves_of_a_tile_stop_at_different_depths(gpu_device):
    _compare(*_wall(gpu_device), gpu_device)
