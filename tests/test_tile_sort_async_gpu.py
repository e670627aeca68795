"""The per-tile sort under the ASYNCHRONOUS forward's contract (include/s3g_raster.h::s3g_raster_forward_async), cell by cell: the
caller's estimate of the longest list (sort_lds_keys, long_lists) against the length the one tile of the scene really has, on both
sides of every switch of csrc/raster_sort.hip::tile_sort_plan.  The estimate sizes buffers and nothing else: whatever it says, a render
whose lists the counting kernel lets through (n <= 4096, or long_lists != 0) is the synchronous render bit for bit -- ranges, sorted
list, instance -> position map, colour, depth -- and one it does not let through is the documented no-op.  tests/test_tile_sort_gpu.py
holds the synchronous forward, where the longest list is read back exactly; tests/test_sort_plan_cpu.py walks the same plan on the host.

The entry point is called directly, with arenas of this file's own: the binning arena is ZEROED first, so a list that no launch
sorted reads as n times Gaussian 0 -- in bounds, and not the expected list -- instead of whatever the allocator handed back (which,
after the synchronous render of the same scene, may well be the right answer)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.util import tiny_scene

pytestmark = pytest.mark.gpu
SIZES = [1, 256, 257, 512, 513, 600, 1025, 3000, 4096, 4097, 7700, 16385]
CAPACITY = 1 << 15          # instances and slots the arenas of the asynchronous calls hold: above every size here
SMALL_KEYS = 4096           # longest list an asynchronous forward without long_lists accepts
W = H = 16

_references = {}


def _scene(n, ties):
    s = tiny_scene(P=n, W=W, H=H, seed=n % 97 + 3, scale=0.004, sigma=0.1, spread=0.05)     # all in the middle of the one tile
    s["opacities"] = s["opacities"] * 0.01 + 0.005
    if ties == "one_depth":
        s["means3D"][:, 2] = 5.0
    return s


def _reference(n, ties, dev):
    """The synchronous render of the one-tile scene of n instances, computed once per scene and shared (read-only): device inputs and
    CPU copies of everything the asynchronous cells are compared with.  Its list is pinned against the (depth bits, index) order."""
    key = (n, ties)
    if key in _references:
        return _references[key]
    from diff_gaussian_rasterization import _C
    from s3gaussian_amd import _debug
    s = _scene(n, ties)
    cam = s["cam"]
    e = torch.Tensor([])
    t = {k: s[k].to(dev).contiguous() for k in ("means3D", "colors_precomp", "opacities", "scales", "rotations", "bg")}
    t.update(view=cam["viewmatrix"].to(dev).contiguous(), proj=cam["projmatrix"].to(dev).contiguous(), campos=cam["campos"].to(dev).contiguous())
    R, color, depth, radii, geom, binning, img = _C.rasterize_gaussians(
        t["bg"], t["means3D"], t["colors_precomp"], t["opacities"], t["scales"], t["rotations"], 1.0, e, t["view"], t["proj"],
        cam["tanfovx"], cam["tanfovy"], H, W, e, 0, t["campos"], False, False)
    g, im, b = _debug.decode_geometry(geom, n), _debug.decode_image(img, W, H), _debug.decode_binning(binning, R)
    radii_np, depths = radii.cpu().numpy(), g["depths"].cpu().numpy()
    ranges, pl = im["ranges"].cpu().numpy(), b["point_list"].cpu().numpy().astype(np.int64)
    vis = np.nonzero(radii_np > 0)[0]
    assert R == vis.size == n and ranges.shape[0] == 1 and tuple(ranges[0]) == (0, n)
    bits = depths.view(np.uint32).astype(np.uint64)[vis]
    expected = vis[np.argsort((bits << np.uint64(32)) | vis.astype(np.uint64), kind="stable")]
    np.testing.assert_array_equal(pl[:n], expected)
    if ties == "one_depth":
        np.testing.assert_array_equal(pl[:n], np.arange(n))              # the index alone decides
    slots = int(im["ctrl"][3].item())
    assert slots == n                                                    # one tile: every rect is that tile
    slot_pos = b["slot_pos"][:slots].cpu().numpy()
    assert sorted(slot_pos.tolist()) == list(range(n))                   # a permutation: every instance has its position
    ref = dict(scene=s, dev=t, color=color.cpu(), depth=depth.cpu(), radii=radii.cpu(), ranges=ranges, point_list=pl[:n].copy(),
               slot_pos=slot_pos)
    _references[key] = ref
    return ref


def _forward_async(ref, n, dev, sort_lds_keys, long_lists, forward_only):
    """One s3g_raster_forward_async call the way raster_C._forward_async issues it (arenas from s3g_raster_arena_bytes, a pinned status
    row, a device status word) -> everything it left behind, on the CPU."""
    from s3gaussian_amd import _debug, _lib, raster_C
    L = _lib.lib()
    t, cam = ref["dev"], ref["scene"]["cam"]
    nb = (C.c_size_t(), C.c_size_t(), C.c_size_t())
    _lib.check(L.s3g_raster_arena_bytes(n, W, H, CAPACITY, CAPACITY, C.byref(nb[0]), C.byref(nb[1]), C.byref(nb[2])))
    geom, img = (torch.empty(int(x.value), dtype=torch.uint8, device=dev) for x in (nb[0], nb[2]))
    binning = torch.zeros(int(nb[1].value), dtype=torch.uint8, device=dev)
    status_dev = torch.full((1,), 0x55, dtype=torch.int32, device=dev)
    status_host = torch.full((8,), -1, dtype=torch.int32).pin_memory()
    color = torch.full((3, H, W), -1.0, device=dev)
    depth = torch.full((1, H, W), -1.0, device=dev)
    radii = torch.full((n,), -1, dtype=torch.int32, device=dev)
    inp = raster_C._inputs(n, 0, 0, W, H, t["bg"], t["means3D"], None, t["colors_precomp"], t["opacities"], t["scales"], 1.0,
                           t["rotations"], None, t["view"], t["proj"], cam["tanfovx"], cam["tanfovy"], t["campos"], False, False)
    desc = _lib.RasterAsync(CAPACITY, CAPACITY, sort_lds_keys, long_lists, geom.data_ptr(), binning.data_ptr(), img.data_ptr(),
                            status_dev.data_ptr(), status_host.data_ptr(), forward_only, None, None)
    with torch.cuda.device(dev):
        _lib.check(L.s3g_raster_forward_async(C.byref(inp), None, C.byref(desc), color.data_ptr(), depth.data_ptr(), None,
                                              radii.data_ptr(), _lib.stream_ptr()))
        torch.cuda.synchronize()
    b = _debug.decode_binning(binning, CAPACITY)
    return dict(row=[x & 0xffffffff for x in status_host.tolist()], word=int(status_dev.item()), color=color.cpu(), depth=depth.cpu(),
                radii=radii.cpu(), ranges=_debug.decode_image(img, W, H)["ranges"].cpu().numpy(),
                point_list=b["point_list"][:n].cpu().numpy().astype(np.int64), slot_pos=b["slot_pos"][:n].cpu().numpy())


def _check_cell(ref, n, dev, sort_lds_keys, long_lists, forward_only):
    cell = f"sort_lds_keys={sort_lds_keys} long_lists={long_lists} forward_only={forward_only} n={n}"
    out = _forward_async(ref, n, dev, sort_lds_keys, long_lists, forward_only)
    row = out["row"]
    assert torch.equal(out["radii"], ref["radii"]), cell          # the per-Gaussian geometry does not depend on any of this
    assert row[2] == 0 and row[7] == 0, (cell, row)
    if n <= SMALL_KEYS or long_lists:
        assert out["word"] == 0 and row[4] == 0 and row[0] == row[5] == n and row[1] == n and row[3] == row[6] == n, (cell, row)
        np.testing.assert_array_equal(out["ranges"], ref["ranges"], err_msg=cell)
        np.testing.assert_array_equal(out["point_list"], ref["point_list"], err_msg=cell)
        assert torch.equal(out["color"], ref["color"]) and torch.equal(out["depth"], ref["depth"]), cell
        if not forward_only:
            np.testing.assert_array_equal(out["slot_pos"], ref["slot_pos"], err_msg=cell)
    else:           # a list of more than 4096 instances and no long-list pass: the documented no-op
        assert out["word"] & 1 and row[4] == 1 and row[0] == 0 and row[5] == n and row[1] == n, (cell, row)
        assert not out["ranges"].any(), cell
        bg = ref["scene"]["bg"]
        assert torch.equal(out["color"], bg[:, None, None].expand(3, H, W)) and not out["depth"].any(), cell


@pytest.mark.parametrize("long_lists", [0, 1])
@pytest.mark.parametrize("sort_lds_keys", [0, 256, 512, 1024, 4096])
def test_every_estimate_renders_every_list_length_like_the_synchronous_forward(gpu_device, sort_lds_keys, long_lists):
    for n in SIZES:
        ref = _reference(n, "none", gpu_device)
        for forward_only in (0, 1):
            _check_cell(ref, n, gpu_device, sort_lds_keys, long_lists, forward_only)


@pytest.mark.parametrize("long_lists", [0, 1])
def test_a_tie_of_the_whole_list_is_sorted_by_index_beyond_the_estimate(gpu_device, long_lists):
    """Every instance at ONE depth: the keys differ in the index alone, and the lists are past an estimate of 256 keys."""
    for n in (600, 3000):
        _check_cell(_reference(n, "one_depth", gpu_device), n, gpu_device, 256, long_lists, 0)
