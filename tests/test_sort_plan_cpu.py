"""CPU-only: the launch plan of the per-tile sort (csrc/raster_sort.hip::tile_sort_plan, the host function launch_tile_sort issues its
launches from), read through the testing hook s3g_raster_sort_plan and walked list length by list length.

The synchronous forward knows the longest list exactly; the asynchronous one (s3g_raster_forward_async) is handed an ESTIMATE
(sort_lds_keys, long_lists) learnt from earlier renders, which the lists of the render at hand need not respect: another camera of the
same size, a densification, one crowded tile.  Whatever the estimate says, a list the counting kernel lets through has to be inside
exactly one launch -- a list no launch takes is never written to point_list, and the blend then reads uninitialised words as
Gaussian indices -- and a launch's LDS carve-up has to fit the dynamic LDS it asks for.  tests/test_tile_sort_async_gpu.py holds the
same matrix on the device."""
import ctypes as C

import pytest

from tests.test_abi_cpu import _struct_fields

N_MAX = 20_011
SYNC_MODES = [(0, k, 0) for k in (1, 256, 512, 513, 4096, 4097, 16384, 20011)]
ASYNC_MODES = [(1, k, ll) for k in (0, 1, 255, 256, 257, 512, 513, 1024, 2048, 4096, 8192) for ll in (0, 1)]
ANY = 0xffffffff


def _plan(asynchronous, keys, long_lists):
    from s3gaussian_amd import _lib
    p = _lib.SortPlan()
    assert _lib.lib().s3g_raster_sort_plan(asynchronous, keys, long_lists, C.byref(p)) == 0
    launches = [tuple(getattr(p.launch[i], f) for f, _ in _lib.SortLaunch._fields_) for i in range(p.launches)]
    return p, launches          # launch = (threads, lds_bytes, lo, hi, lds_keys, bucket_keys)


def test_plan_structs_match_the_header():
    from s3gaussian_amd import _lib
    assert _struct_fields("s3g_raster.h", "s3g_sort_launch") == [f[0] for f in _lib.SortLaunch._fields_]
    assert _struct_fields("s3g_raster.h", "s3g_sort_plan") == [f[0] for f in _lib.SortPlan._fields_]
    assert C.sizeof(_lib.SortLaunch) == 24 and C.sizeof(_lib.SortPlan) == 4 + 3 * 24 + 6 * 4
    assert _lib.lib().s3g_raster_sort_plan(1, 256, 0, None) == 1 and b"NULL plan" in _lib.lib().s3g_last_error()


def test_the_constants_are_the_documented_ones():
    p, _ = _plan(1, 0, 0)
    assert (p.bucket_min, p.small_keys, p.rank_direct, p.max_lds_bytes) == (512, 4096, 256, 128 * 1024)
    assert p.bucket_lds_extra == 2048 * 4 + 256 * 2 * 2           # cursors of the bucket pass + its two bucket lists
    # what the counting kernel is told: nothing (synchronous), 4096 without the long-list pass, no limit with it
    assert _plan(0, 300, 0)[0].count_cap_tile == 0
    assert _plan(1, 300, 0)[0].count_cap_tile == p.small_keys and _plan(1, 300, 1)[0].count_cap_tile == ANY


@pytest.mark.parametrize("asynchronous,keys,long_lists", SYNC_MODES + ASYNC_MODES)
def test_every_list_length_is_sorted_exactly_once_in_a_buffer_that_holds_it(asynchronous, keys, long_lists):
    p, launches = _plan(asynchronous, keys, long_lists)
    assert 1 <= len(launches) <= 3
    uncovered, twice, unfit, stray = [], [], [], []
    for n in range(1, N_MAX + 1):
        if not asynchronous and n > keys:
            break                                    # the synchronous forward read `keys` back: no list is longer
        cover = [l for l in launches if l[2] < n <= l[3]]
        if asynchronous and not long_lists and n > p.small_keys:
            if cover:                                # such a render is the documented no-op: every list is empty
                stray.append(n)
            continue
        if len(cover) != 1:
            (uncovered if not cover else twice).append(n)
            continue
        threads, lds_bytes, lo, hi, lds_keys, bucket_keys = cover[0]
        ok = lds_keys * 8 <= lds_bytes <= p.max_lds_bytes and threads % 64 == 0 and 64 <= threads <= 1024
        if bucket_keys:
            ok = ok and 2 * bucket_keys * 8 + p.bucket_lds_extra <= lds_bytes
        # the branch sort_tiles_kernel takes for this n (in its order): bucket pass, rank by counting, network in LDS, network in global
        if n > p.bucket_min and n <= bucket_keys:
            ok = ok and threads >= 256              # the scan of the bucket pass is done by threads 0 .. 255
        elif n <= p.rank_direct and n <= lds_keys:
            ok = ok and threads >= p.rank_direct    # one thread per key; with fewer the kernel falls to the network: a silent slowdown
        if not ok:
            unfit.append(n)
    span = lambda v: f"{len(v)} lengths, {v[0]} .. {v[-1]}" if v else "none"
    assert not uncovered and not twice and not unfit and not stray, (
        f"mode (async={asynchronous}, keys={keys}, long_lists={long_lists}) plan {launches}: in no launch: {span(uncovered)}; "
        f"in more than one: {span(twice)}; buffer too small: {span(unfit)}; beyond what the counting kernel lets through: {span(stray)}")
    if asynchronous:
        # the counting kernel empties every list iff one exceeds count_cap_tile: the plan ends exactly there, one number in both places
        assert max(hi for _, _, _, hi, _, _ in launches) == p.count_cap_tile == (ANY if long_lists else p.small_keys)


def test_steady_state_plans_are_the_recorded_ones():
    """The plans whose estimate holds cost what they cost before the plan became a function: launch count, workgroup size, dynamic
    LDS and the carve-up of that LDS, written down from launch_tile_sort as it stood (the first launch of an asynchronous plan
    without a medium launch differs in its upper edge alone, which is an argument of the kernel and no resource)."""
    EXTRA = 9216
    long_launch = (1024, 131072, 4096, ANY, 16384, 7616)
    recorded = {
        (0, 256, 0): [(256, 2048, 0, 512, 256, 0)],
        (0, 4096, 0): [(256, 4096, 0, 512, 512, 0), (512, 4096 * 16 + EXTRA, 512, 4096, 8192, 4096)],
        (0, 4097, 0): [(256, 4096, 0, 512, 512, 0), (512, 4096 * 16 + EXTRA, 512, 4096, 8192, 4096),
                       (1024, 2 * 4096 * 8 + EXTRA, 4096, ANY, (2 * 4096 * 8 + EXTRA) // 8, 4096)],
        (0, 20011, 0): [(256, 4096, 0, 512, 512, 0), (512, 4096 * 16 + EXTRA, 512, 4096, 8192, 4096), long_launch],
        (1, 1024, 0): [(256, 4096, 0, 512, 512, 0), (512, 1024 * 16 + EXTRA, 512, 4096, 2048, 1024)],
        (1, 0, 1): [(256, 4096, 0, 512, 512, 0), (512, 4096 * 16 + EXTRA, 512, 4096, 8192, 4096), long_launch],
    }
    for mode, want in recorded.items():
        assert _plan(*mode)[1] == want, mode
    # estimates of at most 512 keys: ONE launch of 256 threads with a buffer of exactly the estimate, as before
    for keys in (1, 256, 512):
        (threads, lds_bytes, lo, hi, lds_keys, bucket_keys), = _plan(1, keys, 0)[1]
        assert (threads, lds_bytes, lo, lds_keys, bucket_keys) == (256, keys * 8, 0, keys, 0), keys
    # and the synchronous plans do not depend on anything but the longest list
    for keys in (1, 256, 512, 513, 4096, 4097, 16384, 20011):
        assert _plan(0, keys, 0)[1] == _plan(0, keys, 1)[1]
    assert [len(_plan(0, k, 0)[1]) for k in (1, 512, 513, 4096, 4097, 20011)] == [1, 1, 2, 2, 3, 3]
