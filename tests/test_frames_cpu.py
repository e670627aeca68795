"""CPU-only: the restatement tests/frames_ref.py against the frames the reference's own save_seperate_videos handed to its video
writers (tests/golden/video_frames.npz, written by tests/golden/make_golden_frames.py), the shares of the fixture's inputs, and the
parts of s3gaussian_amd.frames / s3g_frame_tiles that answer before any device call."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import frames_ref as fr


@pytest.fixture(scope="module")
def fixture():
    return fr.load_fixture()


def test_restatement_reproduces_every_recorded_frame(fixture):
    n, T = fr.NUM_CAMS, fr.NUM_TIMESTAMPS
    assert sorted(fixture) == sorted(fr.SIZES)
    for (H, W), case in fixture.items():
        for k in fr.KEYS:
            ch = 1 if k == "depths" else 3
            assert case["inputs"][k].shape == (n * T, ch, H, W) and case["inputs"][k].dtype == np.float32
            assert case["frames"][k].shape == (T, H, n * W, ch) and case["frames"][k].dtype == np.uint8
            mine = [fr.strip(list(case["inputs"][k][t * n:(t + 1) * n]), normalize=(k == "depths")) for t in range(T)]
            for t in range(T):
                assert np.array_equal(mine[t], case["frames"][k][t]), (H, W, k, t)
            assert np.array_equal(fr.middle(mine), case["middle"][k]) and np.array_equal(case["middle"][k], case["frames"][k][T // 2])


def test_fixture_inputs_reach_the_cases_that_matter(fixture):
    for (H, W), case in fixture.items():
        below, above, share, planted = fr.check_inputs(case["inputs"])
        print(f"{H} x {W}: below 0 {below:.3f}, above 1 {above:.3f}, truncation matters {share:.3f}, reciprocal-sensitive {planted}")


def test_each_wrong_reading_changes_recorded_bytes(fixture):
    n, T = fr.NUM_CAMS, fr.NUM_TIMESTAMPS
    for (H, W), case in fixture.items():
        for v in fr.VARIANTS:
            keys = fr.KEYS if v == "round" else ("depths",)
            changed = sum(int((fr.strip(list(case["inputs"][k][t * n:(t + 1) * n]), normalize=(k == "depths"), variant=v)
                               != case["frames"][k][t]).sum()) for k in keys for t in range(T))
            assert changed > 0, (H, W, v)


def test_strip_shape():
    from s3gaussian_amd.frames import strip_shape
    assert strip_shape(1066, 1600, 3, 3) == (1066, 4800, 3)
    assert strip_shape(5, 7, 1, 1) == (5, 7, 1)
    for bad in ((0, 7, 3, 3), (5, 0, 3, 3), (5, 7, 2, 3), (5, 7, 3, 0)):
        with pytest.raises(ValueError):
            strip_shape(*bad)


def test_cpu_tensors_are_refused():
    from s3gaussian_amd import frames
    img, strip = torch.rand(3, 5, 7), torch.zeros(5, 21, 3, dtype=torch.uint8)
    before = frames.calls
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        frames.compose(img, strip, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        frames.compose([img, img], [strip, strip], 1, normalize=[False, True])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        frames.to8b(img)
    assert frames.calls == before


def test_library_exports_the_frame_entry_points_at_abi_16():
    from s3gaussian_amd import _lib
    L = _lib.lib()
    assert _lib.ABI_VERSION == 16 and L.s3g_abi_version() == 16
    for name in ("s3g_frame_tiles", "s3g_frame_workspace_bytes"):
        assert hasattr(L, name) and name in _lib.EXPORTED_SYMBOLS


def test_job_struct_matches_the_header():
    from s3gaussian_amd import frames
    from tests.test_abi_cpu import _struct_fields
    assert _struct_fields("s3g_frames.h", "s3g_frame_job") == [f[0] for f in frames._Job._fields_]
    assert C.sizeof(frames._Job) == 40 and frames.MAX_JOBS == 8


def test_workspace_bytes_and_refusals_before_any_device_call():
    """Argument validation only: every call below returns S3G_ERR_INVALID_ARG (1) before the library touches a device; the
    pointers are made-up addresses that are never dereferenced."""
    from s3gaussian_amd import frames
    L = frames._bind()
    assert L.s3g_frame_workspace_bytes(0, 7, 1) == 0 and L.s3g_frame_workspace_bytes(5, 7, 0) == 0
    one, eight = L.s3g_frame_workspace_bytes(5, 7, 1), L.s3g_frame_workspace_bytes(1066, 1600, 8)
    assert 0 < one <= eight and one % 128 == 0 and eight % 128 == 0

    def job(src=0x1000, dst=0x2000, row=21 * 3, col=0, ch=3, norm=0):
        j = frames._Job()
        j.src, j.dst, j.dst_row_bytes, j.dst_col, j.channels, j.normalize, j.reserved = src, dst, row, col, ch, norm, 0
        return j

    def call(H, W, jobs, maxima=None, work=0x3000, n=None):
        arr = (frames._Job * max(len(jobs), 1))(*jobs)
        return L.s3g_frame_tiles(H, W, len(jobs) if n is None else n, arr if jobs else None, maxima, work, None)

    refused = {
        "no jobs": call(5, 7, [job()], n=0),
        "nine jobs": call(5, 7, [job()] * 9),
        "H < 1": call(0, 7, [job()]),
        "W < 1": call(5, 0, [job()]),
        "NULL table": L.s3g_frame_tiles(5, 7, 1, None, None, 0x3000, None),
        "NULL src": call(5, 7, [job(src=None)]),
        "NULL dst": call(5, 7, [job(dst=None)]),
        "C = 2": call(5, 7, [job(ch=2)]),
        "C = 4": call(5, 7, [job(ch=4)]),
        "negative column": call(5, 7, [job(col=-1)]),
        "tile beyond the row": call(5, 7, [job(col=15)]),
        "row of another channel count": call(5, 7, [job(row=21, col=14)]),
        "second job bad": call(5, 7, [job(), job(ch=1, row=21, col=15)]),
        "NULL workspace with a normalised job": call(5, 7, [job(ch=1, row=21, norm=1)], work=None),
    }
    for what, rc in refused.items():
        assert rc == 1, (what, rc)
    assert b"s3g_frame_tiles" in L.s3g_last_error()
