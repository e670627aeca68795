"""CPU-only: the restatement tests/split_ref.py against what the reference's own save_ply_split handed to its PLY writer
(tests/golden/split_pcd.npz, written by tests/golden/make_golden_split.py), and the parts of s3gaussian_amd.split / the
s3g_split_* entry points that answer before any device call."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import split_ref as sr


@pytest.fixture(scope="module")
def fixture():
    return sr.load_fixture()


def test_fixture_meets_the_conditions_its_generator_asserts(fixture):
    P = int(fixture["P"])
    assert P == 1000 and P % 64 != 0 and int(fixture["sh_degree"]) == 3 and int(fixture["dx_index"]) == 24
    m = sr.max_abs(fixture["dx"])
    assert sr.no_near_tie(m, fixture["thre"], float(fixture["tie_gap"])) and float(fixture["tie_gap"]) == sr.TIE_GAP
    share = fixture["mask"].mean()
    assert 0.05 <= share <= 0.50
    assert fixture["dynamic_rows"].shape == (int(fixture["mask"].sum()), 62) and fixture["static_rows"].shape == (P - int(fixture["mask"].sum()), 62)
    assert list(fixture["names"]) == sr.attribute_names(15)


def test_restatement_reproduces_the_reference_mask_and_both_tables(fixture):
    mask, thre, m = sr.motion_mask(fixture["dx"])
    assert np.array_equal(mask, fixture["mask"])
    assert thre == np.float32(fixture["mean_f64"])                      # the float64 mean, rounded once
    assert abs(float(thre) - float(fixture["thre"])) <= np.spacing(np.float32(fixture["thre"]))     # torch's fp32 mean: last bit at most
    full = sr.table(*(fixture[k] for k in sr.INPUTS), dx=fixture["dx"])
    dynamic, static = sr.split_tables(mask, full)
    assert dynamic.tobytes() == fixture["dynamic_rows"].tobytes()
    assert static.tobytes() == fixture["static_rows"].tobytes()
    # channel-major SH: column 9 + ch * 15 + k of a row is f_rest[i, k, ch]
    i = int(np.where(mask)[0][3])
    assert dynamic[3, 9 + 1 * 15 + 4] == fixture["f_rest"][i, 4, 1] and dynamic[3, 3:6].tolist() == [0, 0, 0]
    assert np.array_equal(dynamic[3, :3], fixture["xyz"][i] + fixture["dx"][i])


def test_block_offsets_restatement(fixture):
    off = sr.block_offsets(fixture["mask"])
    assert off.shape == (5,) and off[0] == 0 and off[-1] == fixture["mask"].sum()
    assert off[2] == fixture["mask"][:512].sum()
    assert sr.block_offsets(np.zeros(0, bool)).tolist() == [0, 0]


def test_library_exports_the_split_entry_points():
    from s3gaussian_amd import _lib, split
    L = split._bind()
    for name in ("s3g_split_count_words", "s3g_split_workspace_bytes", "s3g_split_classify", "s3g_split_mask_offsets",
                 "s3g_split_pack_rows"):
        assert hasattr(L, name) and name in _lib.EXPORTED_SYMBOLS
    assert L.s3g_abi_version() == _lib.ABI_VERSION


def test_structs_match_the_header():
    from s3gaussian_amd import split
    from tests.test_abi_cpu import _struct_fields
    assert _struct_fields("s3g_split.h", "s3g_split_pack_plan") == [f[0] for f in split._PackPlan._fields_]
    assert _struct_fields("s3g_split.h", "s3g_split_stats") == [f[0] for f in split._Stats._fields_]
    assert C.sizeof(split._PackPlan) == 16 + 11 * 8 and C.sizeof(split._Stats) == 8
    assert split.BLOCK == 256 and split.row_width(15) == 62 and [split.row_width(r) for r in (0, 3, 8)] == [17, 26, 41]
    with pytest.raises(ValueError):
        split.row_width(5)


def test_sizes_and_refusals_before_any_device_call():
    """Argument validation only: every refused call returns S3G_ERR_INVALID_ARG (1) and every P == 0 call S3G_OK (0) before the
    library touches a device; the pointers are made-up addresses that are never dereferenced."""
    from s3gaussian_amd import split
    L = split._bind()
    assert [L.s3g_split_count_words(P) for P in (0, 1, 256, 257, 1000, 70001)] == [2, 2, 2, 3, 5, 275]
    assert L.s3g_split_workspace_bytes(1) == L.s3g_split_workspace_bytes(2_500_000) == 512 * 8
    a = 0x1000
    assert L.s3g_split_classify(0, None, None, None, None, None, None) == 0
    assert L.s3g_split_mask_offsets(0, None, None, None, None) == 0
    refused = {
        "classify P < 0": L.s3g_split_classify(-1, a, a, a, a, a, None),
        "classify NULL dx": L.s3g_split_classify(5, None, a, a, a, a, None),
        "classify NULL mask": L.s3g_split_classify(5, a, None, a, a, a, None),
        "classify NULL offsets": L.s3g_split_classify(5, a, a, None, a, a, None),
        "classify NULL stats": L.s3g_split_classify(5, a, a, a, None, a, None),
        "classify NULL workspace": L.s3g_split_classify(5, a, a, a, a, None, None),
        "offsets P < 0": L.s3g_split_mask_offsets(-1, a, a, None, None),
        "offsets NULL mask": L.s3g_split_mask_offsets(5, None, a, None, None),
        "offsets NULL offsets": L.s3g_split_mask_offsets(5, a, None, None, None),
    }
    for what, rc in refused.items():
        assert rc == 1, (what, rc)
    assert b"s3g_split" in L.s3g_last_error()

    def plan(P=5, R=15, mask=None, offsets=None, out_a=a, out_b=None, rows_a=5, rows_b=0, **over):
        f = dict(xyz=a, dx=None, f_dc=a, f_rest=a, opacity=a, scaling=a, rotation=a)
        f.update(over)
        return split._PackPlan(P, R, rows_a, rows_b, f["xyz"], f["dx"], f["f_dc"], f["f_rest"], f["opacity"], f["scaling"], f["rotation"], mask, offsets,
                               out_a, out_b)

    assert L.s3g_split_pack_rows(C.byref(plan(P=0, xyz=None, out_a=None)), None) == 0
    refused = {
        "NULL plan": L.s3g_split_pack_rows(None, None),
        "P < 0": L.s3g_split_pack_rows(C.byref(plan(P=-1)), None),
        "R = 5": L.s3g_split_pack_rows(C.byref(plan(R=5)), None),
        "R < 0": L.s3g_split_pack_rows(C.byref(plan(R=-3)), None),
        "NULL f_rest at R = 3": L.s3g_split_pack_rows(C.byref(plan(R=3, f_rest=None)), None),
        "no out_a without a mask": L.s3g_split_pack_rows(C.byref(plan(out_a=None, out_b=a)), None),
        "mask without offsets": L.s3g_split_pack_rows(C.byref(plan(mask=a, out_b=a)), None),
        "mask without any output": L.s3g_split_pack_rows(C.byref(plan(mask=a, offsets=a, out_a=None, rows_a=0)), None),
        "mask, rows without their output": L.s3g_split_pack_rows(C.byref(plan(mask=a, offsets=a, out_a=a, rows_a=2, rows_b=3)), None),
        "fewer rows than P without a mask": L.s3g_split_pack_rows(C.byref(plan(rows_a=4)), None),
        "negative rows": L.s3g_split_pack_rows(C.byref(plan(mask=a, offsets=a, out_b=a, rows_a=-1, rows_b=6)), None),
    }
    for name in ("xyz", "f_dc", "opacity", "scaling", "rotation"):
        refused[f"NULL {name}"] = L.s3g_split_pack_rows(C.byref(plan(**{name: None})), None)
    for what, rc in refused.items():
        assert rc == 1, (what, rc)
    assert b"s3g_split_pack_rows" in L.s3g_last_error()


def test_cpu_tensors_are_refused():
    from s3gaussian_amd import split
    P = 4
    before = split.calls
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        split.motion_classify(torch.zeros(P, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        split.pack_ply_rows(torch.zeros(P, 3), torch.zeros(P, 1, 3), torch.zeros(P, 15, 3), torch.zeros(P, 1), torch.zeros(P, 3),
                            torch.zeros(P, 4))
    assert split.calls == before


def test_save_ply_split_reads_entry_24_like_the_reference():
    """A list shorter than 25 raises the reference's IndexError (scene/gaussian_model.py:286) before anything else happens."""
    from s3gaussian_amd.pipeline import GaussianParams, default_hyper
    pc = GaussianParams(3, default_hyper())
    with pytest.raises(IndexError):
        pc.save_ply_split("unused_dynamic.ply", "unused_static.ply", [torch.zeros(1, 3)] * 24, None)
