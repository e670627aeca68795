"""CPU-only: the C-ABI library loads, exports every symbol include/*.h declares, and the Python surface mirrors the
reference's names / signatures / error behaviour.  No compute calls (no GPU here)."""
import ctypes
import glob
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_functions():
    names = []
    for h in glob.glob(os.path.join(ROOT, "include", "*.h")):
        txt = re.sub(r"/\*.*?\*/", "", open(h).read(), flags=re.S)
        names += re.findall(r"\b(s3g_[a-z0-9_]+)\s*\(", txt)
    return sorted(set(n for n in names if not n.endswith("_fn")))


def test_library_exports_every_declared_symbol():
    from s3gaussian_amd import _lib
    L = _lib.lib()
    decl = _declared_functions()
    assert "s3g_raster_forward" in decl and "s3g_raster_backward" in decl
    for hook in ("s3g_raster_set_bin_band", "s3g_raster_sort_plan"):       # the testing hooks are part of the declared, exported ABI
        assert hook in decl and hook in _lib.EXPORTED_SYMBOLS
    for name in decl:
        assert hasattr(L, name), f"libs3g.so does not export {name}"
    assert L.s3g_abi_version() == _lib.ABI_VERSION
    assert set(_lib.EXPORTED_SYMBOLS) <= set(decl)


def test_raster_inputs_struct_matches_header_field_order():
    from s3gaussian_amd import _lib
    txt = open(os.path.join(ROOT, "include", "s3g_raster.h")).read()
    body = re.search(r"typedef struct s3g_raster_inputs \{(.*?)\} s3g_raster_inputs;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        for part in decl.split(","):
            fields.append(re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part)[-1])
    assert fields == [f[0] for f in _lib.RasterInputs._fields_]


def _struct_fields(header, name):
    txt = open(os.path.join(ROOT, "include", header)).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = re.sub(r"\[[^\]]*\]", "", decl.strip())      # drop array extents
        if not decl:
            continue
        for part in decl.split(","):
            fields.append(re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part)[-1])
    return fields


def test_other_structs_match_their_headers():
    """ctypes mirrors of the descriptor structs keep the headers' field order (and sizes where arrays are involved)."""
    from s3gaussian_amd import hexplane, losses, mlp
    assert _struct_fields("s3g_hexplane.h", "s3g_hexplane_desc") == [f[0] for f in hexplane._HexDesc._fields_]
    assert ctypes.sizeof(hexplane._HexDesc) == 4 + 8 * 4 * 4 + 4 + 8 * 6 * 8 + 6 * 4 + 4 + 4   # int, res, pad, planes, aabb, flag, pad
    assert _struct_fields("s3g_loss.h", "s3g_plane_reg_desc") == [f[0] for f in losses._PlaneRegDesc._fields_]
    assert _struct_fields("s3g_mlp.h", "s3g_mlp_params") == [f[0] for f in mlp._Params._fields_]
    from s3gaussian_amd import optim
    assert _struct_fields("s3g_optim.h", "s3g_adam_tensor") == [f[0] for f in optim._AdamTensor._fields_]
    assert ctypes.sizeof(optim._AdamTensor) == 56


def test_python_surface_matches_reference_names():
    import diff_gaussian_rasterization as d
    assert d.GaussianRasterizationSettings._fields == (
        "image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix", "projmatrix",
        "sh_degree", "campos", "prefiltered", "debug")
    sig = inspect.signature(d.GaussianRasterizer.forward)
    assert list(sig.parameters) == ["self", "means3D", "means2D", "opacities", "shs", "colors_precomp", "scales",
                                    "rotations", "cov3D_precomp"]
    assert hasattr(d.GaussianRasterizer, "markVisible")
    for fn in ("rasterize_gaussians", "rasterize_gaussians_backward", "mark_visible"):
        assert callable(getattr(d._C, fn))
    from simple_knn._C import distCUDA2
    assert callable(distCUDA2)


def _settings():
    import diff_gaussian_rasterization as d
    return d.GaussianRasterizationSettings(image_height=16, image_width=16, tanfovx=1.0, tanfovy=1.0, bg=torch.zeros(3),
                                           scale_modifier=1.0, viewmatrix=torch.eye(4), projmatrix=torch.eye(4), sh_degree=0,
                                           campos=torch.zeros(3), prefiltered=False, debug=False)


def test_argument_validation_raises_like_reference():
    import diff_gaussian_rasterization as d
    r = d.GaussianRasterizer(_settings())
    x = torch.zeros(4, 3)
    with pytest.raises(Exception, match="excatly one of either SHs or precomputed colors"):
        r(means3D=x, means2D=x, opacities=torch.zeros(4, 1), scales=x, rotations=torch.zeros(4, 4))
    with pytest.raises(Exception, match="exactly one of either scale/rotation pair"):
        r(means3D=x, means2D=x, opacities=torch.zeros(4, 1), colors_precomp=x, scales=x, rotations=torch.zeros(4, 4),
          cov3D_precomp=torch.zeros(4, 6))


def test_product_path_has_no_cpu_fallback():
    """CPU tensors must fail loudly, never silently route to a slow path."""
    import diff_gaussian_rasterization as d
    from simple_knn._C import distCUDA2
    r = d.GaussianRasterizer(_settings())
    x = torch.rand(4, 3)
    with pytest.raises(RuntimeError, match="GPU"):
        r(means3D=x, means2D=x, opacities=torch.zeros(4, 1), colors_precomp=x, scales=x, rotations=torch.zeros(4, 4))
    with pytest.raises(RuntimeError, match="GPU"):
        distCUDA2(x)


def test_product_package_never_imports_oracle():
    for root in ("s3gaussian_amd", "diff_gaussian_rasterization", "simple_knn"):
        for path in glob.glob(os.path.join(ROOT, root, "**", "*.py"), recursive=True):
            src = open(path).read()
            assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), path


def test_committed_bench_line_follows_the_contract():
    """profiles/rNN_bench_line.json is what `python bench.py` printed on the MI355X at the end of a round; the same validator
    runs on a LIVE bench.py invocation in tests/test_bench_gpu.py (the contract is tested on the program, not only on a file)."""
    import json
    from tests.util import validate_bench_line
    path = os.path.join(ROOT, "profiles", "r04_bench_line.json")
    if os.path.exists(path):
        d = json.loads(open(path).read().strip().splitlines()[-1])
        validate_bench_line(d, default_workload=True)
        assert d["config"]["raster_async"]["enabled"] is True and "host-asynchronous" in d["config"]["rasterizer_forward"]
        d["config"]["paths"]["something_else"] = {"ms_per_step": 1.0, "iters_per_s": 1000.0}     # an unknown path key does not pass
        with pytest.raises(AssertionError):
            validate_bench_line(d, default_workload=True)
    # round 3's lines (blend kernels priced as HBM kernels, render-loop launches mixed into the training bracket: fixed in round 4)
    for name in ("r03_bench_line.json", "r03_bench_line_split.json"):
        old = os.path.join(ROOT, "profiles", name)
        if os.path.exists(old):
            validate_bench_line(json.loads(open(old).read().strip().splitlines()[-1]), default_workload=True, round3_accounting=True)


def test_the_drivers_own_bench_records_validate():
    """BENCH_rNN.json is what the driver measured on its own box (its `parsed` is a trimmed copy of the printed line).  Round 3's
    validator rejected the driver's line (an ordering between two measured fast paths that the driver's box violated) and nobody
    noticed before the round ended: every record in the tree goes through the validator here."""
    import json
    from tests.util import validate_bench_line
    seen = 0
    for path in sorted(glob.glob(os.path.join(ROOT, "BENCH_r*.json"))):
        parsed = json.load(open(path)).get("parsed")
        if not isinstance(parsed, dict) or "value" not in parsed:
            continue
        if "roofline" not in parsed or "cpu_baseline" not in parsed or "path" not in parsed.get("config", {}):
            continue                                                      # round 1's line predates the contract's additions
        validate_bench_line(parsed, default_workload=True, trimmed=True)
        seen += 1
    if not seen:
        pytest.skip("no driver record with a roofline object in the tree")


def test_mlp_arithmetic_switch_round_trips_without_a_gpu():
    """include/s3g_mlp.h::s3g_deform_mlp_set_arithmetic is a host-side, process-wide setting: default exact fp32, the two documented
    modes accepted, anything else refused with S3G_ERR_INVALID_ARG and the setting left alone."""
    import pytest
    from s3gaussian_amd import _lib, mlp
    L = _lib.lib()
    L.s3g_last_error.restype = __import__("ctypes").c_char_p
    # (the Python binding selects mlp.DEFAULT_ARITHMETIC -- "bf16x3" since round 6 -- when it first binds the library, whose own
    #  default is the exact chain)
    assert mlp.get_mlp_arithmetic() == mlp.DEFAULT_ARITHMETIC == "bf16x3" and L.s3g_deform_mlp_get_arithmetic() == 1
    try:
        mlp.set_mlp_arithmetic("f32")
        assert mlp.get_mlp_arithmetic() == "f32" and L.s3g_deform_mlp_get_arithmetic() == 0
        mlp.set_mlp_arithmetic("bf16x3")
        assert mlp.get_mlp_arithmetic() == "bf16x3" and L.s3g_deform_mlp_get_arithmetic() == 1
        assert L.s3g_deform_mlp_set_arithmetic(7) != 0 and b"arithmetic" in L.s3g_last_error()
        assert mlp.get_mlp_arithmetic() == "bf16x3"
        with pytest.raises(ValueError):
            mlp.set_mlp_arithmetic("bf16")
    finally:
        mlp.set_mlp_arithmetic(mlp.DEFAULT_ARITHMETIC)
    with pytest.raises(ValueError):          # the inference kernel's switch is validated before anything touches a device
        mlp.deform_infer(None, None, None, None, None, None, None, arithmetic="fp16")


def test_removed_hexplane_algorithm_is_refused_not_remapped():
    """ABI 12 removed the slab-free "walk" backward (S3G_HEX_WALK = 1): the entry point must say so instead of silently running
    something else under that id (argument validation only: nothing is launched, no GPU needed)."""
    import ctypes as C
    from s3gaussian_amd import _lib
    L = _lib.lib()
    L.s3g_hexplane_backward_algo.restype = C.c_int
    rc = L.s3g_hexplane_backward_algo(None, C.c_int(0), None, None, None, None, C.c_int(1), None, None, None, None, C.c_int(0), None)
    assert rc == 1 and b"removed in ABI 12" in L.s3g_last_error()


def test_hexplane_workspace_layout_is_what_the_single_file_library_carved():
    """The carve functions of csrc/hexplane.hip are host code: no kernel comparison covers them.  The sizes they report for the
    reference field (pipeline.default_hyper: 4 levels, 64 x 64 x 64 x 25 times 1 / 2 / 4 / 8 on the spatial axes) are compared with
    literals recorded from the library of commit 7273f3a, the last one with the whole sampler in one hexplane.hip.  P = 999 999 and
    1 000 000 straddle the switch of segment_length (128 -> 256 sorted points per walker), which the deterministic records follow."""
    import ctypes as C
    from s3gaussian_amd import hexplane
    from s3gaussian_amd.pipeline import default_hyper
    L = hexplane._bind()
    hyper = default_hyper()
    base = hyper.kplanes_config["resolution"]
    assert list(base) == [64, 64, 64, 25] and list(hyper.multires) == [1, 2, 4, 8]
    assert L.s3g_hexplane_sort_state_words(4) == 25
    PS = (0, 1, 999_999, 1_000_000)
    # (deterministic, uniform_time) -> forward bytes, backward bytes per P       recorded from 7273f3a
    recorded = {
        (0, 0): (0, (6842496, 6843520, 670841984, 670842496)),
        (0, 1): (368640, (7579776, 7580800, 671579264, 671579776)),
        (1, 0): (0, (546542976, 546556288, 1283299712, 1246927744)),
        (1, 1): (368640, (547280256, 547293568, 1284036992, 1247665024)),
    }
    prev = L.s3g_hexplane_get_deterministic()
    try:
        for (det, ut), (fwd, bwd) in recorded.items():
            L.s3g_hexplane_set_deterministic(det)
            d = hexplane._HexDesc()
            d.levels = len(hyper.multires)
            d.uniform_time = ut
            for l, m in enumerate(hyper.multires):
                for k in range(4):
                    d.res[l][k] = base[k] * m if k < 3 else base[k]
            assert L.s3g_hexplane_forward_workspace_bytes(C.byref(d)) == fwd, (det, ut)
            for have_features in (0, 1):       # unused since ABI 12, still part of the signature
                got = tuple(L.s3g_hexplane_backward_workspace_bytes(C.byref(d), P, have_features) for P in PS)
                assert got == bwd, (det, ut, have_features, got)
    finally:
        L.s3g_hexplane_set_deterministic(prev)


def test_raster_arena_layout_is_what_the_single_file_library_carved():
    """GeomState / BinningState / ImageState::carve (csrc/raster_dev.hpp) are host code: no kernel comparison covers them.  The three
    byte counts s3g_raster_arena_bytes reports (it launches nothing) are compared with literals recorded from the library of commit
    72424ac, the last one with the whole forward in one raster_forward.hip.  P = 131 071 and 131 073 straddle bin_blocks saturating
    at 512 workgroups (the image arena holds their [workgroup][tile] table); the last case has counts beyond 32 bits of bytes."""
    import ctypes as C
    from s3gaussian_amd import _lib
    L = _lib.lib()
    # (P, W, H, capacity_instances, capacity_slots) -> geometry, binning, image bytes       recorded from 72424ac
    recorded = {
        (0, 16, 16, 1, 1): (0, 384, 4736),
        (1, 17, 1, 1, 1): (1152, 384, 2944),
        (131071, 1600, 1066, 1 << 20, 1 << 21): (10878976, 20971520, 27475968),
        (131073, 1600, 1066, 1 << 20, 1 << 21): (10880128, 20971520, 27475968),
        (1200000, 7680, 4320, 0x7fffffff, 0xffffffff): (99600000, 42949672960, 532917376),
    }
    for case, want in recorded.items():
        n = [C.c_size_t(), C.c_size_t(), C.c_size_t()]
        assert L.s3g_raster_arena_bytes(*case, C.byref(n[0]), C.byref(n[1]), C.byref(n[2])) == 0, case
        assert tuple(x.value for x in n) == want, (case, tuple(x.value for x in n))


def test_raster_backward_workspace_sizes_are_the_recorded_literals():
    """One record per instance: NREC = 10 floats (40 B), 14 for the two-image backward (56 B), the total rounded up to a multiple
    of 128; a negative R counts as 0 and P does not enter.  The literals are what the single-file raster_backward.hip returned."""
    from s3gaussian_amd import _lib
    L = _lib.lib()
    for P in (0, 1_000_003):
        got = [L.s3g_raster_backward_workspace_bytes(P, R) for R in (-5, 0, 1, 3, 4, 1 << 24)]
        assert got == [0, 0, 128, 128, 256, 671088640], (P, got)
        got = [L.s3g_raster_backward2_workspace_bytes(P, R) for R in (-5, 0, 1, 2, 3, 1 << 24)]
        assert got == [0, 0, 128, 128, 256, 939524096], (P, got)


def test_raster_backward_exports_keep_their_host_side_contracts():
    """The five backward exports check their arguments in one order before any device call (no GPU needed): an incomplete
    s3g_densify_accum, then NULL inputs, then P == 0 -> S3G_OK, then NULL arrays; s3g_raster_backward_alpha first treats three NULL
    accumulators as none and wants colors2 / dL_dpix2 / dL_dcolor2 together.  Every string is the one s3g_last_error gave for the
    single-file raster_backward.hip, the export's own name in front."""
    import ctypes as C
    from s3gaussian_amd import _lib
    L = _lib.lib()
    OK, INVALID = 0, 1
    # export -> index of the s3g_densify_accum argument (None: it takes none)
    exports = {"s3g_raster_backward": None, "s3g_raster_backward_accum": -2, "s3g_raster_backward2": None,
               "s3g_raster_backward2_accum": -2, "s3g_raster_backward_alpha": -2}
    keep = []     # ctypes objects the calls point at

    def call(name, inputs=None, dens=None, **at):
        fn = getattr(L, name)
        args = [0 if t is C.c_int else None for t in fn.argtypes]
        if inputs is not None:
            args[0] = C.byref(inputs)
        if dens is not None:
            args[exports[name]] = C.byref(dens)
        for i, v in at.items():
            args[int(i[1:])] = v
        keep.append((inputs, dens))
        rc = fn(*args)
        return rc, L.s3g_last_error().decode()

    def inputs_of(P):
        s = _lib.RasterInputs()
        s.P, s.width, s.height = P, 16, 16
        return s

    word = (C.c_float * 4)()
    some = C.cast(word, C.c_void_p)
    for name, dens_at in exports.items():
        assert call(name) == (INVALID, f"{name}: NULL inputs")
        assert call(name, inputs_of(0))[0] == OK
        assert call(name, inputs_of(5)) == (INVALID, f"{name}: NULL array argument")
        if dens_at is None:
            continue
        for missing in ("xyz_gradient_accum", "denom", "max_radii2D"):
            d = _lib.DensifyAccum(some, some, some)
            setattr(d, missing, None)
            want = (INVALID, f"{name}: s3g_densify_accum needs all three arrays")
            assert call(name, None, d) == want            # reported before the NULL inputs: the order of the checks
            assert call(name, inputs_of(0), d) == want    # and before P == 0 returns
        assert call(name, inputs_of(0), _lib.DensifyAccum(some, some, some))[0] == OK
    # s3g_raster_backward_alpha(in, colors2 [1], R, radii, 3 arenas, workspace, dL_dpix, dL_dpix_depth, dL_dpix2 [10], dL_dalpha,
    #                           dL_dmean2D, dL_dconic, dL_dopacity, dL_dcolor, dL_dcolor2 [16], ...)
    name = "s3g_raster_backward_alpha"
    together = (INVALID, f"{name}: colors2, dL_dpix2 and dL_dcolor2 go together (all three or none)")
    assert call(name, inputs_of(0), a1=some) == together                    # colors2 without dL_dpix2
    assert call(name, None, a1=some, a10=some) == together                  # ... without dL_dcolor2; before the NULL inputs
    assert call(name, inputs_of(0), a10=some, a16=some) == together
    assert call(name, inputs_of(0), a1=some, a10=some, a16=some)[0] == OK
    assert call(name, inputs_of(0), _lib.DensifyAccum(None, None, None))[0] == OK     # three NULL accumulators mean none
    assert call(name, None, _lib.DensifyAccum(None, None, None)) == (INVALID, f"{name}: NULL inputs")
