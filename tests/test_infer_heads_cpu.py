"""One-kernel deformation inference for the head sets beyond dx + dshs (include/s3g_mlp.h::s3g_deform_infer_heads), the part that needs
no GPU: which of the 32 sets of {dx, ds, dr, do, dshs} the kernel serves and with how much LDS, the refusals that come before any
launch, the route predicate of `Deformation`, and the new kernel's register / scratch budget read from the built code object."""
import ctypes as C
import itertools
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(grid_dimensions=2, input_coordinate_dim=4, output_coordinate_dim=32, resolution=[8, 8, 8, 5])
HEADS = ("dx", "ds", "dr", "do", "dshs")          # bit k of the C head mask


def _must_serve():
    """The 18 sets: every non-empty subset of {dx, ds, dr, do} with at most three heads, dshs alone, dshs + one of ds / dr / do."""
    sets = [frozenset(c) for n in (1, 2, 3) for c in itertools.combinations(("dx", "ds", "dr", "do"), n)]
    sets += [frozenset(["dshs"])] + [frozenset(["dshs", g]) for g in ("ds", "dr", "do")]
    assert len(sets) == len(set(sets)) == 18
    return set(sets)


def _all_sets():
    return [frozenset(h for h, on in zip(HEADS, bits) if on) for bits in itertools.product((False, True), repeat=5)]


def _served(s):
    from s3gaussian_amd import mlp
    return mlp.infer_heads_served("dx" in s, "dshs" in s, "ds" in s, "dr" in s, "do" in s)


def _net(**over):
    from s3gaussian_amd.deformation import deform_network
    from s3gaussian_amd.pipeline import default_hyper
    return deform_network(default_hyper(kplanes_config=SMALL, **over)).deformation_net


def test_the_served_sets_are_a_superset_of_the_eighteen():
    served = {s for s in _all_sets() if _served(s)}
    assert _must_serve() <= served
    assert frozenset() not in served and frozenset(["dx", "dshs"]) not in served
    # as built, exactly the eighteen: every other set's weight image does not fit beside the sampler's staging tiles
    assert served == _must_serve()


def test_lds_bytes_of_every_set():
    from s3gaussian_amd import mlp
    L = mlp._bind()
    stage = 8 * 6912                                  # 8 waves x (32 x 36 staging floats + 2 x 8 x 9 tap slots of 16 B)
    for s in _all_sets():
        mask = sum(1 << k for k, h in enumerate(HEADS) if h in s)
        n = L.s3g_deform_infer_heads_lds_bytes(mask)
        assert n == mlp.infer_heads_lds_bytes("dx" in s, "dshs" in s, "ds" in s, "dr" in s, "do" in s)
        if not _served(s):
            assert n == 0, sorted(s)
            continue
        assert 0 < n <= 160 * 1024 and n % 16 == 0, (sorted(s), n)
        first = len(s)                                 # one 64 x 64 first layer per head
        want = 4 * ((2 + first + ("dshs" in s)) * 17 * 256 + ("dx" in s) * 9 * 256 + bool(s & {"ds", "dr", "do"}) * 9 * 256 + 640) + stage
        assert n == want, (sorted(s), n, want)
    assert L.s3g_deform_infer_heads_lds_bytes(-1) == 0 and L.s3g_deform_infer_heads_lds_bytes(32) == 0
    # the largest image served: W0 + three first layers + P2 + the shared geometry block + the biases
    assert mlp.infer_heads_lds_bytes(True, False, True, True, False) == 108032 + stage


def test_the_binding_refuses_cpu_tensors():
    from s3gaussian_amd.mlp import deform_infer_heads
    net = _net(no_dshs=True)
    xyz, t = torch.zeros(4, 3), torch.zeros(4, 1)
    with pytest.raises(RuntimeError, match="deform_infer_heads: xyz must live on the GPU"):
        deform_infer_heads(net.grid, xyz, t, net.feature_out, net.pos_deform, None)
    with pytest.raises(RuntimeError, match="deform_infer_heads: xyz must live on the GPU"):
        deform_infer_heads(net.grid, xyz, t, net.feature_out, None, net.shs_deform, (None, net.rotations_deform, None), uniform_time=True)


@pytest.mark.parametrize("over", [dict(no_dx=True), dict(no_dshs=True), dict(no_dshs=True, feat_head=False, no_ds=False, no_dr=False)])
def test_deform_heads_on_a_cpu_module_never_reaches_the_new_call(over, monkeypatch):
    from s3gaussian_amd import deformation
    net = _net(**over)
    monkeypatch.setattr(deformation, "deform_infer_heads", lambda *a, **k: pytest.fail("deform_infer_heads called for CPU tensors"))
    monkeypatch.setattr(deformation, "deform_infer", lambda *a, **k: pytest.fail("deform_infer called for CPU tensors"))
    assert deformation.FUSED_INFERENCE
    with torch.no_grad(), pytest.raises(RuntimeError, match="GPU"):      # today's route, whose sampler refuses CPU tensors by name
        net.deform_heads(torch.zeros(4, 3), torch.zeros(4, 1), need_feat=False)


def test_the_route_predicate_over_all_64_head_combinations():
    """`_infer_heads_ok`: a fused network whose set the kernel serves -- and, with the SH head on, only in the exact arithmetic, the one
    in which the separate kernels compute what this kernel computes."""
    from s3gaussian_amd import mlp
    switches = ("no_dx", "no_ds", "no_dr", "no_do", "no_dshs", "feat_head")
    try:
        for mode in ("f32", "bf16x3"):
            mlp.set_mlp_arithmetic(mode)
            count = 0
            for values in itertools.product((False, True), repeat=6):
                over = dict(zip(switches, values))
                net = _net(**over)
                s = frozenset(h for h, sw in zip(HEADS, ("no_dx", "no_ds", "no_dr", "no_do", "no_dshs")) if not over[sw])
                want = net._fused_any() and s in _must_serve() and (mode == "f32" or "dshs" not in s)
                assert net._infer_heads_ok() == want, (mode, over)
                count += want
            assert count == (2 * 18 if mode == "f32" else 2 * 14), (mode, count)      # x 2: with and without the feature head module
        assert not _net(no_dshs=True, grid_pe=2)._infer_heads_ok() and not _net(no_dshs=True, static_mlp=True)._infer_heads_ok()
    finally:
        mlp.set_mlp_arithmetic(mlp.DEFAULT_ARITHMETIC)


def test_refusals_before_any_device_call():
    """Host code only: an unserved set is S3G_ERR_INVALID_ARG (1) with a message naming it; missing weights of a requested head, a missing
    geometry struct and a descriptor that does not have four levels are refused; P == 0 returns S3G_OK.  The pointers are made-up
    addresses that are never dereferenced."""
    from s3gaussian_amd import _lib, mlp
    from s3gaussian_amd.hexplane import _HexDesc
    from s3gaussian_amd.mlp_geom import _GeomParams, _NAMES as GEOM_NAMES
    L = mlp._bind()
    L.s3g_last_error.restype = C.c_char_p
    assert L.s3g_abi_version() == _lib.ABI_VERSION
    for name in ("s3g_deform_infer_heads", "s3g_deform_infer_heads_lds_bytes"):
        assert hasattr(L, name) and name in _lib.EXPORTED_SYMBOLS
    fake = 0x1000
    d = _HexDesc()
    d.levels = 4
    for l in range(4):
        for k in range(4):
            d.res[l][k] = 8
        for i in range(6):
            d.planes[l][i] = fake
    w, gw = mlp._Params(), _GeomParams()
    for n in mlp._NAMES:
        setattr(w, n, fake)
    for n in GEOM_NAMES:
        setattr(gw, n, fake)
    fn = L.s3g_deform_infer_heads
    call = lambda P, dx, dshs, ds, dr, do, w_=w, gw_=gw, d_=d: fn(C.byref(d_), C.byref(w_) if w_ is not None else None,
                                                                    C.byref(gw_) if gw_ is not None else None, P, fake, fake, None,
                                                                    dx, dshs, ds, dr, do, fake, None)
    assert call(0, fake, None, fake, fake, None) == 0                           # P == 0: at once
    assert call(0, None, fake, None, None, None, gw_=None) == 0                 # no geometry head: gw may be NULL
    for outs, words in (((None,) * 5, (b"(empty)",)), ((fake, fake, None, None, None), (b"dx + dshs", b"s3g_deform_infer")),
                        ((fake, fake, fake, fake, fake), (b"dx + ds + dr + do + dshs", b"does not fit")),
                        ((fake, None, fake, fake, fake), (b"dx + ds + dr + do", b"does not fit")),
                        ((None, fake, fake, fake, None), (b"ds + dr + dshs", b"does not fit"))):
        assert call(5, *outs) == 1 and call(0, *outs) == 1, outs
        msg = L.s3g_last_error()
        assert b"s3g_deform_infer_heads" in msg and all(x in msg for x in words), msg
    assert call(5, fake, None, None, fake, None, gw_=None) == 1                 # a geometry head without its struct
    assert call(-1, fake, None, None, None, None) == 1
    for names, outs, struct in ((("P1", "pb1", "P2", "pb2"), (fake, None, None, None, None), w), (("S1", "sb1", "S2", "sb2"), (None, fake, None, None, None), w),
                                (("C1", "cb1", "C2", "cb2"), (None, None, fake, None, None), gw), (("R1", "rb1", "R2", "rb2"), (None, None, None, fake, None), gw),
                                (("O1", "ob1", "O2", "ob2"), (None, None, None, None, fake), gw)):
        for missing in names:
            setattr(struct, missing, None)
            assert call(5, *outs) == 1, missing
            assert b"NULL weights" in L.s3g_last_error()
            setattr(struct, missing, fake)
        # ... and an absent head's pointers may all be NULL: the call gets past the argument checks (P == 0 ends it there)
        for missing in names:
            setattr(struct, missing, None)
        other = (None, None, None, None, fake) if outs[4] is None else (fake, None, None, None, None)
        assert call(0, *other) == 0, names
        for missing in names:
            setattr(struct, missing, fake)
    d.levels = 3
    assert call(5, fake, None, None, None, None) == 1 and b"4 levels" in L.s3g_last_error()


def _resources(obj):
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), os.path.join(ROOT, "s3gaussian_amd", "lib", obj)],
                         capture_output=True, text=True, timeout=300).stdout
    res = {}
    for line in out.splitlines():
        m = re.match(r"(\S+)\s+vgpr\s+(\d+).*?lds\s+(\d+)\s+scratch\s+(\d+)", line)
        if m:
            res[m.group(1)] = (int(m.group(2)), int(m.group(3)), int(m.group(4)))
    return res


def test_the_new_kernels_fit_two_waves_per_simd_without_scratch():
    from s3gaussian_amd import _lib
    _lib.build()
    res = _resources("deform_infer_heads.o")
    assert res, "tools/kernel_resources.sh found no kernels (llvm-objcopy / clang-offload-bundler / llvm-readelf)"
    for needle in ("deform_infer_heads_kernelILb1E", "deform_infer_heads_kernelILb0E"):      # uniform / per-point time
        hits = [v for k, v in res.items() if needle in k]
        assert len(hits) == 1, (needle, sorted(res))
        vgpr, static_lds, scratch = hits[0]
        assert vgpr <= 256 and scratch == 0 and static_lds == 0, (needle, hits[0])
