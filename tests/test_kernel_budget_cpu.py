"""CPU-only: register / scratch budgets of the kernels whose speed hangs on an occupancy step (read from the gfx950 code objects
hipcc cross-compiled into s3gaussian_amd/lib/*.o).  Round 4 lost 0.16 ms when a two-line change pushed the division-form per-point
pass from 126 to 128 VGPRs + 64 B of scratch -- still "four waves per SIMD" on paper, 0.76 -> 0.92 ms on the GPU -- and only a
bench line showed it.  This is the cheap guard: the budgets DESIGN.md quotes, asserted on the build."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _resources(obj):
    out = subprocess.run(["bash", os.path.join(ROOT, "tools", "kernel_resources.sh"), os.path.join(ROOT, "s3gaussian_amd", "lib", obj)],
                         capture_output=True, text=True, timeout=300).stdout
    res = {}
    for line in out.splitlines():
        m = re.match(r"(\S+)\s+vgpr\s+(\d+).*?lds\s+(\d+)\s+scratch\s+(\d+)", line)
        if m:
            res[m.group(1)] = (int(m.group(2)), int(m.group(4)))
            LDS[m.group(1)] = int(m.group(3))
    return res


LDS = {}    # kernel -> static LDS bytes, filled by _resources


@pytest.fixture(scope="module")
def built():
    from s3gaussian_amd import _lib
    _lib.build()
    return True


def _one(res, needle):
    hits = [(k, v) for k, v in res.items() if needle in k]
    assert len(hits) == 1, (needle, [k for k, _ in hits])
    return hits[0][1]


def test_hexplane_kernels_keep_their_occupancy(built):
    res = _resources("hexplane_point.o")
    assert res, "tools/kernel_resources.sh found no kernels (llvm-objcopy / clang-offload-bundler / llvm-readelf)"
    vgpr, scratch = _one(res, "hexplane_backward_pointdiv_kernelILb1E")        # uniform time: four waves per SIMD, no spills
    assert vgpr <= 128 and scratch == 0, (vgpr, scratch)
    res = _resources("hexplane_scatter.o")
    vgpr, scratch = _one(res, "hexplane_scatter_kernelILb1ELb0E")             # single-entry footprint, one level per walk
    assert vgpr <= 72 and scratch == 0, (vgpr, scratch)          # round 6 (16-point tap groups, packed corner pairs): seven waves
    vgpr, scratch = _one(res, "hexplane_scatter_kernelILb1ELb1E")             # the deterministic mode's walk (run records, no atomics)
    assert vgpr <= 80 and scratch == 0, (vgpr, scratch)                        # six waves per SIMD
    vgpr, scratch = _one(_resources("hexplane.o"), "hexplane_forward_kernelILb1E")
    assert vgpr <= 102 and scratch == 0, (vgpr, scratch)                       # five waves per SIMD


def test_mlp_and_raster_kernels_do_not_spill(built):
    mlp = _resources("mlp.o")
    for obj, needle in ((mlp, "mlp_forward_kernelILb0E"), (mlp, "mlp_backward_kernelILb0E"), (_resources("mlp_wgrad.o"), "mlp_wgrad_all_kernel"),
                        (_resources("deform_infer.o"), "deform_infer_kernelILb1ELb0E")):
        vgpr, scratch = _one(obj, needle)
        assert vgpr <= 256 and scratch == 0, (needle, vgpr, scratch)
    # round 5: the bf16x3 chains with pre-split weight images (159 KiB of LDS: one workgroup per CU, two waves per SIMD)
    vgpr, scratch = _one(mlp, "mlp_backward_presplit_kernel")
    assert vgpr <= 256 and scratch == 0, (vgpr, scratch)
    vgpr, scratch = _one(mlp, "mlp_forward_presplit_kernel")
    assert vgpr <= 256 and scratch <= 16, (vgpr, scratch)          # three spilled dwords as built; more would show in its 0.55 ms
    bwd = {**_resources("raster_blend_backward.o"), **_resources("raster_geom_backward.o")}
    assert len(bwd) == 6 and sum("blend_backward_kernel" in k for k in bwd) == 4 and sum("geometry_backward_kernel" in k for k in bwd) == 2, sorted(bwd)
    for k, (vgpr, scratch) in bwd.items():
        assert scratch == 0, (k, vgpr, scratch)


def test_round4_latency_fixes_keep_their_occupancy(built):
    """The three late fixes of round 4 bought latency hiding with registers / LDS; each has a step it must stay under."""
    bwd = _resources("raster_geom_backward.o")
    for needle in ("geometry_backward_kernelILi0E", "geometry_backward_kernelILi3E"):
        vgpr, scratch = _one(bwd, needle)          # three tiles of a rect in flight: still five waves per SIMD (four tiles: 105)
        assert vgpr <= 96 and scratch == 0, (needle, vgpr, scratch)
    fwd = _resources("raster_bin.o")
    for needle in ("bin_kernelILb0E", "bin_kernelILb1E"):
        vgpr, scratch = _one(fwd, needle)          # 512 threads x 2 workgroups per CU = four waves per SIMD
        assert vgpr <= 128 and scratch == 0, (needle, vgpr, scratch)
    glue = _resources("glue.o")
    vgpr, scratch = _one(glue, "glue_forward_kernelE")
    assert vgpr <= 128 and scratch == 0, (vgpr, scratch)
    lds = [v for k, v in LDS.items() if "glue_forward_kernelE" in k][0]
    assert 3 * lds <= 160 * 1024, lds              # 256 rows x 49 floats: three workgroups per CU


def _disassemble(obj):
    import tempfile
    LL = "/opt/rocm/lib/llvm/bin"
    with tempfile.TemporaryDirectory() as T:
        subprocess.run([f"{LL}/llvm-objcopy", f"--dump-section=.hip_fatbin={T}/fb", os.path.join(ROOT, "s3gaussian_amd", "lib", obj)], check=True)
        subprocess.run([f"{LL}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={T}/fb",
                        f"--output={T}/co", "--unbundle"], check=True)
        text = subprocess.run([f"{LL}/llvm-objdump", "-d", "--no-show-raw-insn", f"{T}/co"], check=True, capture_output=True, text=True).stdout
    kernels, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:", line)
        if m:
            name = m.group(1)
            kernels[name] = []
        elif name and line.startswith("\t"):
            kernels[name].append(line.split("//")[0].strip())
    return kernels


def _vregs(tok):
    m = re.match(r"v\[(\d+):(\d+)\]", tok)
    if m:
        return list(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"v(\d+)$", tok)
    return [int(m.group(1))] if m else []


def _last_writers_of_b128_stores(ins):
    """For every ds_write_b128: the opcode that last wrote each of its four data registers."""
    out = []
    for i, l in enumerate(ins):
        if not l.startswith("ds_write_b128"):
            continue
        data = _vregs(l.split(None, 1)[1].split(",")[1].split()[0])
        last = {}
        for j in range(i - 1, max(i - 600, -1), -1):
            parts = ins[j].split(None, 1)
            if len(parts) < 2 or parts[0].startswith(("ds_write", "global_store", "buffer_store", "s_", "v_cmp")):
                continue
            for r in _vregs(parts[1].split(",")[0].strip()):
                if r in data and r not in last:
                    last[r] = parts[0]
            if len(last) == len(data):
                break
        out.append([last.get(r, "?") for r in data])
    return out


def test_split_inference_kernel_keeps_the_guard_of_its_staging_stores(built):
    """VERDICT r4 weak #12.  deform_infer_kernel<UT, SPLIT = true> parks the sampler's float4 products in LDS beside the other wave's
    bf16 (XDL) MFMAs.  A DS store whose data registers were last written by a PACKED fp32 instruction reads stale data for the last
    quarter of the wave there (110 872 wrong rows in 1000 launches, profiles/r04_split_hazard.jsonl); the cure is a register
    dependency on a single-pass write -- four `v_mov_b32 vN, vN` in front of the store (deform_infer.hip) -- which lives or dies with the
    compiler not folding the moves away.  This asserts it on the BUILT code object: in both split kernels every 16-byte staging store
    takes its data from v_mov_b32, none takes it from v_pk_mul_f32; the exact kernels (no XDL ops beside them) show what the
    unguarded form looks like."""
    k = _disassemble("deform_infer.o")
    def one(needle):
        hits = [v for n, v in k.items() if needle in n]
        assert len(hits) == 1, needle
        return _last_writers_of_b128_stores(hits[0])
    for needle, n_staging in (("deform_infer_kernelILb1ELb1E", 2), ("deform_infer_kernelILb0ELb1E", 1)):
        stores = one(needle)
        guarded = [s for s in stores if all(op.startswith("v_mov_b32") for op in s)]
        assert len(guarded) == n_staging, (needle, stores)
        assert not any(all(op.startswith("v_pk_mul_f32") for op in s) for s in stores), (needle, stores)
    # the exact kernels: the same stores straight out of the packed multiplies (harmless beside fp32 MFMAs)
    for needle, n_staging in (("deform_infer_kernelILb1ELb0E", 2), ("deform_infer_kernelILb0ELb0E", 1)):
        stores = one(needle)
        assert sum(all(op.startswith("v_pk_mul_f32") for op in s) for s in stores) == n_staging, (needle, stores)
