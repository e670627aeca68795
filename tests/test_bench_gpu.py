"""bench.py's output contract on a LIVE run ("the contract test tests a file, not the bench"): a small workload through
the real program in a subprocess -- with --full every path (fused / patched / import_swap / zero_diff), the roofline leg with its
live hipEvent times, the CPU baseline -- validated by the same checker the committed line of the round goes through; the plain run
(no --full) prints the headline alone and writes the last timed step's outputs (--dump-outputs)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_py_prints_one_line_that_follows_the_contract(gpu_device):
    from tests.util import validate_bench_line
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--P", "60000", "--width", "480", "--height", "320", "--frames", "4",
           "--steps", "4", "--warmup", "2", "--full"]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    validate_bench_line(d, default_workload=False)
    assert d["steps"] == 4 and d["warmup"] == 2 and d["config"]["gaussians"] == 60000 and d["config"]["image"] == [320, 480]
    # counters: collected by this very run when rocprofv3 is on the box (round 6), else absent for a non-default workload (the
    # committed profiles/kernel_traffic.json describes the default workload only)
    assert d["roofline"]["traffic"] is None or d["roofline"]["traffic_source"].startswith("collected IN THIS RUN")


def test_plain_gpus_2_command_line_starts_two_ranks(gpu_device):
    """`python bench.py --gpus 8` without torchrun printed a 1-GPU line under an 8-rank label.  The plain command must
    start the ranks itself.  One GPU per lease: the two ranks share it over gloo (S3G_DIST_BACKEND=gloo; RCCL refuses two ranks on
    one device) -- functional, not a scaling number; without that override the same command must refuse, not mislabel."""
    from tests.util import validate_bench_line
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    args = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--P", "60000", "--width", "480", "--height", "320",
            "--frames", "4", "--steps", "3", "--warmup", "2", "--full"]
    import torch
    if torch.cuda.device_count() < 2:
        out = subprocess.run(args, cwd=ROOT, capture_output=True, text=True, timeout=120, env=env)
        assert out.returncode != 0 and "refusing" in out.stderr and not [l for l in out.stdout.splitlines() if l.startswith("{")]
        env["S3G_DIST_BACKEND"] = "gloo"
    out = subprocess.run(args, cwd=ROOT, capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    validate_bench_line(d, default_workload=False, n_gpus=2)
    assert d["n_gpus"] == 2 and d["comm"]["world_size"] == 2 and len(d["comm"]["devices"]) == 2
    assert d["comm"]["scaling_curve_measured_by_the_builder"] is False


def test_plain_run_prints_the_headline_alone_and_dumps_the_last_step(gpu_device, tmp_path):
    """The plain command times the K steps and nothing else; --dump-outputs writes what the last timed step computed.  Two runs with
    the same arguments see the same inputs: in the deterministic mode of the HexPlane backward (no float atomics in the plane
    gradients, tests/test_determinism_gpu.py) their outputs agree to the last bits of the device-side reductions."""
    import numpy as np
    from tests.util import validate_bench_line
    dumps = []
    for run in range(2):
        d_out = str(tmp_path / f"run{run}")
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--P", "60000", "--width", "480", "--height", "320", "--frames", "4",
               "--steps", "5", "--warmup", "2", "--dump-outputs", d_out]
        out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600, env=dict(os.environ, S3G_HEX_DETERMINISTIC="1"))
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.strip().splitlines() if l.startswith("{")]
        assert len(lines) == 1, out.stdout[-2000:]
        d = json.loads(lines[0])
        validate_bench_line(d, default_workload=False, full=False)
        assert d["steps"] == 5 and d["warmup"] == 2 and d["config"]["gaussians"] == 60000 and d["config"]["image"] == [320, 480]
        assert d["ms_per_step"] > 0 and d["config"]["raster_async"]["calls"] >= 5
        names = sorted(f[:-4] for f in os.listdir(d_out))
        arrays = {n: np.load(os.path.join(d_out, n + ".npy")) for n in names}
        assert sum(v.nbytes for v in arrays.values()) <= 64_000_000
        assert all(v.dtype in (np.float32, np.float64) for v in arrays.values())
        assert {"loss", "render", "depth", "feat", "radii", "visibility_filter", "param_xyz", "deformation_params"} <= set(arrays)
        assert arrays["render"].shape == (3, 320, 480) and arrays["depth"].shape == (1, 320, 480)
        assert all(np.isfinite(v).all() for v in arrays.values())
        assert arrays["visibility_filter"].sum() > 0
        dumps.append(arrays)
    a, b = dumps
    assert set(a) == set(b)
    for n in a:
        assert a[n].shape == b[n].shape, n
        assert np.allclose(a[n], b[n], rtol=1e-5, atol=1e-6), (n, float(np.abs(a[n] - b[n]).max()))
