"""Go/no-go for LDS row windows in the two uniform-time per-point HexPlane passes, priced with a throw-away build.
S3G_LIB_PATH=.../libs3g_rowgate.so python tools/hex_row_windows_gate_probe.py [P] [rounds]

The library is the tree with tools/variants/hex_row_windows_gate.patch applied (git apply; make -C s3gaussian_amd/csrc; copy
lib/libs3g.so to lib/variants/libs3g_rowgate.so; git apply -R; make again -- no GPU needed).  With the tree's own library the three arms
run the same kernels.  That build reads S3G_HEX_ROWGATE on every call:
  0  today's kernels (one 32-point group per 256-thread workgroup)
  1  persistent 1024-thread workgroups, one per CU, contiguous slices of the processing order, every row-table read served from a
     constant LDS buffer (results WRONG on purpose): the ceiling of the change, launch shape included
  2  the same launch shape with the row tables still read from global memory: what the launch shape alone costs
Interleaved rounds in one process (the setup of tools/hex_probe.py: cfg3 aabb, 1.2 M points, blocked order cached), in-library
hipEvent brackets, CALLS forward + backward pairs per arm and round.  One JSON line."""
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from s3gaussian_amd import _lib, synth  # noqa: E402
from s3gaussian_amd.hexplane import HexPlaneField  # noqa: E402

P = int(sys.argv[1]) if len(sys.argv) > 1 else 1_200_000
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 7
CALLS = 6
FWD, POINT = 2, 3      # S3G_PROFILE_HEXPLANE_FORWARD, _HEXPLANE_BACKWARD_POINT
ARMS = {"parent": "0", "lds_rows": "1", "shape_only": "2"}
dev = torch.device("cuda:0")
sc = synth.street_scene(P=P, n_frames=2)
cfg = dict(grid_dimensions=2, input_coordinate_dim=4, output_coordinate_dim=32, resolution=[64, 64, 64, 25])
f = HexPlaneField(1.6, cfg, [1, 2, 4, 8])
f.set_aabb(*sc["aabb"])
f = f.to(dev)
xyz = sc["gaussians"]["xyz"].to(dev).requires_grad_(True)
t = torch.full((P, 1), 0.37, device=dev)
w = torch.randn(P, 128, device=dev)
L = _lib.lib()
L.s3g_profile_read.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]


def step():
    for p in f.parameters():
        p.grad = None
    out = f(xyz, t, uniform_time=True)
    (out * w).sum().backward()


def timed(arm):
    os.environ["S3G_HEX_ROWGATE"] = ARMS[arm]
    for i in (FWD, POINT):
        L.s3g_profile_read(i, None, None, None)
    L.s3g_profile_enable(1)
    for _ in range(CALLS):
        step()
    torch.cuda.synchronize()
    L.s3g_profile_enable(0)
    out = []
    for i in (FWD, POINT):
        ms = C.c_double()
        n = L.s3g_profile_read(i, C.byref(ms), None, None)
        out.append(ms.value / max(n, 1))
    return out


os.environ["S3G_HEX_ROWGATE"] = "0"
for _ in range(3):      # warm-up; the first backward leaves the blocked order in the field's cache
    step()
for arm in ARMS:
    timed(arm)
rounds = {a: {"forward": [], "point": []} for a in ARMS}
for _ in range(ROUNDS):
    for arm in ARMS:
        fw, pt = timed(arm)
        rounds[arm]["forward"].append(round(fw, 4))
        rounds[arm]["point"].append(round(pt, 4))
os.environ["S3G_HEX_ROWGATE"] = "0"
med = {a: {k: round(statistics.median(v), 4) for k, v in r.items()} for a, r in rounds.items()}
both = {a: round(m["forward"] + m["point"], 4) for a, m in med.items()}
print(json.dumps(dict(P=P, rounds=ROUNDS, calls_per_round=CALLS, device=torch.cuda.get_device_name(0), lib=os.path.basename(_lib.LIB_PATH),
                      median_ms=med, forward_plus_point_ms=both,
                      ceiling_ms=round(both["parent"] - both["lds_rows"], 4), launch_shape_ms=round(both["parent"] - both["shape_only"], 4),
                      go=bool(both["parent"] - both["lds_rows"] >= 0.15), rounds_ms=rounds)))
