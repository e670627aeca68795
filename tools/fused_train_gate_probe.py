"""Go/no-go for a fused training forward (HexPlane sampler + bf16x3 MLP chain in one kernel), priced from the kernels that exist.
python tools/fused_train_gate_probe.py [P] [rounds]      (cfg3: 1 200 000 points, blocked processing order cached)

Interleaved rounds in one process, in-library hipEvent brackets (s3g_profile_*), five calls per arm and round:
  pair      hexplane_forward (training: features kept for autograd) + mlp_forward (bf16x3, stash + mask words + feature head):
            the two kernels one training step runs and a fused kernel would replace
  infer     deform_infer_kernel<UT, split> (s3g_deform_infer_split): sampler + feature_out + position / SH heads in one kernel.
            Its work is a strict subset of the fused training kernel's -- no [P,128] feature store, no stash, no mask words, no
            feature head -- and it has 48 KB of LDS staging and LDS tap sharing that the 159 KiB training weight image leaves no
            room for
  mlp_lean  mlp_forward bf16x3 without stash and feature head (what the training forward adds on the MLP side is pair's
            mlp_forward minus this); and with the feature head but without stash (head work vs stash stores)
One JSON line: per-arm medians and mins, and the gate: a fused kernel must beat `pair` by >= 0.18 ms."""
import ctypes as C
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from s3gaussian_amd import _lib, synth  # noqa: E402
from s3gaussian_amd.deformation import deform_network  # noqa: E402
from s3gaussian_amd.mlp import deform_infer, deform_mlp, get_mlp_arithmetic  # noqa: E402
from s3gaussian_amd.pipeline import default_hyper  # noqa: E402

P = int(sys.argv[1]) if len(sys.argv) > 1 else 1_200_000
ROUNDS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
CALLS = 5
HEX, MLP, INFER = 2, 5, 9      # S3G_PROFILE_HEXPLANE_FORWARD, _MLP_FORWARD, _DEFORM_INFER
dev = torch.device("cuda:0")
sc = synth.street_scene(P=P, n_frames=2)
net = deform_network(default_hyper())
net.deformation_net.set_aabb(*sc["aabb"])
d = net.to(dev).deformation_net
xyz = sc["gaussians"]["xyz"].to(dev)
t = torch.full((P, 1), 0.37, device=dev)
x = xyz.clone().requires_grad_(True)
d.grid(x, t, uniform_time=True).sum().backward()     # leaves the blocked processing order in the field's cache
L = _lib.lib()
L.s3g_profile_read.argtypes = [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
heads = (d.feature_out, d.pos_deform, d.shs_deform, d.dino_head)


def pair():
    f = d.grid(x, t, uniform_time=True)
    out = deform_mlp(f, *heads, need_feat=True)
    assert f.grad_fn is not None and out[2] is not None     # the training forward: autograd graph, stash, feature head
    return out


def infer():
    with torch.no_grad():
        return deform_infer(d.grid, xyz, t, *heads, uniform_time=True, arithmetic="bf16x3")


def mlp_lean(f, need_feat=False):
    with torch.no_grad():
        return deform_mlp(f, *heads, need_feat=need_feat)


def timed(fn, ids):
    for i in ids:
        L.s3g_profile_read(i, None, None, None)
    L.s3g_profile_enable(1)
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    L.s3g_profile_enable(0)
    out = []
    for i in ids:
        ms = C.c_double()
        launches[i] = L.s3g_profile_read(i, C.byref(ms), None, None)
        out.append(ms.value / CALLS)     # per call, whatever the number of bracketed launches in it
    return out


launches = {}


with torch.no_grad():
    feats = d.grid(xyz, t, uniform_time=True)
for _ in range(2):      # warm-up: code objects, allocator
    pair(), infer(), mlp_lean(feats)
torch.cuda.synchronize()
arms = {k: [] for k in ("hexplane_forward", "mlp_forward_train", "pair", "infer_split", "mlp_forward_lean", "mlp_forward_feat_no_stash")}
for _ in range(ROUNDS):
    h, m = timed(pair, (HEX, MLP))
    arms["hexplane_forward"].append(h)
    arms["mlp_forward_train"].append(m)
    arms["pair"].append(h + m)
    arms["infer_split"].append(timed(infer, (INFER,))[0])
    arms["mlp_forward_lean"].append(timed(lambda: mlp_lean(feats), (MLP,))[0])
    arms["mlp_forward_feat_no_stash"].append(timed(lambda: mlp_lean(feats, True), (MLP,))[0])
med = {k: round(statistics.median(v), 4) for k, v in arms.items()}
mins = {k: round(min(v), 4) for k, v in arms.items()}
training_adds_mlp = med["mlp_forward_train"] - med["mlp_forward_lean"]
print(json.dumps(dict(
    P=P, rounds=ROUNDS, calls_per_round=CALLS, bracketed_launches_per_round=launches, mlp_arithmetic=get_mlp_arithmetic(),
    device=torch.cuda.get_device_name(0),
    median_ms=med, min_ms=mins, rounds_ms={k: [round(x, 4) for x in v] for k, v in arms.items()},
    gate=dict(need_fused_ms_at_most=round(med["pair"] - 0.18, 4),
              infer_subset_gain_ms=round(med["pair"] - med["infer_split"], 4),
              mlp_training_additions_ms=round(training_adds_mlp, 4),
              estimate_fused_ms=round(med["infer_split"] + training_adds_mlp, 4)))))
