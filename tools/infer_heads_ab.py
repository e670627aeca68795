#!/usr/bin/env python
"""One-kernel deformation inference for the head sets beyond dx + dshs (mlp.deform_infer_heads) against the separate kernels these
networks' no_grad renders took before (HexPlane sampler -> deform_mlp -> geometry_heads, through a [P,128] feature array).

Workload: one scene from synth.street_scene at the benchmark shape (1.2 M Gaussians, 1066 x 1600, fine stage) per network:
  static              no_dx=True                                          dshs          (arithmetic "f32": see below)
  no_dshs             no_dshs=True                                        dx
  4dgs_default        no_dshs=True feat_head=False no_ds=False no_dr=False  dx + ds + dr
  default + dr        no_dr=False                                         dx + dshs + dr: NOT served (its weights do not fit the LDS
                                                                          beside the sampler's tiles): both columns are the same route

  one-kernel   pipeline.render under no_grad as it runs (deformation.FUSED_INFERENCE = True)
  separate     the same call with deformation.FUSED_INFERENCE = False -- S3G_FUSED_INFERENCE=0, the parent commit's path for these sets

    python tools/infer_heads_ab.py [--steps 20] [--warmup 3] [--out profiles/infer_heads_ab.txt]

One model per network, one process, the inference cache off (every frame evaluates the deformation field); after the warm-up the two
routes alternate frame by frame; a device synchronise on both sides of every timed block, wall clock, medians.  Two states: a blocked
processing order cached on the grid (what a training backward leaves behind) and none (a loaded checkpoint).  Also the deformation
evaluation alone (Deformation.deform_heads) and torch.cuda.max_memory_allocated of one frame per route.
A network with the SH head takes the one-kernel route only in the exact arithmetic (mlp.set_mlp_arithmetic("f32")), where it changes no
bit; the static network is measured in that mode, both routes.
Exit status 1 if, for a served network in either state, the one-kernel route's median render is slower than the separate kernels' by more
than the spread (max - min) of the latter's own samples."""
import argparse
import os
import statistics
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

P, W, H = 1_200_000, 1600, 1066
NETWORKS = [("static (no_dx=True), arithmetic f32", dict(no_dx=True), "f32"),
            ("no_dshs=True", dict(no_dshs=True), None),
            ("4dgs default (no_dshs=True feat_head=False no_ds=False no_dr=False)", dict(no_dshs=True, feat_head=False, no_ds=False, no_dr=False), None),
            ("default + dr (no_dr=False): not served, control", dict(no_dr=False), None)]


def measure(name, over, arithmetic, sc, args, dev):
    import s3gaussian_amd.deformation as dm
    from s3gaussian_amd import mlp, raster_C
    from s3gaussian_amd.pipeline import GaussianParams, default_hyper, render
    mlp.set_mlp_arithmetic(arithmetic or mlp.DEFAULT_ARITHMETIC)
    torch.manual_seed(0)
    pc = GaussianParams(sc["sh_degree"], default_hyper(**over))
    gs = sc["gaussians"]
    pc.init_from_tensors(gs["xyz"], gs["log_scales"], gs["rotations_raw"], gs["opacity_logit"], gs["shs"], dev)
    net = pc._deformation.deformation_net
    net.set_aabb(*sc["aabb"])
    served = net._infer_heads_ok()
    cams = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in c.items()} for c in sc["cameras"]]
    bg = sc["bg"].to(dev)
    pipe = SimpleNamespace(convert_SHs_python=True, compute_cov3D_python=False, debug=False)
    by_time = {}
    for c in cams:
        by_time.setdefault(float(c["time"]), c)
    views = list(by_time.values())                      # one camera per timestamp
    xyz = pc.get_xyz.detach()
    calls = []
    real = dm.deform_infer_heads
    dm.deform_infer_heads = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    dm.INFER_CACHE = False

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def on_route(one_kernel, fn):
        dm.FUSED_INFERENCE = one_kernel
        n = len(calls)
        try:
            ms = timed(fn)
        finally:
            dm.FUSED_INFERENCE = True
        assert (len(calls) > n) == (one_kernel and served), (name, one_kernel, served)     # the two routes really are two routes
        return ms

    lines, ok = [f"{name}   [{'served' if served else 'NOT served: both columns run the separate kernels'}]"], True
    try:
        for state in ("order cached", "no order"):
            net.grid._order_cache.clear()
            if state == "order cached":                 # what a training backward leaves behind
                x = xyz.clone().requires_grad_(True)
                net.grid(x, torch.full((xyz.shape[0], 1), float(views[0]["time"]), device=dev), uniform_time=True).sum().backward()
                for p in net.grid.grids.parameters():
                    p.grad = None
                assert net.grid._order_cache.get("order") is not None
            times = {"render one-kernel": [], "render separate": [], "heads one-kernel": [], "heads separate": []}
            with torch.no_grad():
                for i in range(args.warmup + args.steps):
                    v = views[i % len(views)]
                    t = torch.full((xyz.shape[0], 1), float(v["time"]), device=dev)
                    for one in (True, False):
                        ms = on_route(one, lambda: render(v, pc, pipe, bg, stage="fine"))
                        hs = on_route(one, lambda: net.deform_heads(xyz, t, uniform_time=True, need_feat=False, with_geometry=True))
                        if i >= args.warmup:
                            times["render one-kernel" if one else "render separate"].append(ms)
                            times["heads one-kernel" if one else "heads separate"].append(hs)
                peak = {}
                for one in (True, False):
                    raster_C.invalidate_geometry_cache()
                    torch.cuda.empty_cache()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    on_route(one, lambda: render(views[0], pc, pipe, bg, stage="fine"))
                    peak[one] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
            assert (net.grid._order_cache.get("order") is not None) == (state == "order cached")
            med = {k: statistics.median(v) for k, v in times.items()}
            lines.append(f"  {state}")
            for k in times:
                lines.append(f"    {k:<18} ms: median {med[k]:8.3f}  min {min(times[k]):8.3f}  max {max(times[k]):8.3f}   ({len(times[k])} samples)")
            spread = max(times["render separate"]) - min(times["render separate"])
            slower = med["render one-kernel"] - med["render separate"]
            verdict = "within" if slower <= spread else "SLOWER than"
            lines.append(f"    render: one-kernel - separate = {slower:+.3f} ms ({verdict} the separate route's spread of {spread:.3f} ms); "
                         f"heads alone: {med['heads one-kernel'] - med['heads separate']:+.3f} ms")
            lines.append(f"    peak memory above the model during one frame, MiB: one-kernel {peak[True]:.0f}, separate {peak[False]:.0f}")
            if served and slower > spread:
                ok = False
    finally:
        dm.deform_infer_heads = real
        dm.INFER_CACHE = True
        mlp.set_mlp_arithmetic(mlp.DEFAULT_ARITHMETIC)
    return lines, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=P)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "infer_heads_ab.txt"))
    args = ap.parse_args()
    if args.steps < 20:
        raise SystemExit("infer_heads_ab.py reports medians of at least 20 frames per route")
    if not torch.cuda.is_available():
        raise SystemExit("infer_heads_ab.py measures on the GPU; there is none here (nothing measured)")
    from s3gaussian_amd import synth
    dev = torch.device("cuda:0")
    sc = synth.street_scene(P=args.points, seed=0, width=W, height=H, n_frames=4)
    lines = [f"# tools/infer_heads_ab.py --steps {args.steps} --warmup {args.warmup}: {args.points} Gaussians, {H} x {W}, stage fine, no_grad; one model per",
             f"# network, inference cache off, routes alternated frame by frame, synchronised wall clock, medians.  {torch.cuda.get_device_name(0)}"]
    all_ok = True
    for name, over, arithmetic in NETWORKS:
        block, ok = measure(name, over, arithmetic, sc, args, dev)
        lines += block
        all_ok = all_ok and ok
        torch.cuda.empty_cache()
    lines.append("# acceptance (one-kernel not slower than separate by more than the separate route's own spread, served networks, both states): "
                 + ("met" if all_ok else "NOT MET"))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
