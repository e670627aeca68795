#!/usr/bin/env python
"""Point-cloud export: the packer route against what a user had before it existed.

  table     device tensors -> ONE host buffer holding the vertex table of save_ply.  packer: split.pack_ply_rows (one launch) and one
            device-to-host copy.  numpy: the route of GaussianParams.save_ply before the packer -- two transposed .contiguous()
            copies of the SH tensors, seven device-to-host copies, np.concatenate.
  split     dx -> two host buffers, the dynamic and the static table of save_ply_split.  packer: motion_classify (four launches),
            one 4-byte host read, pack_ply_rows with the mask, two device-to-host copies.  numpy: max|dx| > mean on torch ops, then
            per class seven boolean-index gathers and the numpy route above (the reference's own method additionally fills its
            structured arrays through one Python tuple per Gaussian; that is not timed here).
  kernel    the packer launch alone (no mask), output preallocated: events around the call, and the GB/s it implies counting one
            read and one write of the rows (2 x 4 W bytes per Gaussian).

    python tools/split_ab.py [--reps 20] [--warmup 3] [--out profiles/split_ab.txt] [--points 1200000]

The routes alternate in one process; table and split are host wall-clock times around work that ends with the data on the host
(every route's last step is a blocking copy); medians, minima and maxima over the repetitions.  The routes' buffers are compared as
well.  There is no speed gate."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")


def numpy_table(t, idx=None, dx=None):
    """GaussianParams.save_ply's table before the packer (with idx / dx: save_ply_split's, per class)."""
    pick = (lambda a: a) if idx is None else (lambda a: a[idx])
    n = lambda a: a.detach().cpu().numpy()
    xyz = n(pick(t["xyz"] if dx is None else t["xyz"] + dx))
    cols = [xyz, np.zeros_like(xyz), n(pick(t["f_dc"]).transpose(1, 2).flatten(start_dim=1).contiguous()),
            n(pick(t["f_rest"]).transpose(1, 2).flatten(start_dim=1).contiguous()), n(pick(t["opacity"])), n(pick(t["scaling"])),
            n(pick(t["rotation"]))]
    return np.concatenate(cols, axis=1)


def numpy_split(t, dx):
    m = torch.max(torch.abs(dx), dim=1)[0]
    mask = m > torch.mean(m)
    return numpy_table(t, mask, dx), numpy_table(t, ~mask, dx)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def summary(lines, times, what):
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        lines.append(f"  {k:8s} ms per {what}: median {med[k]:.3f}  min {min(v):.3f}  max {max(v):.3f}")
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--points", type=int, default=1_200_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split_ab.txt"))
    args = ap.parse_args()
    if args.reps < 20:
        raise SystemExit("split_ab.py reports medians of at least 20 repetitions")
    if not torch.cuda.is_available():
        raise SystemExit("split_ab.py measures on the GPU; there is none here (nothing measured)")
    from s3gaussian_amd import split
    dev = torch.device("cuda:0")
    P, R = args.points, 15
    W = split.row_width(R)
    g = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g).to(dev)
    t = dict(xyz=r(P, 3) * 20, f_dc=r(P, 1, 3), f_rest=r(P, R, 3) * 0.2, opacity=r(P, 1), scaling=r(P, 3) - 3, rotation=r(P, 4))
    dx = (torch.exp(1.5 * torch.randn(P, 1, generator=g)) * 0.02 * (torch.rand(P, 3, generator=g) * 2 - 1)).to(dev)
    tensors = [t[k] for k in NAMES]
    lines = [f"# tools/split_ab.py --reps {args.reps} --warmup {args.warmup} --points {P}: PLY vertex tables, SH degree 3 ({W} floats per row),",
             f"# packer route vs the numpy route a user had before, alternated in one process, medians.  {torch.cuda.get_device_name(0)}; "
             f"{torch.get_num_threads()} torch threads"]

    # ---- (a) save_ply's table ---------------------------------------------------------------------------------------------------------
    routes = {"packer": lambda: split.pack_ply_rows(*tensors).cpu().numpy(), "numpy": lambda: numpy_table(t)}
    times, res = {k: [] for k in routes}, {}
    for rep in range(args.warmup + args.reps):
        for k, fn in routes.items():
            ms, res[k] = wall(fn)
            if rep >= args.warmup:
                times[k].append(ms)
    lines.append(f"table: {P} Gaussians -> one host buffer of {P * W * 4 / 1e6:.0f} MB (host wall clock, ends with the data on the host)")
    med = summary(lines, times, "table")
    lines.append(f"  numpy / packer (medians): {med['numpy'] / med['packer']:.2f} x;  buffers byte-equal: "
                 f"{res['packer'].tobytes() == np.ascontiguousarray(res['numpy'], dtype='<f4').tobytes()}")
    res.clear()

    # ---- (b) the whole split ------------------------------------------------------------------------------------------------------------
    def packer_split():
        mask, _, _, offsets = split.motion_classify(dx, return_offsets=True)
        a, b = split.pack_ply_rows(*tensors, dx=dx, mask=mask, offsets=offsets)
        return a.cpu().numpy(), b.cpu().numpy()

    routes = {"packer": packer_split, "numpy": lambda: numpy_split(t, dx)}
    times = {k: [] for k in routes}
    for rep in range(args.warmup + args.reps):
        for k, fn in routes.items():
            ms, res[k] = wall(fn)
            if rep >= args.warmup:
                times[k].append(ms)
    nd = res["packer"][0].shape[0]
    lines.append(f"split: classify + scan + pack -> two host buffers ({nd} dynamic + {P - nd} static rows); numpy: torch mask, boolean "
                 f"indexing, the numpy route per class")
    med = summary(lines, times, "split")
    same = all(a.shape == b.shape and a.tobytes() == np.ascontiguousarray(b, dtype="<f4").tobytes() for a, b in zip(res["packer"], res["numpy"]))
    lines.append(f"  numpy / packer (medians): {med['numpy'] / med['packer']:.2f} x;  both tables byte-equal: {same}"
                 + ("" if same else "  (a point within the last bit of the two thresholds changes class: fp32 mean vs float64 mean)"))
    res.clear()

    # ---- (c) the kernels alone -----------------------------------------------------------------------------------------------------------
    out = torch.empty((P, W), dtype=torch.float32, device=dev)
    times = {"pack": [], "classify": []}
    for rep in range(args.warmup + args.reps):
        ms_p, _ = events(lambda: split.pack_ply_rows(*tensors, out=out))
        ms_c, _ = events(lambda: split.motion_classify(dx))
        if rep >= args.warmup:
            times["pack"].append(ms_p)
            times["classify"].append(ms_c)
    lines.append("kernels (device events around the call: the launch(es) and the host code between them; outputs preallocated for pack)")
    med = summary(lines, times, "call")
    moved = 2 * P * W * 4
    lines.append(f"  pack: {moved / 1e6:.0f} MB (one read and one write of the rows) -> {moved / 1e6 / med['pack']:.0f} GB/s;  "
                 f"classify: four launches, {P * 24 / 1e6:.0f} MB read")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
