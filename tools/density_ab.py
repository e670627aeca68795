#!/usr/bin/env python
"""One densify + prune event at full size: the native route (s3gaussian_amd/density.py, four launches and one 12-byte host read per
operation) against the torch-op route a user had to run before it existed -- the boolean-index / cat sequence of the reference's
densify_and_clone, densify_and_split, prune_points (scene/gaussian_model.py:412-522, 661-678), restated here on torch ops the way the
helpers of tests/test_cfg5_flow_gpu.py do, with the reference's mask arithmetic.

    python tools/density_ab.py [--points 1200000] [--reps 10] [--out profiles/density_control_ab.txt]

Model: P Gaussians, SH degree 3, Adam moments present, inputs seeded so that about 5 % clone, 3 % split and 8 % are pruned.  The two
routes alternate; every timed event starts from a fresh copy of the same model and is bracketed by device synchronisations (host
clock around work that ends in a synchronise).  Moved bytes are computed from the shapes: every per-Gaussian float and both moments
read once and written once."""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GROUPS = (("xyz", "_xyz", (3,)), ("f_dc", "_features_dc", (1, 3)), ("f_rest", "_features_rest", (15, 3)), ("opacity", "_opacity", (1,)),
          ("scaling", "_scaling", (3,)), ("rotation", "_rotation", (4,)))


class Model:
    """What density control touches of a GaussianParams: the six per-Gaussian parameters in single-parameter Adam groups with their
    moments, the accumulators, the deformation table."""
    percent_dense = 0.01

    def __init__(self, template):
        from s3gaussian_amd.optim import Adam
        groups = []
        for name, attr, _ in GROUPS:
            setattr(self, attr, nn.Parameter(template[attr].clone()))
            groups.append({"params": [getattr(self, attr)], "lr": 1e-3, "name": name})
        self.optimizer = Adam(groups, lr=0.0, eps=1e-15)
        for name, attr, _ in GROUPS:
            self.optimizer.state[getattr(self, attr)] = {"step": torch.tensor(5.0), "exp_avg": template["m" + attr].clone(),
                                                         "exp_avg_sq": template["v" + attr].clone()}
        self.xyz_gradient_accum, self.denom = template["accum"].clone(), template["denom"].clone()
        self.max_radii2D, self._deformation_table = template["radii"].clone(), template["table"].clone()


def make_template(P, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g)
    t = {}
    for _, attr, shape in GROUPS:
        t[attr] = torch.randn((P,) + shape, generator=g).to(dev)
        t["m" + attr] = (0.01 * torch.randn((P,) + shape, generator=g)).to(dev)
        t["v" + attr] = (1e-4 * u(P, *shape)).to(dev)
    t["_scaling"] = torch.log(0.005 * torch.exp(u(P, 1) * 5.3) * torch.exp(0.25 * (u(P, 3) - 0.5))).to(dev)     # log-uniform 0.005 .. 1
    t["_opacity"] = (-2.0 + 2.0 * torch.randn(P, 1, generator=g)).to(dev)
    t["denom"] = torch.floor(1.0 + u(P, 1) * 11.0).to(dev)
    t["accum"] = (u(P, 1) * (0.0002 / 0.92)).to(dev) * t["denom"]         # mean gradient uniform: 8 % reach 0.0002
    t["radii"] = torch.floor(u(P) * 19.0).to(dev)
    t["table"] = (u(P) < 0.7).to(dev)
    ms = torch.exp(t["_scaling"]).max(dim=1).values
    extent = float(torch.quantile(ms[:1_000_000], 0.625)) / 0.01          # 5 of the 8 % are small enough to clone, 3 split
    min_opacity = float(torch.quantile(torch.sigmoid(t["_opacity"][:1_000_000, 0]), 0.08))
    return t, extent, min_opacity


# ---- the torch-op route ------------------------------------------------------------------------------------------------------------
def _rebind(pc, tensors):
    for name, attr, _ in GROUPS:
        setattr(pc, attr, tensors[name])


def torch_append(pc, new, new_table):
    out = {}
    for group in pc.optimizer.param_groups:
        if len(group["params"]) > 1:
            continue
        old, ext = group["params"][0], new[group["name"]]
        st = pc.optimizer.state.get(old, None)
        fresh = nn.Parameter(torch.cat((old, ext), dim=0).requires_grad_(True))
        if st is not None:
            st["exp_avg"] = torch.cat((st["exp_avg"], torch.zeros_like(ext)), dim=0)
            st["exp_avg_sq"] = torch.cat((st["exp_avg_sq"], torch.zeros_like(ext)), dim=0)
            del pc.optimizer.state[old]
            pc.optimizer.state[fresh] = st
        group["params"][0] = fresh
        out[group["name"]] = fresh
    _rebind(pc, out)
    n, dev = pc._xyz.shape[0], pc._xyz.device
    pc._deformation_table = torch.cat([pc._deformation_table, new_table], -1)
    pc.xyz_gradient_accum, pc.denom = torch.zeros((n, 1), device=dev), torch.zeros((n, 1), device=dev)
    pc.max_radii2D = torch.zeros(n, device=dev)


def torch_remove(pc, drop):
    keep = ~drop
    out = {}
    for group in pc.optimizer.param_groups:
        if len(group["params"]) > 1:
            continue
        old = group["params"][0]
        st = pc.optimizer.state.get(old, None)
        fresh = nn.Parameter(old[keep].requires_grad_(True))
        if st is not None:
            st["exp_avg"], st["exp_avg_sq"] = st["exp_avg"][keep], st["exp_avg_sq"][keep]
            del pc.optimizer.state[old]
            pc.optimizer.state[fresh] = st
        group["params"][0] = fresh
        out[group["name"]] = fresh
    _rebind(pc, out)
    pc.xyz_gradient_accum, pc.denom = pc.xyz_gradient_accum[keep], pc.denom[keep]
    pc._deformation_table, pc.max_radii2D = pc._deformation_table[keep], pc.max_radii2D[keep]


def _rotation_matrices(q):
    q = q / torch.sqrt((q * q).sum(dim=1, keepdim=True))
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).view(-1, 3, 3)


@torch.no_grad()
def torch_event(pc, max_grad, min_opacity, extent, max_screen_size):
    grads = pc.xyz_gradient_accum / pc.denom
    grads[grads.isnan()] = 0.0
    attrs = {name: attr for name, attr, _ in GROUPS}
    # clone
    sel = (torch.norm(grads, dim=-1) >= max_grad) & (torch.exp(pc._scaling).max(dim=1).values <= pc.percent_dense * extent)
    torch_append(pc, {n: getattr(pc, a)[sel] for n, a in attrs.items()}, pc._deformation_table[sel])
    # split
    P = pc._xyz.shape[0]
    padded = torch.zeros(P, device=pc._xyz.device)
    padded[:grads.shape[0]] = grads.squeeze()
    sel = (padded >= max_grad) & (torch.exp(pc._scaling).max(dim=1).values > pc.percent_dense * extent)
    if sel.any():
        stds = torch.exp(pc._scaling[sel]).repeat(2, 1)
        samples = torch.normal(mean=torch.zeros_like(stds), std=stds)
        rots = _rotation_matrices(pc._rotation[sel]).repeat(2, 1, 1)
        new = {n: getattr(pc, a)[sel].repeat(2, *([1] * (getattr(pc, a).dim() - 1))) for n, a in attrs.items()}
        new["xyz"] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + pc._xyz[sel].repeat(2, 1)
        new["scaling"] = torch.log(torch.exp(pc._scaling[sel]).repeat(2, 1) / 1.6)
        n_new = 2 * int(sel.sum())
        torch_append(pc, new, pc._deformation_table[sel].repeat(2))
        torch_remove(pc, torch.cat((sel, torch.zeros(n_new, device=sel.device, dtype=torch.bool))))
    # prune
    drop = (torch.sigmoid(pc._opacity) < min_opacity).squeeze()
    if max_screen_size:
        drop = drop | (pc.max_radii2D > max_screen_size) | (torch.exp(pc._scaling).max(dim=1).values > 0.1 * extent)
    torch_remove(pc, drop)


def native_event(pc, max_grad, min_opacity, extent, max_screen_size):
    from s3gaussian_amd import density
    a = density.densify(pc, max_grad, extent, seed=1)
    b = density.prune(pc, min_opacity, extent, max_screen_size)
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_200_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "density_control_ab.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("density_ab.py measures on the GPU; there is none here (nothing measured)")
    dev = torch.device("cuda:0")
    P = args.points
    template, extent, min_opacity = make_template(P, dev)
    max_grad = 0.0002
    times = {"native": [], "torch": []}
    sizes = {}
    counts = None
    for rep in range(args.warmup + args.reps):
        for route in ("native", "torch"):
            pc = Model(template)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if route == "native":
                counts = native_event(pc, max_grad, min_opacity, extent, None)
            else:
                torch_event(pc, max_grad, min_opacity, extent, None)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if rep >= args.warmup:
                times[route].append(dt)
            sizes[route] = pc._xyz.shape[0]
            del pc
    per_row = sum(4 * 3 * int(torch.tensor(shape).prod()) for _, _, shape in GROUPS)      # parameter + two moments, fp32
    moved = 2 * per_row * P              # every row read once and written once
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = [
        f"# tools/density_ab.py --points {P} --reps {args.reps}: one densify + prune event, native route vs torch-op route, alternated,",
        f"# each event on a fresh copy of the same model, a device synchronise on both sides of the host clock.  {torch.cuda.get_device_name(0)}",
        f"model: P = {P}, SH degree 3, Adam moments present ({per_row} B per Gaussian); native counts: densify {counts[0]}, prune {counts[1]}",
        f"P after the event: native {sizes['native']}, torch {sizes['torch']}",
    ]
    for k in ("native", "torch"):
        v = times[k]
        lines.append(f"{k:6s} ms per event: median {med[k]:.3f}  min {min(v):.3f}  max {max(v):.3f}  all " + " ".join(f"{x:.3f}" for x in v))
    lines.append(f"torch / native (medians): {med['torch'] / med['native']:.2f} x")
    lines.append(f"moved bytes (2 x {per_row} B x P, from the shapes): {moved / 1e9:.3f} GB -> {moved / 1e9 / (med['native'] * 1e-3):.0f} GB/s "
                 f"over the native event (whole event: launches, host reads, allocation and optimizer surgery included).  densify and "
                 f"prune are two passes here, so the device traffic is about twice that figure: "
                 f"{2 * moved / 1e9 / (med['native'] * 1e-3):.0f} GB/s")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")
    if med["native"] > med["torch"]:
        raise SystemExit("the native event is SLOWER than the torch route")


if __name__ == "__main__":
    main()
