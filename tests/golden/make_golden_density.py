"""Generate tests/golden/density_control.npz by RUNNING THE REFERENCE'S OWN `GaussianModel.densify`, `prune` and `reset_opacity`
(scene/gaussian_model.py:350-353, 412-522, 661-678) on CPU tensors in the build container.  /root/reference is only ever imported
here, never copied; without it this script refuses to run.

    python tests/golden/make_golden_density.py        # rewrites density_control.npz next to this file

How the reference's methods run without a GPU:
  1. `scene.gaussian_model` is imported with the stub finder of oracle/ref_py.py standing in for the packages the image lacks;
  2. the name `torch` inside `scene.gaussian_model` and `utils.general_utils` is a proxy whose `zeros` drops `device="cuda"` and
     whose `normal(mean, std)` returns `mean + std * z` for a recorded `z = randn` (so the deviates can be replayed on the GPU);
  3. the model is `GaussianModel.__new__` + plain attributes + a torch.optim.Adam that has taken one step.

Stored: the DECISION inputs only (xyz, scaling, rotation, opacity, accum, denom, max_radii2D, table, scalars), the recorded z, the
source row and kind of every output row of densify, the children's xyz / scaling, the kept index of prune with max_screen_size = 20
and None, the reset opacities -- and, per computed quantity, the same formula evaluated in float64 with ref_err = max |reference
fp32 - float64|.  Features and moments are not stored: in the reference's run they carry their row number, which is how the source
rows are read back; the tests fill them with row-coded values of their own and check the gather through the stored source rows.

The generator ASSERTS that no decision quantity lies within 4 fp32 ulp of its threshold (device exp / sigmoid may then differ from
the CPU's without changing a class) and that every class holds between 1 % and 30 % of P.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "density_control.npz")

P = 4096
EXTENT = 5.0
PERCENT_DENSE = 0.01
MAX_GRAD = 0.0002
MIN_OPACITY = 0.005
MAX_SCREEN = 20
KIND_ORIGINAL, KIND_CLONE, KIND_CHILD1, KIND_CHILD2 = 0, 1, 2, 3
ULP_GAP = 4


def reference_present() -> bool:
    return os.path.isfile(os.path.join(REF, "scene", "gaussian_model.py"))


class _TorchProxy(types.ModuleType):
    """`torch` as the two reference modules see it on a machine without a GPU."""

    def __init__(self, recorded):
        super().__init__("torch")
        self._recorded = recorded

    def __getattr__(self, name):
        return getattr(torch, name)

    def zeros(self, *a, **k):
        k.pop("device", None)
        return torch.zeros(*a, **k)

    def normal(self, mean, std):
        z = torch.randn(std.shape, generator=self._recorded["generator"])
        self._recorded["z"].append(z.clone())
        return mean + std * z


def _import_reference(recorded):
    """-> (GaussianModel class, cleanup()).  Nothing of what is imported here stays in sys.modules afterwards."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from oracle import ref_py
    before = set(sys.modules)
    finder = ref_py._StubFinder([n for n in ref_py.STUBBED if ref_py._missing(n)])
    sys.meta_path.append(finder)
    for pkg in ("scene", "utils"):       # package objects that do not execute the reference's __init__.py (dataset readers)
        m = types.ModuleType(pkg)
        m.__path__ = [os.path.join(REF, pkg)]
        sys.modules[pkg] = m
    sys.path.insert(0, REF)

    def cleanup():
        for name in set(sys.modules) - before:
            del sys.modules[name]
        if finder in sys.meta_path:
            sys.meta_path.remove(finder)
        if REF in sys.path:
            sys.path.remove(REF)

    try:
        gm = importlib.import_module("scene.gaussian_model")
        gu = importlib.import_module("utils.general_utils")
        proxy = _TorchProxy(recorded)
        gm.torch = proxy
        gu.torch = proxy
    except Exception:
        cleanup()
        raise
    return gm.GaussianModel, cleanup


def make_inputs():
    """Seeded decision inputs: uniform gradients, log-uniform scales, normal opacity logits; some rows never seen (denom == 0)."""
    g = torch.Generator().manual_seed(20240611)
    u = lambda *s: torch.rand(*s, generator=g)
    xyz = (u(P, 3) - 0.5) * 40.0
    base = torch.exp(np.log(0.005) + u(P, 1) * (np.log(1.0) - np.log(0.005)))
    scaling = torch.log(base * torch.exp(0.25 * (u(P, 3) - 0.5)))
    rotation = torch.randn(P, 4, generator=g)
    opacity = -2.0 + 2.0 * torch.randn(P, 1, generator=g)
    denom = torch.floor(u(P, 1) * 12.0)                       # 0 .. 11 views; ~8 % of the rows were never visible
    accum = u(P, 1) * 0.00031 * denom                         # mean viewspace gradient uniform in [0, 0.00031)
    radii = torch.floor(u(P) * 22.0)
    radii = torch.where(radii == float(MAX_SCREEN), radii + 1.0, radii)      # 0 .. 22 without the threshold itself
    table = u(P) < 0.7
    return dict(xyz=xyz, scaling=scaling, rotation=rotation, opacity=opacity, accum=accum, denom=denom, max_radii2D=radii, table=table)


def _ulps(a: torch.Tensor, t: float) -> torch.Tensor:
    """fp32 ulp distance between the (positive or zero) values of `a` and the threshold as the comparison sees it, fp32(t)."""
    ai = a.contiguous().view(torch.int32).to(torch.int64)
    ti = int(np.float32(t).view(np.int32))
    d = (ai - ti).abs()
    return torch.where(torch.isfinite(a), d, torch.full_like(d, 1 << 40))


def decision_quantities(inp):
    """The five compared quantities, evaluated by torch on the CPU exactly as the reference evaluates them, with their thresholds."""
    g = inp["accum"] / inp["denom"]
    g[g.isnan()] = 0.0
    ms = torch.exp(inp["scaling"]).max(dim=1).values
    op = torch.sigmoid(inp["opacity"]).squeeze(1)
    return [("grad", g.squeeze(1), MAX_GRAD), ("scale_dense", ms, PERCENT_DENSE * EXTENT), ("opacity", op, MIN_OPACITY),
            ("screen", inp["max_radii2D"], float(MAX_SCREEN)), ("scale_world", ms, 0.1 * EXTENT)]


def no_near_ties(inp) -> bool:
    return all(int(_ulps(q, t).min()) > ULP_GAP for _, q, t in decision_quantities(inp))


def class_shares(inp):
    q = {n: (v, t) for n, v, t in decision_quantities(inp)}
    sel = q["grad"][0] >= np.float32(q["grad"][1])
    small = q["scale_dense"][0] <= np.float32(q["scale_dense"][1])
    drop_none = q["opacity"][0] < np.float32(q["opacity"][1])
    drop_screen = drop_none | (q["screen"][0] > q["screen"][1]) | (q["scale_world"][0] > np.float32(q["scale_world"][1]))
    return dict(clone=float((sel & small).float().mean()), split=float((sel & ~small).float().mean()),
                prune_none=float(drop_none.float().mean()), prune_screen=float(drop_screen.float().mean()))


def _model(GaussianModel, inp):
    """GaussianModel.__new__ + plain attributes + an Adam that has stepped once.  Row numbers ride in the features."""
    m = GaussianModel.__new__(GaussianModel)
    m.setup_functions()
    rows = torch.arange(P, dtype=torch.float32)
    par = lambda t: torch.nn.Parameter(t.clone().requires_grad_(True))
    m._xyz, m._scaling, m._rotation, m._opacity = par(inp["xyz"]), par(inp["scaling"]), par(inp["rotation"]), par(inp["opacity"])
    m._features_dc = par(rows[:, None, None].repeat(1, 1, 3))
    m._features_rest = par(rows[:, None, None].repeat(1, 15, 3))
    m._deformation_table = inp["table"].clone()
    m._deformation_accum = torch.zeros(P, 3)
    m.xyz_gradient_accum, m.denom, m.max_radii2D = inp["accum"].clone(), inp["denom"].clone(), inp["max_radii2D"].clone()
    m.percent_dense = PERCENT_DENSE
    groups = [{"params": [getattr(m, a)], "lr": 1e-3, "name": n} for n, a in
              (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("opacity", "_opacity"),
               ("scaling", "_scaling"), ("rotation", "_rotation"))]
    m.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
    for grp in groups:
        p = grp["params"][0]
        p.grad = torch.zeros_like(p)           # a step with zero gradients: moments and `step` exist, the parameters do not move
    m.optimizer.step()
    m.optimizer.zero_grad(set_to_none=True)
    return m


def children_float64(inp, src, z):
    """xyz' = R(q / |q|) (exp(s) o z) + xyz and s' = log(exp(s) / 1.6) in float64 from the fp32 inputs, for child rows `src`."""
    s = inp["scaling"].double()[src]
    q = inp["rotation"].double()[src]
    q = q / q.norm(dim=1, keepdim=True)
    r, x, y, zz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([1 - 2 * (y * y + zz * zz), 2 * (x * y - r * zz), 2 * (x * zz + r * y),
                     2 * (x * y + r * zz), 1 - 2 * (x * x + zz * zz), 2 * (y * zz - r * x),
                     2 * (x * zz - r * y), 2 * (y * zz + r * x), 1 - 2 * (x * x + y * y)], dim=1).view(-1, 3, 3)
    xyz = torch.bmm(R, (torch.exp(s) * z.double()).unsqueeze(-1)).squeeze(-1) + inp["xyz"].double()[src]
    return xyz, torch.log(torch.exp(s) / 1.6)


def reset_float64(inp):
    y = torch.minimum(torch.sigmoid(inp["opacity"].double()), torch.tensor(float(np.float32(0.01)), dtype=torch.float64))
    return torch.log(y / (1 - y))


def generate():
    """-> dict of numpy arrays (what density_control.npz holds)."""
    if not reference_present():
        raise SystemExit(f"{REF} is not here: this generator runs the reference's own code and cannot run without it")
    recorded = {"z": [], "generator": torch.Generator().manual_seed(77)}
    GaussianModel, cleanup = _import_reference(recorded)
    try:
        inp = make_inputs()
        assert no_near_ties(inp), "a decision quantity lies within 4 ulp of its threshold: change the seed"
        shares = class_shares(inp)
        assert all(0.01 <= v <= 0.30 for v in shares.values()), shares
        with torch.no_grad():
            # ---- densify ----
            m = _model(GaussianModel, inp)
            step_before = float(m.optimizer.state[m._xyz]["step"])
            m.densify(MAX_GRAD, MIN_OPACITY, EXTENT, None, 5, 5, None, 1000, "fine")
            assert len(recorded["z"]) == 1
            z = recorded["z"][0]
            src = m._features_dc[:, 0, 0].long()
            assert torch.equal(m._features_rest[:, 7, 1].long(), src)
            down = torch.nonzero(src[1:] <= src[:-1]).squeeze(1) + 1       # four ascending segments: three descents
            assert down.numel() == 3, down
            kind = torch.zeros_like(src)
            for k, b in enumerate(down.tolist()):
                kind[b:] = k + 1
            n_split = int((kind == KIND_CHILD1).sum())
            assert torch.equal(src[kind == KIND_CHILD1], src[kind == KIND_CHILD2]) and z.shape == (2 * n_split, 3)
            assert float(m.optimizer.state[m._xyz]["step"]) == step_before
            child = kind >= KIND_CHILD1
            child_xyz, child_scaling = m._xyz[child].detach().clone(), m._scaling[child].detach().clone()
            xyz64, scaling64 = children_float64(inp, src[child], z)
            assert float(m.xyz_gradient_accum.abs().max()) == 0 and m.max_radii2D.shape[0] == src.shape[0]
            # ---- prune, both cases, each on the untouched inputs ----
            kept = {}
            for tag, screen in (("screen", MAX_SCREEN), ("none", None)):
                m = _model(GaussianModel, inp)
                m.prune(MAX_GRAD, MIN_OPACITY, EXTENT, screen)
                kept[tag] = m._features_dc[:, 0, 0].long()
                assert torch.equal(m.denom, inp["denom"][kept[tag]])
            # ---- reset_opacity ----
            m = _model(GaussianModel, inp)
            m.reset_opacity()
            reset = m._opacity.detach().clone()
            assert float(m.optimizer.state[m._opacity]["exp_avg"].abs().max()) == 0
            reset64 = reset_float64(inp)
    finally:
        cleanup()
    n = lambda t: t.detach().cpu().numpy()
    out = {k: n(v) for k, v in inp.items()}
    out.update(
        P=np.int64(P), extent=np.float64(EXTENT), percent_dense=np.float64(PERCENT_DENSE), max_grad=np.float64(MAX_GRAD),
        min_opacity=np.float64(MIN_OPACITY), max_screen_size=np.int64(MAX_SCREEN), no_near_ties=np.bool_(True), ulp_gap=np.int64(ULP_GAP),
        share_clone=np.float64(shares["clone"]), share_split=np.float64(shares["split"]),
        share_prune_none=np.float64(shares["prune_none"]), share_prune_screen=np.float64(shares["prune_screen"]),
        z=n(z), densify_src=n(src).astype(np.int32), densify_kind=n(kind).astype(np.uint8),
        child_xyz=n(child_xyz), child_scaling=n(child_scaling), child_xyz_f64=n(xyz64), child_scaling_f64=n(scaling64),
        ref_err_xyz=np.float64((child_xyz.double() - xyz64).abs().max()),
        ref_err_scaling=np.float64((child_scaling.double() - scaling64).abs().max()),
        prune_kept_screen=n(kept["screen"]).astype(np.int32), prune_kept_none=n(kept["none"]).astype(np.int32),
        reset_opacity=n(reset), reset_opacity_f64=n(reset64), ref_err_reset=np.float64((reset.double() - reset64).abs().max()))
    return out


if __name__ == "__main__":
    arrays = generate()
    np.savez_compressed(OUT, **arrays)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes; P {P} -> {arrays['densify_src'].shape[0]} after densify "
          f"({int((arrays['densify_kind'] == 1).sum())} clones, {int((arrays['densify_kind'] == 2).sum())} splits), "
          f"{arrays['prune_kept_screen'].shape[0]} / {arrays['prune_kept_none'].shape[0]} kept by prune(20) / prune(None); "
          f"ref_err xyz {arrays['ref_err_xyz']:.3g} scaling {arrays['ref_err_scaling']:.3g} reset {arrays['ref_err_reset']:.3g}")
