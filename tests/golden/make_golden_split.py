"""Generate tests/golden/split_pcd.npz by RUNNING THE REFERENCE'S OWN `GaussianModel.save_ply_split`
(scene/gaussian_model.py:277-348) on CPU tensors in the build container.  /root/reference is only ever imported here, never copied;
without it this script refuses to run.

    python tests/golden/make_golden_split.py        # rewrites split_pcd.npz next to this file

How the reference's method runs without a GPU and without `plyfile`:
  1. `scene.gaussian_model` is imported with the stub finder of oracle/ref_py.py standing in for the packages the image lacks;
  2. the names `PlyElement` / `PlyData` inside `scene.gaussian_model` are stand-ins: `PlyElement.describe(array, "vertex")` keeps
     the structured array it is handed -- that array IS the data the reference writes -- and `PlyData([el]).write(path)` records it
     under the path instead of encoding it;
  3. the model is `GaussianModel.__new__` + plain attributes; the two paths point into a temporary directory.

Stored: the inputs (xyz, f_dc, f_rest, opacity, scaling, rotation, dx = dx_list[24]), both recorded tables as [n, 62] float32 with
their attribute names, the reference's mask (recomputed by its own three lines, and checked against the recorded row counts), its
fp32 `thre`, and the float64 mean of the fp32 maxima.

The generator ASSERTS that no max|dx_i| lies within a relative 1e-5 of thre (a threshold that differs in its last bits -- torch's
fp32 mean against the float64 mean rounded once -- then moves no point) and that the dynamic class holds between 5 % and 50 % of P;
it reseeds until both hold.
"""
import importlib
import os
import sys
import tempfile
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "split_pcd.npz")

P = 1000                 # not a multiple of 64 or 256
SH_DEGREE = 3
R = (SH_DEGREE + 1) ** 2 - 1
N_DX = 25                # the reference reads dx_list[24]
TIE_GAP = 1e-5
FIRST_SEED = 20240917


def reference_present() -> bool:
    return os.path.isfile(os.path.join(REF, "scene", "gaussian_model.py"))


class _Element:
    def __init__(self, data, name):
        self.data, self.name = data, name


class _PlyElement:
    @staticmethod
    def describe(data, name, *a, **k):
        assert isinstance(data, np.ndarray) and data.dtype.names is not None
        return _Element(data, name)


def _import_reference(written):
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

    class _PlyData:
        def __init__(self, elements, *a, **k):
            (self.element,) = elements

        def write(self, path):
            assert self.element.name == "vertex"
            written[path] = self.element.data

    try:
        gm = importlib.import_module("scene.gaussian_model")
        gm.PlyElement, gm.PlyData = _PlyElement, _PlyData
    except Exception:
        cleanup()
        raise
    return gm.GaussianModel, cleanup


def make_inputs(seed):
    g = torch.Generator().manual_seed(seed)
    n = lambda *s: torch.randn(*s, generator=g)
    inp = dict(xyz=n(P, 3) * 20.0, f_dc=n(P, 1, 3), f_rest=n(P, R, 3) * 0.2, opacity=n(P, 1) * 2.0 - 1.0, scaling=n(P, 3) * 0.7 - 3.0,
               rotation=n(P, 4))
    mag = torch.exp(1.5 * n(P, 1)) * 0.02                                   # log-normal magnitudes: a heavy tail of movers
    inp["dx"] = mag * (torch.rand(P, 3, generator=g) * 2.0 - 1.0)
    return inp


def reference_mask(dx):
    """The reference's three lines (scene/gaussian_model.py:291-295) on the CPU tensor."""
    max_values = torch.max(torch.abs(dx), dim=1)[0]
    thre = torch.mean(max_values)
    return max_values > thre, thre, max_values


def conditions(inp):
    mask, thre, m = reference_mask(inp["dx"])
    t = float(thre)
    tie_free = bool(((m.double() - t).abs() > TIE_GAP * abs(t)).all())
    share = float(mask.float().mean())
    return tie_free and 0.05 <= share <= 0.50, share


def _rows(structured):
    return np.ascontiguousarray(np.stack([structured[n] for n in structured.dtype.names], axis=1), dtype=np.float32)


def generate():
    """-> dict of numpy arrays (what split_pcd.npz holds)."""
    if not reference_present():
        raise SystemExit(f"{REF} is not here: this generator runs the reference's own code and cannot run without it")
    seed = FIRST_SEED
    while True:
        inp = make_inputs(seed)
        ok, share = conditions(inp)
        if ok:
            break
        seed += 1
    written = {}
    GaussianModel, cleanup = _import_reference(written)
    try:
        with torch.no_grad(), tempfile.TemporaryDirectory() as tmp:
            m = GaussianModel.__new__(GaussianModel)
            m._xyz, m._features_dc, m._features_rest = inp["xyz"].clone(), inp["f_dc"].clone(), inp["f_rest"].clone()
            m._opacity, m._scaling, m._rotation = inp["opacity"].clone(), inp["scaling"].clone(), inp["rotation"].clone()
            g = torch.Generator().manual_seed(seed + 1)
            dx_list = [torch.randn(P, 3, generator=g) for _ in range(N_DX)]       # only entry 24 is meaningful
            dx_list[24] = inp["dx"].clone()
            dyn_path, sta_path = os.path.join(tmp, "pcd", "dynamic.ply"), os.path.join(tmp, "pcd", "static.ply")
            names = m.construct_list_of_attributes()
            m.save_ply_split(dyn_path, sta_path, dx_list, None)
            dynamic, static = written[dyn_path], written[sta_path]
            assert list(dynamic.dtype.names) == names and list(static.dtype.names) == names and len(names) == 17 + 3 * R
            assert torch.equal(m._xyz, inp["xyz"] + inp["dx"])                    # the reference's side effect (:289)
    finally:
        cleanup()
    mask, thre, maxima = reference_mask(inp["dx"])
    dynamic_rows, static_rows = _rows(dynamic), _rows(static)
    assert dynamic_rows.shape == (int(mask.sum()), len(names)) and static_rows.shape == (P - int(mask.sum()), len(names))
    out = {k: v.numpy() for k, v in inp.items()}
    out.update(P=np.int64(P), sh_degree=np.int64(SH_DEGREE), dx_index=np.int64(24), seed=np.int64(seed), names=np.array(names),
               dynamic_rows=dynamic_rows, static_rows=static_rows, mask=mask.numpy(), thre=np.float32(float(thre)),
               mean_f64=np.float64(maxima.double().sum().item() / P), tie_gap=np.float64(TIE_GAP), dynamic_share=np.float64(share))
    return out


if __name__ == "__main__":
    arrays = generate()
    np.savez_compressed(OUT, **arrays)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes; seed {int(arrays['seed'])}, {arrays['dynamic_rows'].shape[0]} dynamic + "
          f"{arrays['static_rows'].shape[0]} static rows of {arrays['dynamic_rows'].shape[1]} floats, thre {float(arrays['thre']):.9g} "
          f"(float64 mean {float(arrays['mean_f64']):.17g})")
