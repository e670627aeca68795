"""CPU-only: the formulae of the camera gradients and of the pose map, without a GPU.

  * tests/pose_ref.py::camera_terms_ref -- the restatement the GPU tests hold the kernel to -- fed with the fp32 per-Gaussian
    gradients of the CPU oracle's backward (internals included), against float64 autograd of oracle/torch_ref.rasterize with
    respect to viewmatrix, projmatrix and campos.  Bar, per block (view, proj, campos): the error relative to the block's
    float64 sum of |term| is at most 4 x the relative error the same oracle run's dL_dmeans3D shows against the same autograd
    (the same fp32 intermediates feed both; 4 x is the project's margin).  `python -m tests.test_camera_grad_cpu` writes the
    measured values into profiles/pose_errors.json.
  * tests/pose_ref.py::pose_map_ref: identity at delta = 0, its autograd derivative against the closed-form generators at zero
    and against central differences in float64 elsewhere, the series and the closed form of Rodrigues' coefficients agreeing
    where they meet.  (The kernels are pinned to this restatement at 1e-12 on the GPU: tests/test_camera_grad_gpu.py.)
  * the refusals, by name.

The restatement and pose-map tests pin the REFERENCE the GPU tests lean on, not the library: they exercise tests/pose_ref.py only
and would pass without the feature.  The tests that need the feature here are the refusals, the PoseRefiner surface and the ABI
exports; on the GPU, every test of tests/test_camera_grad_gpu.py and tests/test_pose_route_gpu.py.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests.pose_ref import BLOCKS, UNUSED, camera_terms_ref, pose_map_ref
from tests.util import cam_kwargs, oracle_forward, rel_l2, tiny_scene, to_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, P = 40, 24, 300          # neither a multiple of 16
SEEDS = {"sh": 3, "precomp": 5}


def camera_scene(seed, P=P, W=W, H=H, **over):
    """tiny_scene with Gaussians behind the camera (z from -1) and beyond the 1.3 * tan(fov) clamp (wide spread, large scales so
    that some of those still reach the image), and a camera that is neither at the origin nor axis-aligned."""
    from s3gaussian_amd import synth
    s = tiny_scene(P=P, W=W, H=H, seed=seed, **{**dict(scale=0.35, spread=3.4, zmin=-1.0, zmax=6.0), **over})
    a, b = 0.21, -0.13
    Ry = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    fov = math.radians(60)
    s["cam"] = synth.make_camera(Ry @ Rx, np.array([0.3, -0.2, 0.4]), fov, 2 * math.atan(math.tan(fov / 2) * H / W), W, H)
    # the C ABI carries the field of view as fp32: every party gets those values
    s["cam"]["tanfovx"] = float(np.float32(s["cam"]["tanfovx"]))
    s["cam"]["tanfovy"] = float(np.float32(s["cam"]["tanfovy"]))
    return s


def upstream(seed, H=H, W=W):
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randn(3, H, W, generator=g, dtype=torch.float64), torch.randn(1, H, W, generator=g, dtype=torch.float64)


def autograd_truth(s, mode, gc, gd, sh_degree=3):
    """float64 autograd of torch_ref.rasterize: d loss / d (viewmatrix, projmatrix, campos, means3D); loss = <color, gc> + <depth, gd>."""
    from oracle import torch_ref
    d = lambda t: t.detach().to(torch.float64)
    cam = s["cam"]
    view = d(cam["viewmatrix"]).requires_grad_(True)
    proj = d(cam["projmatrix"]).requires_grad_(True)
    campos = d(cam["campos"]).requires_grad_(True)
    m3 = d(s["means3D"]).requires_grad_(True)
    kw = dict(bg=d(s["bg"]), means3D=m3, opacities=d(s["opacities"]), viewmatrix=view, projmatrix=proj, campos=campos,
              tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], image_height=cam["image_height"], image_width=cam["image_width"],
              scales=d(s["scales"]), rotations=d(s["rotations"]))
    if mode == "sh":
        kw.update(shs=d(s["shs"]), sh_degree=sh_degree)
    else:
        kw.update(colors_precomp=d(s["colors_precomp"]))
    color, radii, depth = torch_ref.rasterize(**kw)
    loss = (color * gc).sum() + (depth * gd).sum()
    gv, gp, gcam, gm = torch.autograd.grad(loss, (view, proj, campos, m3), allow_unused=True)
    z = lambda g, like: torch.zeros_like(like) if g is None else g
    g35 = torch.cat([z(gv, view).reshape(-1), z(gp, proj).reshape(-1), z(gcam, campos).reshape(-1)]).numpy()
    return g35, gm.numpy(), radii.numpy()


def block_errors(got35, want35, abs35):
    """Per block: ||got - want|| / ||sum of |term| ||, both over the block's outputs."""
    return {name: float(np.linalg.norm(got35[sl] - want35[sl]) / max(np.linalg.norm(abs35[sl]), 1e-300)) for name, sl in BLOCKS.items()}


def measure(mode, seed):
    from oracle.oracle import RasterOracle
    s = camera_scene(seed)
    gc, gd = upstream(seed)
    orc = RasterOracle(np.float32)
    fwd = oracle_forward(orc, s, mode=mode, sh_degree=3)
    rb = orc.backward(fwd, gc.numpy(), gd.numpy())
    cam = to_np(cam_kwargs(s))
    sums, abs_sums = camera_terms_ref(
        P=P, means3D=s["means3D"].numpy(), radii=fwd["radii"], cov3D=fwd["state"]["cov3D"][:P], clamped=fwd["state"]["clamped"][:3 * P],
        viewmatrix=cam["viewmatrix"], projmatrix=cam["projmatrix"], campos=cam["campos"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
        image_height=H, image_width=W, dL_dmeans2D=rb["dL_dmeans2D"], dL_dconic=rb["dL_dconic"], dL_ddepths=rb["dL_ddepths"],
        dL_dcolors=rb["dL_dcolors"], shs=s["shs"].numpy() if mode == "sh" else None, sh_degree=3 if mode == "sh" else 0)
    truth, truth_m3, radii64 = autograd_truth(s, mode, gc, gd)
    # what the scene exercises
    view = cam["viewmatrix"].astype(np.float64)
    m = s["means3D"].numpy().astype(np.float64)
    t = m @ view[:3, :3] + view[3, :3]
    vis = fwd["radii"] > 0
    clamp = vis & ((np.abs(t[:, 0] / t[:, 2]) > 1.3 * cam["tanfovx"]) | (np.abs(t[:, 1] / t[:, 2]) > 1.3 * cam["tanfovy"]))
    return dict(mode=mode, seed=seed, visible=int(vis.sum()), behind=int((t[:, 2] <= 0.2).sum()), visible_on_clamp=int(clamp.sum()),
                radii_agree=bool((radii64 == fwd["radii"]).all()), means3D_rel=rel_l2(rb["dL_dmeans3D"], truth_m3),
                blocks=block_errors(sums, truth, abs_sums), sums=sums, truth=truth, abs_sums=abs_sums)


@pytest.mark.parametrize("mode", ["sh", "precomp"])
def test_restatement_matches_float64_autograd(mode):
    r = measure(mode, SEEDS[mode])
    print({k: v for k, v in r.items() if k not in ("sums", "truth", "abs_sums")})
    assert r["radii_agree"] and r["visible"] > 50 and r["behind"] > 5 and r["visible_on_clamp"] > 0
    assert math.isfinite(r["means3D_rel"]) and r["means3D_rel"] > 0
    for name, err in r["blocks"].items():
        if name == "campos" and mode == "precomp":
            assert not r["sums"][BLOCKS[name]].any() and not r["truth"][BLOCKS[name]].any()   # the camera centre enters nothing
            continue
        assert err <= 4 * r["means3D_rel"], (name, err, r["means3D_rel"])
    assert float(np.abs(r["truth"][BLOCKS["view"]]).max()) > 0 and float(np.abs(r["truth"][BLOCKS["proj"]]).max()) > 0
    for j in UNUSED:
        assert r["sums"][j] == 0.0 and r["truth"][j] == 0.0


def test_dropped_pieces_and_g_dir():
    """A None gradient array drops its terms; g_dir alone gives minus its column sums on campos and nothing else."""
    rng = np.random.default_rng(0)
    g = rng.standard_normal((7, 3)).astype(np.float32)
    sums, abs_sums = camera_terms_ref(P=7, g_dir=g)
    assert np.array_equal(sums[32:35], -g.astype(np.float64).sum(0)) and not sums[:32].any()
    assert np.array_equal(abs_sums[32:35], np.abs(g.astype(np.float64)).sum(0))
    sums, _ = camera_terms_ref(P=0)
    assert sums.shape == (35,) and not sums.any()


# ---- pose map ---------------------------------------------------------------------------------------------------------------------
def _camera():
    s = camera_scene(0)
    return s["cam"]


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


POSE_CASES = [np.zeros(6), np.r_[1e-9 * _unit([1, -2, 0.5]), 0.0, 0.0, 0.0], np.r_[1e-4 * _unit([0.3, 1, -1]), 0.01, -0.02, 0.03],
              np.r_[0.3 * _unit([1, 1, -0.5]), 0.2, -0.1, 0.05]]


def _pose_jacobian(delta, cam):
    d = torch.tensor(delta, dtype=torch.float64, requires_grad=True)
    out = torch.cat([o.reshape(-1) for o in pose_map_ref(d, cam["viewmatrix"], cam["projmatrix"])])
    return torch.stack([torch.autograd.grad(out[j], d, retain_graph=True)[0] for j in range(35)]).numpy(), out.detach().numpy()


def test_pose_map_is_the_identity_at_zero_and_states_its_rounding():
    cam = _camera()
    view, proj, campos = pose_map_ref(torch.zeros(6, dtype=torch.float64), cam["viewmatrix"], cam["projmatrix"])
    assert torch.equal(view, cam["viewmatrix"].double())                      # view0 D^T with D = I: exact
    # proj' = view0 (view0^-1 proj0): the rigid inverse of an fp32 rotation is not its exact inverse; measured 2.2e-8 here
    diff = float((proj - cam["projmatrix"].double()).abs().max())
    print("proj' - projmatrix at delta = 0:", diff)
    assert diff <= 4 * 2.0 ** -24 * float(cam["projmatrix"].abs().max()) * 4  # a few fp32 roundings of the largest entry
    assert float((campos - cam["campos"].double()).abs().max()) <= 8 * 2.0 ** -24 * max(1.0, float(cam["campos"].abs().max()))


def test_pose_map_derivative_at_zero_is_the_generators():
    """d view'/d omega_a at 0 = view0 K_a^T (K_a the generator of rotations about axis a), d view'/d tau_c = column 3 of view0 into
    column c: finite and exact although theta = 0."""
    cam = _camera()
    J, _ = _pose_jacobian(np.zeros(6), cam)
    A0 = cam["viewmatrix"].double().numpy()
    for a in range(3):
        K = np.zeros((3, 3))
        K[(a + 2) % 3, (a + 1) % 3], K[(a + 1) % 3, (a + 2) % 3] = 1.0, -1.0      # skew of e_a
        D = np.zeros((4, 4))
        D[:3, :3] = K
        assert np.abs(J[:16, a].reshape(4, 4) - A0 @ D.T).max() <= 1e-15
        D = np.zeros((4, 4))
        D[a, 3] = 1.0
        assert np.abs(J[:16, 3 + a].reshape(4, 4) - A0 @ D.T).max() <= 1e-15
    assert np.isfinite(J).all()


@pytest.mark.parametrize("case", range(len(POSE_CASES)))
def test_pose_map_derivative_against_central_differences(case):
    cam = _camera()
    delta = POSE_CASES[case]
    J, _ = _pose_jacobian(delta, cam)
    h = 1e-6
    for k in range(6):
        e = np.zeros(6)
        e[k] = h
        f = lambda d: torch.cat([o.reshape(-1) for o in pose_map_ref(torch.tensor(d, dtype=torch.float64), cam["viewmatrix"],
                                                                      cam["projmatrix"])]).numpy()
        fd = (f(delta + e) - f(delta - e)) / (2 * h)
        # central differences in float64: truncation h^2 |f'''| / 6 + rounding eps |f| / h ~ 1e-12 + 1e-9 for |f| <= 10
        assert np.abs(fd - J[:, k]).max() <= 1e-8, (case, k, np.abs(fd - J[:, k]).max())


def test_rodrigues_series_meets_the_closed_form():
    """Just below and just above theta^2 = 1e-4 the two branches give the same map to 1e-14."""
    cam = _camera()
    u = _unit([0.4, -1.0, 0.7])
    lo = np.r_[math.sqrt(1e-4) * (1 - 1e-9) * u, 0.1, 0.2, 0.3]
    hi = np.r_[math.sqrt(1e-4) * (1 + 1e-9) * u, 0.1, 0.2, 0.3]
    Jl, fl = _pose_jacobian(lo, cam)
    Jh, fh = _pose_jacobian(hi, cam)
    assert np.abs(fl - fh).max() <= 1e-10 and np.abs(Jl - Jh).max() <= 1e-8     # 1e-11 apart in theta, |f'| and |f''| <= 100


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_multi_view_routes_refuse_a_camera_that_requires_a_gradient():
    from s3gaussian_amd import glue, pipeline
    x = torch.zeros(4, 3)
    campos = torch.zeros(2, 3, requires_grad=True)
    with pytest.raises(RuntimeError, match="activations_and_colors_views: a camera centre requires a gradient"):
        glue.activations_and_colors_views(3, x, x, None, x, campos, x, x, x)
    cam = dict(_camera())
    cam["viewmatrix"] = cam["viewmatrix"].clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="render_views: a camera requires a gradient"):
        pipeline.render_views([cam], None, None, None)


def test_pose_refiner_is_refused_under_data_parallel(monkeypatch):
    from s3gaussian_amd import dp, pipeline, pose
    monkeypatch.setattr(dp, "active", lambda: True)
    with pytest.raises(RuntimeError, match="PoseRefiner: pose refinement under the data-parallel wrapper"):
        pose.PoseRefiner(3, "cpu", lr=1e-3)
    with pytest.raises(RuntimeError, match=r"training_step\(pose=...\): pose refinement under the data-parallel wrapper"):
        pipeline.training_step(None, {}, None, None, None, None, None, None, pose=object(), cam_index=0)


def test_pose_refiner_has_no_default_learning_rate_and_no_cpu_route():
    from s3gaussian_amd import pose
    with pytest.raises(TypeError):
        pose.PoseRefiner(3, "cpu")
    r = pose.PoseRefiner(3, "cpu", lr=1e-3)
    assert r.delta.dtype == torch.float64 and r.delta.shape == (3, 6) and not r.delta.detach().any()
    assert isinstance(r.optimizer, torch.optim.Adam)
    with pytest.raises(RuntimeError, match="GPU"):
        r.corrected(_camera(), 0)
    with pytest.raises(RuntimeError, match="cam_index"):
        from s3gaussian_amd import pipeline
        pipeline.render(_camera(), None, None, None, pose=r)


def test_abi_exports_the_camera_entry_points():
    from s3gaussian_amd import _lib
    L = _lib.lib()
    for name in ("s3g_camera_backward_workspace_bytes", "s3g_camera_backward", "s3g_pose_apply", "s3g_pose_apply_backward"):
        assert hasattr(L, name) and name in _lib.EXPORTED_SYMBOLS
    assert L.s3g_abi_version() == _lib.ABI_VERSION
    # one partial of 27 doubles per workgroup of 256 Gaussians, at most 512 workgroups, rounded up to 128 bytes
    assert [L.s3g_camera_backward_workspace_bytes(p) for p in (0, 1, 256, 257, 131072, 10 ** 7)] == [0, 256, 256, 512, 110592, 110592]
    # argument checks come before any device call
    assert L.s3g_camera_backward(None, None, None, None, None, None, None, None, None, None, None) == 1
    assert b"s3g_camera_backward: NULL inputs" in L.s3g_last_error()
    assert L.s3g_pose_apply(None, None, None, None, None, None, None) == 1 and b"s3g_pose_apply" in L.s3g_last_error()


if __name__ == "__main__":      # python -m tests.test_camera_grad_cpu: the CPU part of profiles/pose_errors.json
    path = os.path.join(ROOT, "profiles", "pose_errors.json")
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc["restatement_vs_float64_autograd"] = [
        {k: v for k, v in measure(mode, seed).items() if k not in ("sums", "truth", "abs_sums")} for mode, seed in SEEDS.items()]
    cam = _camera()
    _, proj, _ = pose_map_ref(torch.zeros(6, dtype=torch.float64), cam["viewmatrix"], cam["projmatrix"])
    doc["proj_at_zero_delta_max_abs_difference"] = float((proj - cam["projmatrix"].double()).abs().max())
    json.dump(doc, open(path, "w"), indent=1)
    print(json.dumps(doc, indent=1))
