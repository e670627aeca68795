"""CPU: pose refinement in the multi-view step -- the float64 restatement the GPU tests compare against, and the refusals.

  * tests/glue_campos_ref.py (dL/dcampos_v = -sum_p t_v[p], term by term as csrc/glue_views.hip forms t_v) against float64
    autograd of oracle/torch_ref._sh_color with respect to campos: 1e-12 relative to sum_p |t_v[p]| per component, degrees 0-3,
    clamped colours included; degree 0 does not depend on the direction: exact zeros.
  * refusals, by name and before anything touches a device: repeated indices and wrong lengths in PoseRefiner.corrected_views,
    cam_indices of the wrong length or without pose, pose= with sky_model=, pose= under an active data-parallel wrapper; and the two
    refusals for cameras that the CALLER made require a gradient still stand (tests/test_camera_grad_cpu.py pins them too).
"""
import pytest
import torch

from tests.glue_campos_ref import campos_grad_autograd, campos_grad_ref
from tests.test_camera_grad_cpu import _camera


def scene(P, seed, deg=3):
    """Coefficients, positions, one camera centre and a colour gradient; a third of the colours sit around the clamp."""
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    shs = torch.cat([mk(P, 1, 3), 0.3 * mk(P, 15, 3)], 1) + 0.1 * mk(P, 16, 3)
    shs[::3, 0] -= 2.5
    return shs, 3 * mk(P, 3), 2.0 * mk(3), mk(P, 3)


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_restatement_against_autograd_of_the_sh_colours(deg):
    shs, xyz, campos, g_colors = scene(2000, 40 + deg)
    want, live = campos_grad_autograd(deg, shs, xyz, campos, g_colors)
    assert bool(live.any()) and bool((~live).any())
    got, abs_sum = campos_grad_ref(deg, shs, xyz, campos, g_colors, live)
    if deg == 0:
        assert not got.any() and not want.any() and not abs_sum.any()
        return
    err = (got - want).abs() / abs_sum
    print("deg", deg, "restatement", got.numpy(), "autograd", want.numpy(), "err / sum|term|", err.numpy())
    assert float(want.abs().min()) > 0 and float(err.max()) <= 1e-12


def _refiner(n=4):
    from s3gaussian_amd import pose
    return pose.PoseRefiner(n, "cpu", lr=1e-3)


def test_corrected_views_refuses_repeated_indices_and_wrong_lengths():
    cam = _camera()
    r = _refiner()
    with pytest.raises(RuntimeError, match="corrected_views: repeated camera indices"):
        r.corrected_views([cam, cam, cam], [0, 2, 0])
    with pytest.raises(RuntimeError, match="corrected_views: 2 cameras, 3 indices"):
        r.corrected_views([cam, cam], [0, 1, 2])
    with pytest.raises(RuntimeError, match="corrected_views: camera indices .* outside 0 .. 3"):
        r.corrected_views([cam, cam], [0, 4])
    assert r.corrected_views([], []) == []


def _step_args(V):
    from s3gaussian_amd import pipeline
    cam = _camera()
    H, W = cam["image_height"], cam["image_width"]
    img = torch.zeros(3, H, W)
    return ([dict(cam) for _ in range(V)], [img] * V, [img[:1]] * V, None, pipeline.default_hyper(), pipeline.default_opt(),
            torch.zeros(3))


@pytest.mark.parametrize("entry", ["render_views", "training_step_views"])
def test_multi_view_routes_refuse_by_name(entry, monkeypatch):
    from s3gaussian_amd import dp, pipeline
    r = _refiner()
    cams, gts, gtd, gtf, hyper, opt, bg = _step_args(3)

    def call(**kw):
        if entry == "render_views":
            return pipeline.render_views(cams, None, pipeline._default_pipe(None), bg, **kw)
        return pipeline.training_step_views(None, cams, gts, gtd, gtf, hyper, opt, bg, **kw)

    with pytest.raises(RuntimeError, match=r"\(pose=\.\.\.\): 2 cam_indices for 3 views"):
        call(pose=r, cam_indices=[0, 1])
    with pytest.raises(RuntimeError, match=r"\(pose=\.\.\.\): cam_indices says which"):
        call(pose=r)
    with pytest.raises(RuntimeError, match=rf"{entry}\(cam_indices=\.\.\.\) without pose="):
        call(cam_indices=[0, 1, 2])
    with pytest.raises(RuntimeError, match=rf"{entry}\(sky_model=\.\.\., pose=\.\.\.\)"):
        call(pose=r, cam_indices=[0, 1, 2], sky_model=object())
    monkeypatch.setattr(dp, "active", lambda: True)
    with pytest.raises(RuntimeError, match=rf"{entry}\(pose=\.\.\.\): pose refinement under the data-parallel wrapper"):
        call(pose=r, cam_indices=[0, 1, 2])


def test_a_callers_own_requires_grad_camera_is_still_refused():
    from s3gaussian_amd import glue, pipeline
    x = torch.zeros(4, 3)
    campos = torch.zeros(2, 3, requires_grad=True)
    with pytest.raises(RuntimeError, match="activations_and_colors_views: a camera centre requires a gradient"):
        glue.activations_and_colors_views(3, x, x, None, x, campos, x, x, x)
    with pytest.raises(RuntimeError, match="activations_and_colors_views: a camera centre requires a gradient"):
        glue.activations_and_colors_views(3, x, x, None, x, campos, x, x, x, campos_grad=False)
    cam = dict(_camera())
    cam["campos"] = cam["campos"].clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="render_views: a camera requires a gradient"):
        pipeline.render_views([_camera(), cam], None, pipeline._default_pipe(None), torch.zeros(3))
