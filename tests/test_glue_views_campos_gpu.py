"""GPU: every view's camera-centre gradient from the one shared glue backward (glue.activations_and_colors_views(campos_grad=True),
csrc/glue_views_camera.hip) against V calls of the single-camera node, whose campos gradient tests/test_camera_grad_gpu.py pins.

Bit equality is the bar, and why it can be: view v's direction term t_v[p] is formed by the same source under -ffp-contract=off
in both kernels (for V = 1 the two g_xyz are the same bits, tests/test_glue_views_gpu.py), and the sum over P runs in double in the
order of camera_backward_kernel + camera_fold_kernel -- the same workgroup count, stride, butterfly and fold.  So campos.grad[v] is
`torch.equal` to the campos.grad of activations_and_colors for camera v fed the same colour gradient, and asking for it changes no
other gradient by a bit.

Sizes: P around a wave (63 / 64 / 65) and around the 256-thread workgroup (255 / 256 / 257), several workgroups with a ragged last
one (1000, 4001), and 131 329 = 512 * 256 + 257: past CAM_MAX_BLOCKS workgroups, so the stride loop runs a second time for some
threads.  V = 1, 2 | 3 | 5, 8 take the three block sizes of the backward (256 / 128 / 64 rows).

Against float64: each view's gradient against float64 autograd of oracle/torch_ref._sh_color (tests/glue_campos_ref.py), the error
of component k relative to sum_p |t_v[p]_k| at most 4 x the rel-L2 error of that view's single-camera g_xyz against the same
autograd (the project's 4 x rule: a sum over P of terms as accurate as g_xyz's entries, added in double and rounded once).
Measured on an MI355X (profiles/pose_views_errors.json, P = 4001, V = 3): error / sum|term| at most 5.5e-9, g_xyz rel-L2 1.5e-7 .. 1.6e-7.
"""
import pytest
import torch

from tests.glue_campos_ref import campos_grad_ref
from tests.test_glue_views_gpu import NAMES, _grads, _inputs, _leaves
from tests.util import rel_l2

pytestmark = pytest.mark.gpu


def _views_backward(t, dev, deg, with_dshs, campos, w_colors, w_act, campos_grad, live=None):
    """One shared pass each way -> (gradients of the leaves, campos.grad or None)."""
    from s3gaussian_amd.glue import activations_and_colors_views
    L = _leaves(t, dev, with_dshs)
    c = campos.clone().requires_grad_(campos_grad)
    cols, sc, rot, op = activations_and_colors_views(deg, L["f_dc"], L["f_rest"], L["dshs"], L["xyz"], c, L["log_scales"], L["rot_raw"],
                                                     L["opacity_logit"], **({"campos_grad": True} if campos_grad else {}))
    live = range(len(cols)) if live is None else live
    loss = (sc * w_act[0]).sum() + (rot * w_act[1]).sum() + (op * w_act[2]).sum()
    for v in live:
        loss = loss + (cols[v] * w_colors[v]).sum()
    loss.backward()
    return _grads(L), c.grad


def _single_backward(t, dev, deg, with_dshs, campos_v, w_colors_v):
    """The single-camera node for one view, colour gradient only -> (campos.grad [3], xyz.grad [P,3])."""
    from s3gaussian_amd.glue import activations_and_colors
    L = _leaves(t, dev, with_dshs)
    c = campos_v.clone().requires_grad_(True)
    cols = activations_and_colors(deg, L["f_dc"], L["f_rest"], L["dshs"], L["xyz"], c, L["log_scales"], L["rot_raw"], L["opacity_logit"])[0]
    (cols * w_colors_v).sum().backward()
    return c.grad, L["xyz"].grad


def _check(dev, P, V, deg, with_dshs):
    t, campos, w_colors, w_act = _inputs(P, V, 2000 * V + 10 * deg + int(with_dshs) + P)
    campos, w_colors, w_act = campos.to(dev), [w.to(dev) for w in w_colors], [w.to(dev) for w in w_act]
    got, g_campos = _views_backward(t, dev, deg, with_dshs, campos, w_colors, w_act, True)
    assert g_campos.shape == (V, 3) and g_campos.dtype == torch.float32
    want = torch.stack([_single_backward(t, dev, deg, with_dshs, campos[v], w_colors[v])[0] for v in range(V)])
    assert torch.equal(g_campos, want), (g_campos, want)
    if deg == 0 or P == 0:
        assert not g_campos.any()
    elif P >= 63:
        assert bool((g_campos != 0).all())
    plain, none = _views_backward(t, dev, deg, with_dshs, campos, w_colors, w_act, False)
    assert none is None
    for k in NAMES:
        if k == "dshs" and not with_dshs:
            assert got[k] is None and plain[k] is None
        else:
            assert torch.equal(got[k], plain[k]), k
    again, g_again = _views_backward(t, dev, deg, with_dshs, campos, w_colors, w_act, True)
    assert torch.equal(g_again, g_campos) and all(torch.equal(again[k], got[k]) for k in NAMES if got[k] is not None)


@pytest.mark.parametrize("V", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("P", [0, 1, 63, 64, 65, 255, 256, 257, 1000, 4001, 131329])
@pytest.mark.parametrize("with_dshs", [True, False])
def test_campos_gradients_equal_single_camera_calls(gpu_device, P, V, with_dshs):
    _check(gpu_device, P, V, 3, with_dshs)


@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("deg", [0, 1, 2])
def test_campos_gradients_lower_degrees(gpu_device, deg, V):
    _check(gpu_device, 1000, V, deg, True)


@pytest.mark.parametrize("V,skip", [(2, 0), (3, 1), (8, 7)])
def test_a_view_without_a_colour_gradient_gets_exact_zeros(gpu_device, V, skip):
    dev, P = gpu_device, 1000
    t, campos, w_colors, w_act = _inputs(P, V, 91 + V)
    campos, w_colors, w_act = campos.to(dev), [w.to(dev) for w in w_colors], [w.to(dev) for w in w_act]
    live = [v for v in range(V) if v != skip]
    _, g_campos = _views_backward(t, dev, 3, True, campos, w_colors, w_act, True, live=live)
    assert not g_campos[skip].any()
    for v in live:
        assert torch.equal(g_campos[v], _single_backward(t, dev, 3, True, campos[v], w_colors[v])[0]), v


@pytest.mark.parametrize("V", [2, 5])
def test_zero_colour_gradients_give_exact_zeros(gpu_device, V):
    """Zero gradients that do arrive (tensors of zeros, not NULL pointers): every term is 0 * finite, the sums exact zeros, no NaN."""
    dev, P = gpu_device, 257
    t, campos, w_colors, w_act = _inputs(P, V, 17 + V)
    campos, w_act = campos.to(dev), [w.to(dev) for w in w_act]
    zeros = [torch.zeros(P, 3, device=dev) for _ in range(V)]
    _, g_campos = _views_backward(t, dev, 3, True, campos, zeros, w_act, True)
    assert bool(torch.isfinite(g_campos).all()) and not g_campos.any()


def campos_errors(dev, P=4001, V=3, deg=3, seed=7):
    """Per view: (error of campos.grad over sum|term| per component, rel-L2 of the single-camera g_xyz), both against float64
    autograd of torch_ref._sh_color on the fp32 inputs."""
    from oracle import torch_ref
    t, campos, w_colors, w_act = _inputs(P, V, seed)
    _, g_campos = _views_backward(t, dev, deg, True, campos.to(dev), [w.to(dev) for w in w_colors], [w.to(dev) for w in w_act], True)
    shs = torch.cat([t["f_dc"], t["f_rest"]], 1).double() + t["dshs"].double()
    rows = []
    for v in range(V):
        c = campos[v].double().clone().requires_grad_(True)
        x = t["xyz"].double().clone().requires_grad_(True)
        col = torch_ref._sh_color(deg, shs, x, c)
        want_c, want_x = torch.autograd.grad((col * w_colors[v].double()).sum(), (c, x))
        _, abs_sum = campos_grad_ref(deg, shs, t["xyz"], campos[v], w_colors[v], col.detach() > 0)
        g_xyz = _single_backward(t, dev, deg, True, campos[v].to(dev), w_colors[v].to(dev))[1]
        rows.append(dict(view=v, err_over_sum_abs_term=((g_campos[v].double().cpu() - want_c).abs() / abs_sum).tolist(),
                         g_xyz_rel=float(rel_l2(g_xyz.cpu().numpy(), want_x.numpy()))))
    return rows


def test_campos_gradients_against_float64_autograd(gpu_device):
    rows = campos_errors(gpu_device)
    print("campos gradient of the shared glue pass vs float64 autograd:", rows)
    for r in rows:
        assert 0 < r["g_xyz_rel"] < 1e-5
        assert max(r["err_over_sum_abs_term"]) <= 4 * r["g_xyz_rel"], r
