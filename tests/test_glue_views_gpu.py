"""Render glue for V cameras of one timestamp (glue.activations_and_colors_views, csrc/glue_views.hip) against V calls of the
single-camera node (glue.activations_and_colors, pinned to the reference by tests/test_glue_gpu.py).

What is asserted, and why bit equality is the right bar: both kernels run the same per-camera source (csrc/glue_dev.hpp) under
-ffp-contract=off, so a view's colours are the same bits; a coefficient gradient is sum_v basis_v[k] * dRGB_v[c] with every
product rounded before it is added, view 0 first, which is exactly what adding the V single-camera gradients left to right in
fp32 computes.  Only with the mean|dshs| term the order differs (the batch adds it after the sum, the V calls' sum has it inside
call 0): rel-L2 1e-6, i.e. a few fp32 roundings.

Block edges: P = 0 (no launch), 1, 255 / 256 / 257 around the forward's 256-row block, 4001 = many blocks and a ragged last one
for every backward block size (256 rows up to 2 views, 128 up to 4, 64 up to 8: V = 1, 2 | 3 | 8 take the three)."""
import pytest
import torch

from tests.util import rel_l2

pytestmark = pytest.mark.gpu

NAMES = ("f_dc", "f_rest", "dshs", "xyz", "log_scales", "rot_raw", "opacity_logit")


def _inputs(P, V, seed):
    g = torch.Generator().manual_seed(seed)
    mk = lambda *s: torch.randn(*s, generator=g)
    f_dc = mk(P, 1, 3)
    f_dc[::3] -= 2.5                       # a third of the Gaussians around the clamp: colours at 0 with a dead gradient
    t = dict(f_dc=f_dc, f_rest=0.3 * mk(P, 15, 3), dshs=0.1 * mk(P, 16, 3), xyz=3 * mk(P, 3), log_scales=0.5 * mk(P, 3),
             rot_raw=mk(P, 4), opacity_logit=mk(P, 1))
    campos = 2.0 * mk(V, 3)
    w_colors = [mk(P, 3) for _ in range(V)]
    w_act = [mk(P, 3), mk(P, 4), mk(P, 1)]
    return t, campos, w_colors, w_act


def _leaves(t, dev, with_dshs):
    L = {k: v.clone().to(dev).requires_grad_(True) for k, v in t.items()}
    if not with_dshs:
        L["dshs"] = None
    return L


def _views(L, deg, campos, l1):
    from s3gaussian_amd.glue import activations_and_colors_views
    return activations_and_colors_views(deg, L["f_dc"], L["f_rest"], L["dshs"], L["xyz"], campos, L["log_scales"], L["rot_raw"],
                                        L["opacity_logit"], with_dshs_l1=l1)


def _single(L, deg, campos_v, l1):
    from s3gaussian_amd.glue import activations_and_colors
    return activations_and_colors(deg, L["f_dc"], L["f_rest"], L["dshs"], L["xyz"], campos_v, L["log_scales"], L["rot_raw"],
                                  L["opacity_logit"], with_dshs_l1=l1)


def _grads(L):
    return {k: (None if (v is None or v.grad is None) else v.grad.clone()) for k, v in L.items()}


def _sum_of_single_calls(t, dev, deg, with_dshs, campos, w_colors, w_act, views=None):
    """Left-to-right fp32 sum of the gradients of one single-camera backward per view; the activation gradients go into call 0."""
    total = None
    for n, v in enumerate(range(len(w_colors)) if views is None else views):
        L = _leaves(t, dev, with_dshs)
        cols, sc, rot, op = _single(L, deg, campos[v], False)
        loss = (cols * w_colors[v]).sum()
        if n == 0:
            loss = loss + (sc * w_act[0]).sum() + (rot * w_act[1]).sum() + (op * w_act[2]).sum()
        loss.backward()
        g = _grads(L)
        total = g if total is None else {k: (None if total[k] is None else total[k] + g[k]) for k in total}
    return total


def _check(dev, P, V, deg, with_dshs):
    t, campos, w_colors, w_act = _inputs(P, V, 1000 * V + 10 * deg + int(with_dshs) + P)
    campos, w_colors, w_act = campos.to(dev), [w.to(dev) for w in w_colors], [w.to(dev) for w in w_act]
    # ---- forward: every view's colours, the activations and mean|dshs| are those of the single-camera node
    Lv = _leaves(t, dev, with_dshs)
    out = _views(Lv, deg, campos, with_dshs)
    cols, sc, rot, op = out[:4]
    assert len(cols) == V and all(c.shape == (P, 3) for c in cols)
    assert len({c.data_ptr() for c in cols}) == V or P == 0          # tensors of their own, not slices of one block
    for v in range(V):
        ref = _single(_leaves(t, dev, with_dshs), deg, campos[v], with_dshs)
        assert torch.equal(cols[v], ref[0]), (v, "colors")
        assert torch.equal(sc, ref[1]) and torch.equal(rot, ref[2]) and torch.equal(op, ref[3]), v
        if with_dshs:
            assert torch.equal(out[4], ref[4]), (v, "dshs_l1")
    if P >= 255:
        assert all(bool((c == 0).any()) and bool((c > 0).any()) for c in cols)      # clamped and live colours in every view
    # ---- backward without the L1 term: bit-equal to the sum of V single-camera calls
    Lv = _leaves(t, dev, with_dshs)
    cols, sc, rot, op = _views(Lv, deg, campos, False)
    (sum((c * w).sum() for c, w in zip(cols, w_colors)) + (sc * w_act[0]).sum() + (rot * w_act[1]).sum() + (op * w_act[2]).sum()).backward()
    got, want = _grads(Lv), _sum_of_single_calls(t, dev, deg, with_dshs, campos, w_colors, w_act)
    for k in NAMES:
        if k == "dshs" and not with_dshs:
            assert got[k] is None
            continue
        assert got[k].shape == want[k].shape and torch.equal(got[k], want[k]), k
    if not with_dshs:
        return
    # ---- backward with the L1 term (700 * mean|dshs| rides along): V = 1 is the existing node bit for bit, V > 1 rel-L2 1e-6
    Lv = _leaves(t, dev, True)
    cols, sc, rot, op, l1 = _views(Lv, deg, campos, True)
    (sum((c * w).sum() for c, w in zip(cols, w_colors)) + (sc * w_act[0]).sum() + (rot * w_act[1]).sum() + (op * w_act[2]).sum()
     + 700.0 * l1).backward()
    got = _grads(Lv)
    if V == 1:
        Ls = _leaves(t, dev, True)
        c1, s1, r1, o1, l1s = _single(Ls, deg, campos[0], True)
        ((c1 * w_colors[0]).sum() + (s1 * w_act[0]).sum() + (r1 * w_act[1]).sum() + (o1 * w_act[2]).sum() + 700.0 * l1s).backward()
        ref = _grads(Ls)
        for k in NAMES:
            assert torch.equal(got[k], ref[k]), k
        return
    if P == 0:
        return
    want["dshs"] = want["dshs"] + torch.sign(Lv["dshs"].detach()) * (torch.tensor(700.0, device=dev) / (48.0 * P))
    for k in NAMES:
        if float(want[k].abs().max()) == 0.0:      # degree 0 does not depend on the view direction
            assert float(got[k].abs().max()) == 0.0, k
        else:
            assert rel_l2(got[k].cpu().numpy(), want[k].cpu().numpy()) < 1e-6, k


@pytest.mark.parametrize("V", [1, 2, 3, 8])
@pytest.mark.parametrize("P", [0, 1, 255, 256, 257, 4001])
@pytest.mark.parametrize("with_dshs", [True, False])
def test_views_equal_single_camera_calls_block_edges(gpu_device, P, V, with_dshs):
    _check(gpu_device, P, V, 3, with_dshs)


@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("deg", [0, 1, 2])
@pytest.mark.parametrize("with_dshs", [True, False])
def test_views_equal_single_camera_calls_lower_degrees(gpu_device, deg, V, with_dshs):
    _check(gpu_device, 257, V, deg, with_dshs)


@pytest.mark.parametrize("V,skip", [(2, 0), (3, 1), (8, 7)])
def test_a_view_without_a_colour_gradient_passes_null(gpu_device, V, skip):
    """A view whose colours fed nothing hands the node no gradient (it does not materialise zeros): s3g_glue_backward_views gets
    NULL for it.  The result is the sum over the other views' single-camera calls."""
    dev, P = gpu_device, 257
    t, campos, w_colors, w_act = _inputs(P, V, 77 + V)
    campos, w_colors, w_act = campos.to(dev), [w.to(dev) for w in w_colors], [w.to(dev) for w in w_act]
    Lv = _leaves(t, dev, True)
    cols, sc, rot, op = _views(Lv, 3, campos, False)
    live = [v for v in range(V) if v != skip]
    (sum((cols[v] * w_colors[v]).sum() for v in live) + (sc * w_act[0]).sum() + (rot * w_act[1]).sum() + (op * w_act[2]).sum()).backward()
    got, want = _grads(Lv), _sum_of_single_calls(t, dev, 3, True, campos, w_colors, w_act, views=live)
    for k in NAMES:
        assert torch.equal(got[k], want[k]), k


def test_only_the_l1_term_reaches_backward(gpu_device):
    """No colour and no activation gradient at all (every upstream pointer NULL): g_dshs is the sign term alone, all else zero."""
    dev, P, V = gpu_device, 300, 3
    t, campos, _, _ = _inputs(P, V, 5)
    Lv = _leaves(t, dev, True)
    out = _views(Lv, 3, campos.to(dev), True)
    (96.0 * out[4]).backward()
    g = _grads(Lv)
    assert torch.equal(g["dshs"], torch.sign(Lv["dshs"].detach()) * (torch.tensor(96.0, device=dev) / (48.0 * P)))
    for k in NAMES:
        if k != "dshs":
            assert float(g[k].abs().max()) == 0.0, k


def test_refusals(gpu_device):
    from s3gaussian_amd.glue import activations_and_colors_views
    t, campos, _, _ = _inputs(4, 9, 0)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        activations_and_colors_views(3, t["f_dc"], t["f_rest"], None, t["xyz"], campos[:2], t["log_scales"], t["rot_raw"], t["opacity_logit"])
    d = {k: v.to(gpu_device) for k, v in t.items()}
    with pytest.raises(RuntimeError, match="9 views"):
        activations_and_colors_views(3, d["f_dc"], d["f_rest"], None, d["xyz"], campos, d["log_scales"], d["rot_raw"], d["opacity_logit"])
