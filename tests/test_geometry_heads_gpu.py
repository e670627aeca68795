"""Geometry heads (scales_deform / rotations_deform / opacity_deform on the matrix cores, include/s3g_mlp_geom.h) against the same
nn.Linear stack evaluated by PyTorch on the CPU in float64 (scene/deformation.py:61-65,126-152), at the bars tests/test_mlp_gpu.py
holds the same exact fp32 chains to: outputs rtol = atol = 2e-5, g_features relative L2 < 1e-5, parameter gradients relative L2 < 2e-5.

Sizes (the argument of tests/test_static_mlp_gpu.py): 1 .. 33 cover the edge of the 32-point tile, 257 is more than one workgroup
(8 waves x 32 points), 70 001 is more tiles (2188) than the forward's grid has waves (2048) with a ragged last tile.
Points within 1e-5 of a ReLU kink get zero loss weight (both sides then see zero gradient); at most 2 % of the points of any case
(asserted here on the float64 stack).  The float64 reference of a case is computed once and shared."""
import copy
import functools

import numpy as np
import pytest
import torch

from tests.test_mlp_gpu import _min_abs_preactivation, _modules
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

SIZES = [1, 31, 32, 33, 257, 70_001]
HEADS = ("scales_deform", "rotations_deform", "opacity_deform")
WIDTH = (3, 4, 1)
ALL = (True, True, True)
# input seeds: P + 1 as in tests/test_mlp_gpu.py, except where that draw puts a point on a kink and the 2 % cap would not hold
# (P = 33, seed 34: one of 33 points; checked on the float64 stack before the seeds were fixed -- excluded: 0 of 1, 31, 32, 33;
# 1 of 257; 0.24 % of 70 001, 0.50 % there with the MLP's own heads in the loss)
DATA_SEED = {33: 35}


def _geometry_min_abs_preactivation(d, x):
    """tests/test_mlp_gpu.py::_min_abs_preactivation for the three geometry heads: per point, the smallest |input| of any of their ReLUs."""
    with torch.no_grad():
        hidden = d.feature_out(x)
        worst = torch.full((x.shape[0],), float("inf"), dtype=x.dtype)
        for name in HEADS:
            t = hidden
            for m in getattr(d, name):
                if isinstance(m, torch.nn.ReLU):
                    worst = torch.minimum(worst, t.abs().min(dim=1).values)
                t = m(t)
    return worst


def _heads(d, present):
    return [getattr(d, n) if on else None for n, on in zip(HEADS, present)]


@functools.lru_cache(maxsize=None)
def _case(P, present=ALL, with_mlp=False):
    """Float64 reference of one case (read-only): modules, inputs, loss weights, outputs and every gradient.  with_mlp: the loss also
    covers dx / dshs / feat of the same hidden (the graph with both autograd nodes)."""
    d64 = _modules(P).double()
    g = torch.Generator().manual_seed(DATA_SEED.get(P, P + 1))
    x = torch.randn(P, 128, generator=g)
    w = [torch.randn(P, n, generator=g) for n in WIDTH]
    w_mlp = [torch.randn(P, n, generator=g) for n in (3, 48, 3)]
    margin = _geometry_min_abs_preactivation(d64, x.double())
    if with_mlp:
        margin = torch.minimum(margin, _min_abs_preactivation(d64, x.double()))
    keep = (margin > 1e-5).float()[:, None]
    assert float(1 - keep.mean()) <= 0.02, (P, float(1 - keep.mean()))          # the exclusion's cap
    w, w_mlp = [wi * keep for wi in w], [wi * keep for wi in w_mlp]
    x64 = x.double().requires_grad_(True)
    hidden = d64.feature_out(x64)
    outs = [h(hidden) if h is not None else None for h in _heads(d64, present)]
    loss = sum((o * wi.double()).sum() for o, wi in zip(outs, w) if o is not None)
    outs_mlp = None
    if with_mlp:
        outs_mlp = [d64.pos_deform(hidden), d64.shs_deform(hidden), d64.dino_head(hidden)]
        loss = loss + sum((o * wi.double()).sum() for o, wi in zip(outs_mlp, w_mlp))
    loss.backward()
    return dict(d64=d64, x=x, w=w, w_mlp=w_mlp, outs=[None if o is None else o.detach().numpy() for o in outs], gx=x64.grad.numpy(),
                grads={k: (None if p.grad is None else p.grad.numpy()) for k, p in d64.named_parameters()},
                kept=float(keep.mean()))


def _run(case, dev, present=ALL, grad=True):
    """One forward (and backward) of geometry_heads on the case's inputs -> (module copy, outputs, features.grad)."""
    from s3gaussian_amd.mlp_geom import geometry_heads
    dg = copy.deepcopy(case["d64"]).float().to(dev)
    dg.zero_grad(set_to_none=True)
    xg = case["x"].to(dev).requires_grad_(grad)
    with torch.set_grad_enabled(grad):
        outs = geometry_heads(xg, dg.feature_out, *_heads(dg, present))
    if grad:
        sum((o * wi.to(dev)).sum() for o, wi in zip(outs, case["w"]) if o is not None).backward()
    return dg, outs, xg.grad


def _check_against_float64(case, dg, outs, gx, present):
    figures = {}
    for name, o, r in zip(HEADS, outs, case["outs"]):
        assert (o is None) == (r is None), name
        if o is not None:
            figures[name] = float(np.abs(o.detach().cpu().numpy() - r).max())
    figures["g_features"] = rel_l2(gx.cpu().numpy(), case["gx"])
    live = ("feature_out",) + tuple(n for n, on in zip(HEADS, present) if on)
    compared = 0
    for name, p in dg.named_parameters():
        head = name.split(".")[0]
        if head in HEADS and head not in live:
            assert p.grad is None, name                                  # an absent head's parameters are no inputs of the node
        elif head in live:
            assert p.grad is not None, name
            figures[name] = rel_l2(p.grad.cpu().numpy(), case["grads"][name])
            compared += 1
    print("geometry heads vs float64:", figures)                          # every figure before the first assertion
    for o, r in zip(outs, case["outs"]):
        if o is not None:
            np.testing.assert_allclose(o.detach().cpu().numpy(), r, rtol=2e-5, atol=2e-5)
    assert figures["g_features"] < 1e-5
    for name in figures:
        if "." in name:
            assert figures[name] < 2e-5, (name, figures[name])
    assert compared == 2 + 4 * sum(present)
    return figures


@pytest.mark.parametrize("P", SIZES)
def test_geometry_heads_match_the_float64_stack(gpu_device, P):
    """Outputs, g_features and all fourteen parameter gradients."""
    case = _case(P)
    dg, outs, gx = _run(case, gpu_device)
    assert [tuple(o.shape) for o in outs] == [(P, 3), (P, 4), (P, 1)]
    _check_against_float64(case, dg, outs, gx, ALL)


@pytest.mark.parametrize("P", [33, 257])
@pytest.mark.parametrize("present", [(False, True, False), (True, False, True)], ids=["dr", "ds+do"])
def test_head_subsets(gpu_device, present, P):
    """{dr} and {ds, do}: same bars; absent heads return None and leave their parameters' .grad at None; the outputs of the heads that
    are present are bit-identical to the all-heads call."""
    case = _case(P, present)
    dg, outs, gx = _run(case, gpu_device, present)
    _check_against_float64(case, dg, outs, gx, present)
    _, full, _ = _run(_case(P), gpu_device, grad=False)
    for on, o, f in zip(present, outs, full):
        assert (o is None) == (not on)
        if on:
            assert torch.equal(o.detach(), f)


@pytest.mark.parametrize("P", [33, 257])
def test_both_nodes_in_one_graph_add_up(gpu_device, P):
    """deform_mlp and geometry_heads on the same features and the same feature_out, a loss on all six outputs: features.grad, W0.grad
    and b0.grad are the sums autograd forms of the two nodes' terms -- the additivity the separate kernel family rests on."""
    from s3gaussian_amd.mlp import deform_mlp
    from s3gaussian_amd.mlp_geom import geometry_heads
    dev = gpu_device
    case = _case(P, ALL, True)
    dg = copy.deepcopy(case["d64"]).float().to(dev)
    dg.zero_grad(set_to_none=True)
    xg = case["x"].to(dev).requires_grad_(True)
    outs_mlp = deform_mlp(xg, dg.feature_out, dg.pos_deform, dg.shs_deform, dg.dino_head)
    outs = geometry_heads(xg, dg.feature_out, dg.scales_deform, dg.rotations_deform, dg.opacity_deform)
    (sum((o * wi.to(dev)).sum() for o, wi in zip(outs, case["w"]))
     + sum((o * wi.to(dev)).sum() for o, wi in zip(outs_mlp, case["w_mlp"]))).backward()
    figures = {"g_features": rel_l2(xg.grad.cpu().numpy(), case["gx"])}
    for name in ("feature_out.0.weight", "feature_out.0.bias"):
        figures[name] = rel_l2(dict(dg.named_parameters())[name].grad.cpu().numpy(), case["grads"][name])
    print("both nodes vs float64:", figures)
    assert figures["g_features"] < 1e-5
    assert figures["feature_out.0.weight"] < 2e-5 and figures["feature_out.0.bias"] < 2e-5
    for name, p in dg.named_parameters():             # and every head of either node has its gradient
        if name.split(".")[0] in HEADS + ("pos_deform", "shs_deform", "dino_head"):
            assert rel_l2(p.grad.cpu().numpy(), case["grads"][name]) < 2e-5, name


def test_forward_and_backward_are_bit_reproducible(gpu_device):
    """P = 70 001 twice: every output and every gradient equal bit for bit (the weight gradients use no float atomics and a fixed
    summation order)."""
    case = _case(70_001)
    runs = []
    for _ in range(2):
        dg, outs, gx = _run(case, gpu_device)
        runs.append([o.detach() for o in outs] + [gx] + [p.grad for n, p in dg.named_parameters() if p.grad is not None])
    assert len(runs[0]) == 3 + 1 + 14
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("P", [33, 70_001])
def test_outputs_do_not_depend_on_the_stash(gpu_device, P):
    """no_grad (no stash saved) and grad-enabled forwards give bit-identical outputs."""
    case = _case(P)
    _, lean, _ = _run(case, gpu_device, grad=False)
    _, full, _ = _run(case, gpu_device, grad=True)
    for a, b in zip(lean, full):
        assert not a.requires_grad and torch.equal(a, b.detach())
