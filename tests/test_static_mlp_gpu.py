"""The fused deformation MLP without its position head (`deform_mlp(..., need_dx=False)`: static scenes, ModelHiddenParams
no_dx=True) in every arithmetic: against the float64 nn.Linear stack of tests/test_mlp_gpu.py, bit for bit against the full call
(forward; backward with an explicitly zero gradient on dx), pre-split against on-the-fly split, and run-to-run.

P: 1 / 31 / 32 / 33 = the 32-point tile edge; 257 = nine tiles, more than one 8-wave workgroup; 70 001 = 2188 tiles, more than the
256 x 8 = 2048 waves of the grid, so some waves take a second tile through the prefetch hand-over, and the last tile is ragged."""
import copy

import numpy as np
import pytest
import torch

from tests.test_mlp_gpu import _min_abs_preactivation, _modules, _ref
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

SIZES = [1, 31, 32, 33, 257, 70_001]
LIVE = ("feature_out", "shs_deform", "dino_head")


@pytest.fixture
def arithmetic(request):
    """Sets the process-wide arithmetic of the per-point GEMM chains for one test and restores the default."""
    from s3gaussian_amd import mlp
    mlp.set_mlp_arithmetic(request.param)
    yield request.param
    mlp.set_mlp_arithmetic(mlp.DEFAULT_ARITHMETIC)


def _mods(d):
    return d.feature_out, d.pos_deform, d.shs_deform, d.dino_head


@pytest.mark.parametrize("arithmetic", ["f32", "bf16x3"], indirect=True)
@pytest.mark.parametrize("P", SIZES)
def test_static_mlp_matches_linear_stack(gpu_device, P, arithmetic):
    """Outputs, g_features and the twelve live parameter gradients against the float64 stack at the bars tests/test_mlp_gpu.py holds
    the full call to; dx is None and the position head's parameters receive no gradient at all."""
    from s3gaussian_amd.mlp import deform_mlp, get_mlp_arithmetic
    assert get_mlp_arithmetic() == arithmetic
    d64 = _modules(P).double()
    dg = copy.deepcopy(d64).float().to(gpu_device)
    g = torch.Generator().manual_seed(P + 1)
    x = torch.randn(P, 128, generator=g)
    w = [torch.randn(P, n, generator=g) for n in (48, 3)]
    x64 = x.double().requires_grad_(True)
    keep = (_min_abs_preactivation(d64, x.double()) > 1e-5).float()[:, None]   # points on a ReLU kink: zero loss weight
    w = [wi * keep for wi in w]
    outs64 = _ref(d64, x64)[1:]
    sum((o * wi.double()).sum() for o, wi in zip(outs64, w)).backward()
    xg = x.to(gpu_device).requires_grad_(True)
    dx, dshs, feat = deform_mlp(xg, *_mods(dg), need_dx=False)
    assert dx is None
    sum((o * wi.to(gpu_device)).sum() for o, wi in zip((dshs, feat), w)).backward()
    for o, r in zip((dshs, feat), outs64):
        np.testing.assert_allclose(o.detach().cpu().numpy(), r.detach().numpy(), rtol=2e-5, atol=2e-5)
    e = rel_l2(xg.grad.cpu().numpy(), x64.grad.numpy())
    print(f"P={P} {arithmetic}: g_features rel L2 {e:.3g}")
    assert e < 1e-5
    ref_params = dict(d64.named_parameters())
    for name, p in dg.named_parameters():
        if name.startswith("pos_deform"):
            assert p.grad is None and ref_params[name].grad is None, name
        elif name.startswith(LIVE):
            assert p.grad is not None, name
            e = rel_l2(p.grad.cpu().numpy(), ref_params[name].grad.numpy())
            print(f"  {name}: rel L2 {e:.3g}")
            assert e < 2e-5, name


@pytest.mark.parametrize("arithmetic", ["f32", "bf16x3", "bf16x3_onthefly"], indirect=True)
@pytest.mark.parametrize("P", [33, 70_001])
def test_static_forward_is_bit_identical_to_the_full_call(gpu_device, P, arithmetic):
    from s3gaussian_amd.mlp import deform_mlp
    d = _modules(5).float().to(gpu_device)
    x = torch.randn(P, 128, generator=torch.Generator().manual_seed(P)).to(gpu_device)
    with torch.no_grad():
        full = deform_mlp(x, *_mods(d))
        static = deform_mlp(x, *_mods(d), need_dx=False)
        lean = deform_mlp(x, *_mods(d), need_feat=False, need_dx=False)      # dx == NULL combined with feat == NULL
    assert static[0] is None and torch.equal(static[1], full[1]) and torch.equal(static[2], full[2])
    assert lean[0] is None and lean[2] is None and torch.equal(lean[1], full[1])
    xg = x.clone().requires_grad_(True)       # with a stash (a backward may follow): same outputs again
    train = deform_mlp(xg, *_mods(d), need_dx=False)
    assert train[0] is None and torch.equal(train[1], full[1]) and torch.equal(train[2], full[2])


def _backward(d, x, w, need_dx, with_feat):
    from s3gaussian_amd.mlp import deform_mlp
    d.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_(True)
    dx, dshs, feat = deform_mlp(xg, *_mods(d), need_dx=need_dx)
    loss = (dshs * w[0]).sum()
    if with_feat:
        loss = loss + (feat * w[1]).sum()
    if need_dx:
        loss = loss + dx.sum() * 0.0          # an explicitly zero gradient on dx
    loss.backward()
    return xg.grad, {k: (None if p.grad is None else p.grad.clone()) for k, p in d.named_parameters()}


@pytest.mark.parametrize("arithmetic", ["f32", "bf16x3", "bf16x3_onthefly"], indirect=True)
@pytest.mark.parametrize("ordered", [True, False])
@pytest.mark.parametrize("with_feat", [True, False])
@pytest.mark.parametrize("P", [33, 70_001])
def test_static_backward_equals_the_full_call_with_a_zero_dx_gradient(gpu_device, P, with_feat, ordered, arithmetic, monkeypatch):
    """The pattern of test_unused_feature_head_gets_no_gradient: skipping the head = feeding it zeros.  g_features may differ in the
    sign of a zero only; so may the live weight gradients under the ordered flush; the atomic flush is held to summation-order
    round-off (that test's 1e-6)."""
    from s3gaussian_amd import mlp as M
    monkeypatch.setattr(M, "ORDERED_WGRAD_FLUSH", ordered)
    dev = gpu_device
    d = _modules(11).float().to(dev)
    g = torch.Generator().manual_seed(P + 7)
    x = (torch.randn(P, 128, generator=g) * 0.5).to(dev)
    w = [torch.randn(P, n, generator=g).to(dev) for n in (48, 3)]
    gx_f, g_f = _backward(d, x, w, True, with_feat)
    gx_s, g_s = _backward(d, x, w, False, with_feat)
    assert torch.equal(gx_s + 0.0, gx_f + 0.0)
    for k in g_s:
        if k.startswith("pos_deform"):
            assert g_s[k] is None and g_f[k] is not None and float(g_f[k].abs().max()) == 0.0, k
        elif k.startswith("dino_head") and not with_feat:
            assert g_s[k] is None and g_f[k] is None, k
        elif k.startswith(LIVE):
            assert g_s[k] is not None and g_f[k] is not None, k
            if ordered:
                assert torch.equal(g_s[k] + 0.0, g_f[k] + 0.0), k
            else:
                assert rel_l2(g_s[k].cpu().numpy(), g_f[k].cpu().numpy()) < 1e-6, k


@pytest.mark.parametrize("P", [33, 70_001])
def test_static_presplit_is_bit_identical_to_the_on_the_fly_split(gpu_device, P):
    from s3gaussian_amd import mlp as M
    dev = gpu_device
    d = _modules(2).float().to(dev)
    g = torch.Generator().manual_seed(P + 3)
    x = (torch.rand(P, 128, generator=g) * 0.5).to(dev)
    w = [torch.randn(P, n, generator=g).to(dev) for n in (48, 3)]
    res = {}
    try:
        for mode in ("bf16x3_onthefly", "bf16x3"):
            M.set_mlp_arithmetic(mode)
            xg = x.clone().requires_grad_(True)
            dx, dshs, feat = M.deform_mlp(xg, *_mods(d), need_dx=False)
            ((dshs * w[0]).sum() + (feat * w[1]).sum()).backward()
            res[mode] = (dshs.detach(), feat.detach(), xg.grad)
    finally:
        M.set_mlp_arithmetic(M.DEFAULT_ARITHMETIC)
    for a, b in zip(res["bf16x3_onthefly"], res["bf16x3"]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("with_feat", [True, False])
def test_static_weight_gradients_are_bit_reproducible(gpu_device, with_feat):
    """Seven jobs (four without a feature gradient) instead of eight in the weight-gradient launch: the ordered flush still sums
    every job's partial blocks in workgroup order."""
    from s3gaussian_amd import mlp as M
    assert M.ORDERED_WGRAD_FLUSH
    dev = gpu_device
    P = 70_001
    d = _modules(3).float().to(dev)
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(P, 128, generator=g) * 0.5).to(dev)
    w = [torch.randn(P, n, generator=g).to(dev) for n in (48, 3)]
    runs = [_backward(d, x, w, False, with_feat)[1] for _ in range(3)]
    used = [k for k, v in runs[0].items() if v is not None]
    assert len(used) == (12 if with_feat else 6), used
    assert not any(k.startswith("pos_deform") for k in used)
    for r in runs[1:]:
        for k in used:
            assert torch.equal(r[k].view(torch.int32), runs[0][k].view(torch.int32)), k
