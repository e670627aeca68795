"""The fused deformation MLP with the SH head or the feature head switched off (`deform_mlp(..., need_dshs=False)`,
`dino_head=None`; ModelHiddenParams no_dshs / feat_head): the five head triples (dx, dshs, feat) the library did not serve under
autograd -- (1,1,0) (0,1,0) on the existing chain kernels with feat == NULL and a stash, (1,0,1) (1,0,0) (0,0,1) on the kernels
without the SH head (csrc/mlp_heads.hip) -- against the float64 nn.Linear stack of tests/test_mlp_gpu.py at the bars that file holds
the full call to, bit for bit against the full call, with the unwritten stash planes / mask words overwritten, and run to run.

The kernels without the SH head run the exact fp32 MFMA chain in every S3G_MLP_ARITHMETIC mode: their results do not depend on the
mode, and they are bit-identical to the full call's in mode "f32" only.  The (.,1,0) triples run the mode's own kernels: bit-identical
to the full call in all three modes.

P: 1 / 31 / 32 / 33 = the 32-point tile edge; 257 = nine tiles, more than one 8-wave workgroup; 70 001 = 2188 tiles, more than the
256 x 8 = 2048 waves of the grid, with a ragged last tile.

Measured on one MI355X (profiles/head_subsets_errors.json): outputs within 1.5e-6 of float64 (bar 2e-5 absolute + relative),
g_features relative L2 <= 2.5e-7 (bar 1e-5), parameter gradients <= 2.0e-6 (bar 2e-5), over both arithmetics."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests.test_mlp_gpu import _min_abs_preactivation, _modules, _ref
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

SIZES = [1, 31, 32, 33, 257, 70_001]
TRIPLES = [(1, 1, 0), (0, 1, 0), (1, 0, 1), (1, 0, 0), (0, 0, 1)]     # (dx, dshs, feat)
HEADS = ("pos_deform", "shs_deform", "dino_head")
WIDTHS = (3, 48, 3)
ALL_MODES = ["f32", "bf16x3", "bf16x3_onthefly"]


@pytest.fixture
def arithmetic(request):
    """Sets the process-wide arithmetic of the per-point GEMM chains for one test and restores the default."""
    from s3gaussian_amd import mlp
    mlp.set_mlp_arithmetic(request.param)
    yield request.param
    mlp.set_mlp_arithmetic(mlp.DEFAULT_ARITHMETIC)


def _call(d, x, triple):
    from s3gaussian_amd.mlp import deform_mlp
    return deform_mlp(x, d.feature_out, d.pos_deform, d.shs_deform, d.dino_head if triple[2] else None,
                      need_dx=bool(triple[0]), need_dshs=bool(triple[1]))


@functools.lru_cache(maxsize=None)
def _reference(P, triple):
    """The float64 side, computed once per (P, triple) and shared by the arithmetics: (module, x, loss weights, float64 outputs,
    float64 g_features, float64 parameter gradients, share of points left out).  Nothing of it is modified afterwards."""
    d64 = _modules(P).double()
    g = torch.Generator().manual_seed(P + 1)
    x = torch.randn(P, 128, generator=g)
    w = [torch.randn(P, n, generator=g) for n in WIDTHS]
    keep = (_min_abs_preactivation(d64, x.double()) > 1e-5).float()[:, None]   # points on a ReLU kink: zero loss weight
    w = [wi * keep for wi in w]
    x64 = x.double().requires_grad_(True)
    outs64 = _ref(d64, x64)
    sum((o * wi.double()).sum() for o, wi, on in zip(outs64, w, triple) if on).backward()
    grads = {k: (None if p.grad is None else p.grad.numpy()) for k, p in d64.named_parameters()}
    return d64, x, w, [o.detach().numpy() for o in outs64], x64.grad.numpy(), grads, 1.0 - float(keep.mean())


def float64_errors(P, triple, dev):
    """-> (outputs, float64 outputs, {name: relative L2 error}, share of points left out, parameters whose .grad is None)."""
    d64, x, w, outs64, gx64, grads64, left_out = _reference(P, triple)
    dg = copy.deepcopy(d64).float().to(dev)
    xg = x.to(dev).requires_grad_(True)
    outs = _call(dg, xg, triple)
    sum((o * wi.to(dev)).sum() for o, wi, on in zip(outs, w, triple) if on).backward()
    errs = {"g_features": rel_l2(xg.grad.cpu().numpy(), gx64)}
    none = []
    for name, p in dg.named_parameters():
        if not name.startswith(("feature_out",) + HEADS):
            continue
        if p.grad is None:
            assert grads64[name] is None, name
            none.append(name)
        else:
            errs[name] = rel_l2(p.grad.cpu().numpy(), grads64[name])
    return outs, outs64, errs, left_out, none


@pytest.mark.parametrize("arithmetic", ["f32", "bf16x3"], indirect=True)
@pytest.mark.parametrize("triple", TRIPLES)
@pytest.mark.parametrize("P", SIZES)
def test_head_subset_matches_linear_stack(gpu_device, P, triple, arithmetic):
    """Outputs, g_features and every live parameter gradient against the float64 stack; an absent head's output is None and its
    parameters receive no gradient at all."""
    from s3gaussian_amd.mlp import get_mlp_arithmetic
    assert get_mlp_arithmetic() == arithmetic
    outs, outs64, errs, left_out, none = float64_errors(P, triple, gpu_device)
    assert left_out <= 0.01, left_out
    for o, r, on in zip(outs, outs64, triple):
        assert (o is not None) == bool(on)
        if on:
            np.testing.assert_allclose(o.detach().cpu().numpy(), r, rtol=2e-5, atol=2e-5)
    print(f"P={P} {triple} {arithmetic}: left out {left_out:.4f} " + " ".join(f"{k}={v:.3g}" for k, v in errs.items()))
    assert errs.pop("g_features") < 1e-5
    absent = tuple(h for h, on in zip(HEADS, triple) if not on)
    assert sorted(none) == sorted(n for n in none if n.startswith(absent)) and len(none) == sum(6 if h == "dino_head" else 4 for h in absent)
    assert len(errs) == 16 - len(none)
    for name, e in errs.items():
        assert e < 2e-5, name


def _modes(triple):
    """The arithmetic modes in which the triple's kernels compute what the full call's kernels compute."""
    return ALL_MODES if triple[1] else ["f32"]


def _backward(d, x, w, triple, full):
    """The triple's backward; full=True: the full call with an explicitly zero gradient on the absent heads' outputs."""
    d.zero_grad(set_to_none=True)
    xg = x.clone().requires_grad_(True)
    outs = _call(d, xg, (1, 1, 1) if full else triple)
    loss = sum((o * wi).sum() if on else o.sum() * 0.0 for o, wi, on in zip(outs, w, triple) if o is not None)
    loss.backward()
    return outs, xg.grad, {k: (None if p.grad is None else p.grad.clone()) for k, p in d.named_parameters()}


@pytest.mark.parametrize("triple", TRIPLES)
@pytest.mark.parametrize("P", [33, 70_001])
def test_head_subset_is_bit_identical_to_the_full_call(gpu_device, P, triple):
    """Present outputs equal the full call's (no_grad and with a stash); with the ordered flush g_features and the live weight
    gradients equal a full backward fed zeros for the absent heads.  In every mode of _modes(triple); in the other modes the
    kernels without the SH head give their "f32" results again."""
    from s3gaussian_amd import mlp as M
    assert M.ORDERED_WGRAD_FLUSH
    dev = gpu_device
    d = _modules(11).float().to(dev)
    g = torch.Generator().manual_seed(P + 7)
    x = (torch.randn(P, 128, generator=g) * 0.5).to(dev)
    w = [torch.randn(P, n, generator=g).to(dev) for n in WIDTHS]
    live = ("feature_out",) + tuple(h for h, on in zip(HEADS, triple) if on)
    exact = None
    try:
        for mode in ALL_MODES:
            M.set_mlp_arithmetic(mode)
            with torch.no_grad():
                lean = _call(d, x, triple)
            outs_s, gx_s, g_s = _backward(d, x, w, triple, full=False)
            for a, b in zip(lean, outs_s):
                assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
            if mode in _modes(triple):
                outs_f, gx_f, g_f = _backward(d, x, w, triple, full=True)
                for o, f, on in zip(outs_s, outs_f, triple):
                    assert (o is not None) == bool(on) and (o is None or torch.equal(o, f)), mode
                assert torch.equal(gx_s, gx_f), mode
                for k in g_s:
                    if k.startswith(live):
                        assert g_s[k] is not None and torch.equal(g_s[k], g_f[k]), (mode, k)
                    elif k.startswith(HEADS):
                        assert g_s[k] is None and g_f[k] is not None and float(g_f[k].abs().max()) == 0.0, (mode, k)
            if not triple[1]:      # the exact chain whatever the mode
                res = [o for o in outs_s if o is not None] + [gx_s] + [g_s[k] for k in sorted(g_s) if g_s[k] is not None]
                if exact is None:
                    exact = res
                assert len(res) == len(exact) and all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(res, exact)), mode
    finally:
        M.set_mlp_arithmetic(M.DEFAULT_ARITHMETIC)


@pytest.mark.parametrize("triple", TRIPLES)
def test_head_subset_is_bit_reproducible(gpu_device, triple):
    from s3gaussian_amd import mlp as M
    assert M.ORDERED_WGRAD_FLUSH
    dev = gpu_device
    P = 70_001
    d = _modules(3).float().to(dev)
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(P, 128, generator=g) * 0.5).to(dev)
    w = [torch.randn(P, n, generator=g).to(dev) for n in WIDTHS]
    runs = [_backward(d, x, w, triple, full=False) for _ in range(2)]
    used = [k for k, v in runs[0][2].items() if v is not None]
    assert len(used) == 2 + sum(n for n, on in zip((4, 4, 6), triple) if on)
    for a, b in zip(runs[0][0], runs[1][0]):
        assert (a is None) == (b is None) and (a is None or torch.equal(a.view(torch.int32), b.view(torch.int32)))
    assert torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32))
    for k in used:
        assert torch.equal(runs[0][2][k].view(torch.int32), runs[1][2][k].view(torch.int32)), k


@pytest.mark.parametrize("arithmetic", ["f32", "bf16x3"], indirect=True)
@pytest.mark.parametrize("triple", TRIPLES)
@pytest.mark.parametrize("P", [33, 70_001])
def test_backward_does_not_depend_on_the_unwritten_stash(gpu_device, P, triple, arithmetic):
    """C ABI level: after the forward, the stash planes and mask words of the absent heads (which the forward leaves unwritten) are
    overwritten with NaN / all-ones; the ordered backward's g_features and weight gradients do not change by a bit."""
    from s3gaussian_amd import _lib
    from s3gaussian_amd import mlp as M
    dev = gpu_device
    L = M._bind()
    d = _modules(4).float().to(dev)
    g = torch.Generator().manual_seed(P + 13)
    x = (torch.randn(P, 128, generator=g) * 0.5).to(dev)
    ps = [p.detach() for p in M._head_params(d.feature_out, d.pos_deform, d.shs_deform, d.dino_head)]
    w = M._pack(ps)
    outs = [torch.empty(P, n, device=dev) if on else None for n, on in zip(WIDTHS, triple)]
    gs = [torch.randn(P, n, generator=g).to(dev) if on else None for n, on in zip(WIDTHS, triple)]
    ptr = lambda t: None if t is None else t.data_ptr()
    stash = torch.empty(L.s3g_deform_mlp_stash_bytes(P) // 4, device=dev)
    pack = L.s3g_deform_mlp_pack_bytes() // 4
    tiles = (P + 31) // 32
    assert stash.numel() == pack + 5 * P * 64 + tiles * 5 * 64
    stream = _lib.stream_ptr()
    _lib.check(L.s3g_deform_mlp_forward(C.byref(w), P, x.data_ptr(), *map(ptr, outs), stash.data_ptr(), 1, stream))
    poisoned = stash.clone()
    planes = poisoned[pack:pack + 5 * P * 64].view(5, P, 64)
    words = poisoned[pack + 5 * P * 64:].view(torch.int32).view(tiles, 5, 64)
    absent_planes = [k for k, on in ((1, triple[0]), (2, triple[1]), (3, triple[2]), (4, triple[2])) if not on]
    for k in absent_planes:
        planes[k] = float("nan")
        words[:, k] = -1
    results = []
    for st in (stash, poisoned):
        grads = [torch.zeros_like(p) if triple[HEADS.index(h)] else None
                 for p, h in zip(ps[2:], ("pos_deform",) * 4 + ("shs_deform",) * 4 + ("dino_head",) * 6)]
        grads = [torch.zeros_like(ps[0]), torch.zeros_like(ps[1])] + grads
        gw = M._pack(grads)
        gx = torch.empty_like(x)
        ws = torch.empty(5, P, 64, device=dev)
        part = torch.empty(L.s3g_deform_mlp_wgrad_partial_bytes() // 4, device=dev)
        _lib.check(L.s3g_deform_mlp_backward_ordered(C.byref(w), P, x.data_ptr(), st.data_ptr(), *map(ptr, gs), gx.data_ptr(), C.byref(gw),
                                                     ws.data_ptr(), part.data_ptr(), stream))
        results.append([gx] + [t for t in grads if t is not None])
    torch.cuda.synchronize()
    assert len(results[0]) == 3 + sum(n for n, on in zip((4, 4, 6), triple) if on)
    for a, b in zip(*results):
        assert not torch.isnan(a).any()
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_nothing_to_compute_means_no_launch(gpu_device):
    from s3gaussian_amd.mlp import deform_mlp
    d = _modules(1).float().to(gpu_device)
    x = torch.randn(40, 128, device=gpu_device)
    with torch.no_grad():
        assert deform_mlp(x, d.feature_out, d.pos_deform, d.shs_deform, d.dino_head, need_feat=False, need_dx=False, need_dshs=False) == (None,) * 3
        lean = deform_mlp(x, d.feature_out, d.pos_deform, d.shs_deform, d.dino_head, need_feat=False, need_dshs=False)     # (1,0,0) under no_grad
        full = deform_mlp(x, d.feature_out, d.pos_deform, d.shs_deform, d.dino_head)
    assert lean[1] is None and lean[2] is None and lean[0].shape == (40, 3)
    np.testing.assert_allclose(lean[0].cpu().numpy(), full[0].cpu().numpy(), rtol=2e-5, atol=2e-5)
    assert deform_mlp(x.requires_grad_(True), d.feature_out, d.pos_deform, d.shs_deform, None, need_dx=False, need_dshs=False) == (None,) * 3
