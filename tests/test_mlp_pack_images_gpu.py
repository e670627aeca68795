"""Which weight image each arithmetic of the deformation MLP packs.  A bf16x3 forward builds only the pre-split image its kernel reads
and leaves the slot of the fp32 image unwritten; a backward in another mode (f32, on-the-fly split) packs the fp32 image itself.
Stashes are pre-filled with NaN, so a kernel that read an unwritten image would show it in every output."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu


def _setup(dev, P, seed):
    from s3gaussian_amd import mlp
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(P, 128, generator=g) * 0.5).to(dev)
    params = [(torch.randn(*s, generator=g) * (0.2 if len(s) == 2 else 0.05)).to(dev) for s in mlp._SHAPES]
    g_dx, g_dshs, g_feat = (torch.randn(P, n, generator=g).to(dev) for n in (3, 48, 3))
    return x, params, g_dx, g_dshs, g_feat


def _forward(L, x, params, stash, save):
    from s3gaussian_amd import _lib, mlp
    P, dev = x.shape[0], x.device
    dx, dshs, feat = (torch.empty(P, n, device=dev) for n in (3, 48, 3))
    w = mlp._pack(params)
    _lib.check(L.s3g_deform_mlp_forward(C.byref(w), P, x.data_ptr(), dx.data_ptr(), dshs.data_ptr(), feat.data_ptr(), stash.data_ptr(),
                                        save, torch.cuda.current_stream().cuda_stream))
    return dx, dshs, feat


def _backward(L, x, params, stash, g_dx, g_dshs, g_feat):
    """ordered weight-gradient flush: every output is bit-reproducible"""
    from s3gaussian_amd import _lib, mlp
    P, dev = x.shape[0], x.device
    grads = [torch.zeros_like(p) for p in params]
    w, gw = mlp._pack(params), mlp._pack(grads)
    gx, ws = torch.empty_like(x), torch.empty(5, P, 64, device=dev)
    part = torch.empty(L.s3g_deform_mlp_wgrad_partial_bytes() // 4, device=dev)
    _lib.check(L.s3g_deform_mlp_backward_ordered(C.byref(w), P, x.data_ptr(), stash.data_ptr(), g_dx.data_ptr(), g_dshs.data_ptr(),
                                                 g_feat.data_ptr(), gx.data_ptr(), C.byref(gw), ws.data_ptr(), part.data_ptr(),
                                                 torch.cuda.current_stream().cuda_stream))
    return [gx, ws] + grads


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("P", [1, 33, 70_001])
def test_bf16x3_forward_and_backward_never_read_the_fp32_image(gpu_device, P):
    """Default arithmetic: a stash pre-filled with NaN and one pre-filled with zeros give bit-identical, finite outputs, activations,
    mask words and gradients."""
    from s3gaussian_amd import mlp
    L = mlp._bind()
    x, params, g_dx, g_dshs, g_feat = _setup(gpu_device, P, 11)
    n = L.s3g_deform_mlp_stash_bytes(P) // 4
    out = []
    try:
        mlp.set_mlp_arithmetic("bf16x3")
        for fill in (float("nan"), 0.0):
            stash = torch.full((n,), fill, device=gpu_device)
            fwd = _forward(L, x, params, stash, 1)
            bwd = _backward(L, x, params, stash, g_dx, g_dshs, g_feat)
            torch.cuda.synchronize()
            out.append(list(fwd) + [stash[L.s3g_deform_mlp_pack_bytes() // 4:].clone()] + bwd)
    finally:
        mlp.set_mlp_arithmetic(mlp.DEFAULT_ARITHMETIC)
    for a, b in zip(*out):
        assert torch.equal(_bits(a), _bits(b))
    for t in out[0][:3] + out[0][4:]:
        assert bool(torch.isfinite(t).all())


@pytest.mark.parametrize("P", [1, 33, 70_001])
@pytest.mark.parametrize("bwd_mode", ["f32", "bf16x3_onthefly"])
def test_a_backward_in_another_mode_packs_the_fp32_image_itself(gpu_device, P, bwd_mode):
    """bf16x3 forward into a NaN-filled stash, then the backward in a mode that reads the fp32 image: bit-identical to the same
    backward on a copy of the stash whose fp32 image an f32 forward (save_activations = 0: only the image is written) has packed."""
    from s3gaussian_amd import mlp
    L = mlp._bind()
    x, params, g_dx, g_dshs, g_feat = _setup(gpu_device, P, 12)
    pk = L.s3g_deform_mlp_pack_bytes() // 4
    try:
        mlp.set_mlp_arithmetic("bf16x3")
        stash_a = torch.full((L.s3g_deform_mlp_stash_bytes(P) // 4,), float("nan"), device=gpu_device)
        _forward(L, x, params, stash_a, 1)
        stash_b = stash_a.clone()
        mlp.set_mlp_arithmetic("f32")
        _forward(L, x, params, stash_b, 0)
        torch.cuda.synchronize()
        assert torch.equal(_bits(stash_a[pk:]), _bits(stash_b[pk:]))     # activations and mask words untouched
        mlp.set_mlp_arithmetic(bwd_mode)
        a = _backward(L, x, params, stash_a, g_dx, g_dshs, g_feat)
        b = _backward(L, x, params, stash_b, g_dx, g_dshs, g_feat)
        torch.cuda.synchronize()
    finally:
        mlp.set_mlp_arithmetic(mlp.DEFAULT_ARITHMETIC)
    for ta, tb in zip(a, b):
        assert torch.equal(_bits(ta), _bits(tb))
        assert bool(torch.isfinite(ta).all())
