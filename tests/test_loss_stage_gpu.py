"""The strip-walking loss stage (csrc/ssim.hip; the separate per-pixel entry points and the combine: csrc/pixel_loss.hip): `ssim`
and `photometric_loss` at shapes that straddle every edge of the tiling, on impulse images, fused against the separate entry
points, and with poisoned output buffers.

Reference: oracle.hexplane_ref evaluated in float64 on the CPU.  Bar per tensor (the rule of test_optim_trajectory_gpu.py):
    max |gpu - f64| <= 4 x max |the same restatement in float32 on the CPU - f64| + one float32 ulp of the tensor's largest magnitude
(for the scalar value: the same with absolute differences).  g_depth and g_feat are zero exactly where the reference's are."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SW = 64          # strip width of a wave   (SS_SW of csrc/ssim.hip)
RH = 21          # output rows of a wave   (SS_RH); a workgroup's eight waves are eight strips, x fastest, so it spans RH rows too
W_SSIM, W_DEPTH, W_FEAT, SEED_GRAD = 0.2, 0.5, 0.001, 2.5

# (W, H, C): W from {1, 5, 6, 11, SW-1, SW, SW+1, 2 SW+5}, H from {1, 5, 6, 11, RH-1, RH, RH+1, 2 RH+1}, paired
SHAPES = [(1, 1, 1), (5, 11, 3), (6, 5, 3), (11, 6, 1), (SW - 1, RH + 1, 3), (SW, RH, 3), (SW + 1, RH - 1, 3),
          (2 * SW + 5, 2 * RH + 1, 3), (1, RH + 1, 3), (2 * SW + 5, 1, 1), (SW + 1, 2 * RH + 1, 1), (SW, 6, 3), (11, RH, 3)]


def _inputs(H, W, seed):
    """Inputs as in test_losses_gpu.py: seeded rand plus noise, depths that hit every mask and clamp branch."""
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(3, H, W, generator=g)
    gt = (img + 0.1 * torch.randn(3, H, W, generator=g)).clamp(0, 1)
    gdep = 100.0 * torch.rand(1, H, W, generator=g)          # below 0.01, inside, beyond max_depth (mask) ...
    gdep[0, ::7, ::5] = 0.0
    gdep[0, 0, 0] = 40.0                                     # (a 1 x 1 image keeps a pixel in the mask: an empty one gives NaN)
    dep = gdep + 30.0 * torch.randn(1, H, W, generator=g)    # ... predictions below 0 and above max_depth (clamp)
    ft, gft = torch.randn(3, H, W, generator=g), torch.randn(3, H, W, generator=g)
    return img, gt, dep, gdep, ft, gft


def _photometric_ref(hr, img, gt, dep, gdep, ft, gft):
    loss = hr.l1_loss(img[None], gt[None])
    if dep is not None:
        loss = loss + W_DEPTH * hr.depth_l2(dep[None], gdep[None])
    loss = loss + W_SSIM * (1.0 - hr.ssim(img[None], gt[None]))
    if ft is not None:
        loss = loss + W_FEAT * hr.l2_loss(ft, gft)
    return loss


def _run(fn, leaves, others):
    """fn(*tensors) -> scalar; returns (value, [gradients of the leaves])."""
    ls = [None if t is None else t.clone().requires_grad_(True) for t in leaves]
    v = fn(*ls, *others)
    (SEED_GRAD * v).backward()
    return v.detach(), [None if t is None else t.grad for t in ls]


def _check(name, gpu, ref64, ref32, report):
    gpu, ref64, ref32 = (np.asarray(t.detach().cpu().numpy(), np.float64) for t in (gpu, ref64, ref32))
    yard = float(np.max(np.abs(ref32 - ref64)))
    ulp = float(np.spacing(np.float32(np.max(np.abs(ref64)))))
    err = float(np.max(np.abs(gpu - ref64)))
    print(f"{name}: |gpu - f64| {err:.3e}   |f32 - f64| {yard:.3e}   ulp {ulp:.3e}   bar {4 * yard + ulp:.3e}")
    report.append((name, err, 4 * yard + ulp))


def _assert(report):
    bad = [(n, e, b) for n, e, b in report if not e <= b]
    assert not bad, bad


def _compare_ssim(dev, a, b, report, tag):
    from oracle import hexplane_ref as hr
    from s3gaussian_amd.losses import ssim
    f = lambda x, y: hr.ssim(x[None], y[None])
    v64, (g64,) = _run(f, [a.double()], [b.double()])
    v32, (g32,) = _run(f, [a], [b])
    vg, (gg,) = _run(lambda x, y: ssim(x[None], y[None]), [a.to(dev)], [b.to(dev)])
    _check(f"{tag} ssim value", vg, v64, v32, report)
    _check(f"{tag} ssim g_image", gg, g64, g32, report)


def _compare_photometric(dev, ins, report, tag):
    from oracle import hexplane_ref as hr
    from s3gaussian_amd.losses import photometric_loss
    img, gt, dep, gdep, ft, gft = ins
    f = lambda i, d, t, g, gd, gf: _photometric_ref(hr, i, g, d, gd, t, gf)
    d64 = lambda t: t.double()
    v64, g64 = _run(f, [d64(img), d64(dep), d64(ft)], [d64(gt), d64(gdep), d64(gft)])
    v32, g32 = _run(f, [img, dep, ft], [gt, gdep, gft])
    to = lambda t: t.to(dev)
    fg = lambda i, d, t, g, gd, gf: photometric_loss(i, g, d, gd, t, gf, lambda_dssim=W_SSIM, lambda_depth=W_DEPTH, lambda_feat=W_FEAT)
    vg, gg = _run(fg, [to(img), to(dep), to(ft)], [to(gt), to(gdep), to(gft)])
    _check(f"{tag} photometric value", vg, v64, v32, report)
    for name, a, b, c in zip(("g_image", "g_depth", "g_feat"), gg, g64, g32):
        _check(f"{tag} photometric {name}", a, b, c, report)
    for name, a, b in (("g_depth", gg[1], g64[1]), ("g_feat", gg[2], g64[2])):
        assert torch.equal(a.cpu() == 0, b == 0), f"{tag} {name}: zero pattern differs from the reference's"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "W%d_H%d_C%d" % s)
def test_seams_and_borders(gpu_device, shape):
    W, H, C = shape
    ins = _inputs(H, W, seed=1000 * H + W)
    report = []
    _compare_ssim(gpu_device, ins[0][:C], ins[1][:C], report, f"{shape}")
    _compare_photometric(gpu_device, ins, report, f"{shape}")
    _assert(report)


IMPULSE_HW = (2 * RH + 3, 2 * SW + 5)
IMPULSES = {"top_left": (0, 0), "top_right": (0, IMPULSE_HW[1] - 1), "bottom_left": (IMPULSE_HW[0] - 1, 0),
            "bottom_right": (IMPULSE_HW[0] - 1, IMPULSE_HW[1] - 1), "left_of_strip_seam": (17, SW - 1), "right_of_strip_seam": (17, SW),
            "above_row_seam": (RH - 1, 30), "below_row_seam": (RH, 30), "second_seams_corner": (2 * RH - 1, 2 * SW)}


@pytest.mark.parametrize("where", list(IMPULSES), ids=list(IMPULSES))
def test_impulse_images(gpu_device, where):
    """One nonzero pixel in the rendered image (all channels) over a black target: a halo one column or row short shows here."""
    H, W = IMPULSE_HW
    y, x = IMPULSES[where]
    _, _, dep, gdep, ft, gft = _inputs(H, W, seed=7)
    img, gt = torch.zeros(3, H, W), torch.zeros(3, H, W)
    img[:, y, x] = torch.tensor([1.0, 0.5, 0.25])
    report = []
    _compare_ssim(gpu_device, img, gt, report, where)
    _compare_photometric(gpu_device, (img, gt, dep, gdep, ft, gft), report, where)
    _assert(report)


@pytest.mark.parametrize("shape", [(SW + 1, RH - 1), (2 * SW + 5, 2 * RH + 1)], ids=lambda s: "W%d_H%d" % s)
def test_fused_launches_against_separate_entry_points(gpu_device, shape):
    """photometric_loss (two fused launches) against the same expression assembled from pixel_terms() and ssim() (the old entry
    points on the new core).  Every gradient is torch.equal: g_image is one float addition of the same two terms either way
    (the kernel forms ssim + l1, autograd's accumulation l1 + ssim or the reverse, and float addition commutes)."""
    from s3gaussian_amd.losses import photometric_loss, pixel_terms, ssim
    W, H = shape
    dev = gpu_device
    img, gt, dep, gdep, ft, gft = (t.to(dev) for t in _inputs(H, W, seed=H))
    fused = lambda i, d, t: photometric_loss(i, gt, d, gdep, t, gft, lambda_dssim=W_SSIM, lambda_depth=W_DEPTH, lambda_feat=W_FEAT)
    split = lambda i, d, t: (pixel_terms(i, gt, d, gdep, t, gft, w_l1=1.0, w_depth=W_DEPTH, w_feat=W_FEAT)
                             + W_SSIM * (1.0 - ssim(i[None], gt[None])))
    vf, gf = _run(fused, [img, dep, ft], [])
    vs, gs = _run(split, [img, dep, ft], [])
    for name, a, b in zip(("g_image", "g_depth", "g_feat"), gf, gs):
        assert torch.equal(a, b), (name, (a - b).abs().max().item())
    assert abs(vf.item() - vs.item()) < 5e-6 * max(1.0, abs(vs.item()))


def test_optional_pairs_and_poisoned_outputs(gpu_device, monkeypatch):
    """Missing pairs give None gradients as before, and every element of every output the kernels own is written: the maps and
    the gradient buffers are NaN-filled before the launches."""
    from s3gaussian_amd import losses
    monkeypatch.setattr(losses, "_new_grad", lambda t: torch.full_like(t, float("nan")))
    monkeypatch.setattr(losses, "_new_maps", lambda *a, **k: torch.full(*a, float("nan"), **k))
    dev = gpu_device
    W, H = 2 * SW + 5, RH + 1
    img, gt, dep, gdep, ft, gft = (t.to(dev) for t in _inputs(H, W, seed=3))
    kw = dict(lambda_dssim=W_SSIM, lambda_depth=W_DEPTH, lambda_feat=W_FEAT)
    cases = {"all": (dep, ft, kw), "no_depth_pair": (None, ft, kw), "no_feat_pair": (dep, None, kw),
             "zero_depth_weight": (dep, ft, dict(kw, lambda_depth=0.0))}
    for name, (d, t, k) in cases.items():
        f = lambda i, dd, tt: losses.photometric_loss(i, gt, dd, None if dd is None else gdep, tt, None if tt is None else gft, **k)
        v, (gi, gd, gf) = _run(f, [img, d, t], [])
        assert torch.isfinite(v).item() and torch.isfinite(gi).all().item(), name
        want_d = d is not None and k["lambda_depth"] != 0.0
        assert (gd is not None) == want_d and (gf is not None) == (t is not None), name
        assert gd is None or torch.isfinite(gd).all().item(), name
        assert gf is None or torch.isfinite(gf).all().item(), name
    v, (gi,) = _run(lambda i: losses.ssim(i[None], gt[None]), [img], [])
    assert torch.isfinite(v).item() and torch.isfinite(gi).all().item()
