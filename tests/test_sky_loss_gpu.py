"""s3g_sky_loss (sky.sky_opacity_loss, sky.sky_loss_raw): value and d/dA against the float64 restatement of tests/alpha_ref.py.

Bar: four times the error of the SAME restatement evaluated in float32 on the CPU, measured here, and nothing else.  (On these
inputs that is 7e-8 ... 2e-7 rel-L2 for the gradient image -- at or below one fp32 ulp -- which the kernel meets because it forms
each gradient in double and rounds it once: 1.5e-8 ... 2.9e-8 on an MI355X; the value bars are 2e-7 ... 5e-4.)"""
import pytest
import torch

from tests import alpha_ref as R
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

SHAPES = [(13, 11), (29, 37), (48, 64), (500, 600)]     # < one workgroup's 1024 pixels; 1073 = 1024 + 49; 3 x 1024; 293 partials (> 256)


def _rel(x, ref):
    return abs(float(x) - float(ref)) / abs(float(ref))


def _bars(a, s):
    """(value bar, gradient bar, float64 loss, float64 gradient)"""
    l64, g64 = R.sky_loss_ref(a, s, torch.float64)
    l32, g32 = R.sky_loss_ref(a, s, torch.float32)
    return (4 * _rel(l32, l64), 4 * rel_l2(g32.numpy(), g64.numpy()), l64, g64)


@pytest.mark.parametrize("H,W", SHAPES)
def test_value_and_gradient_against_float64(gpu_device, H, W):
    from s3gaussian_amd import sky
    a, s = R.sky_inputs(H, W, seed=H)
    bar_v, bar_g, l64, g64 = _bars(a, s)
    for mask in (s, s[None]):                                # [H,W] and [1,H,W]
        loss, grad, _ = sky.sky_loss_raw(a.to(gpu_device), mask.to(gpu_device), 1.0)
        ev, eg = _rel(loss.cpu(), l64), rel_l2(grad.cpu().numpy(), g64.numpy())
        print(f"sky_loss {H}x{W}: value err {ev:.3e} (bar {bar_v:.3e}), gradient err {eg:.3e} (bar {bar_g:.3e})")
        assert loss.dtype == torch.float32 and grad.shape == (H, W)
        assert ev <= bar_v and eg <= bar_g
        outside = (a.double() < R.LO) | (a.double() > R.HI)
        assert outside.any() and (grad.cpu()[outside] == 0).all()         # the clamp passes no gradient, as torch.clamp


def test_weight_scales_value_and_gradient(gpu_device):
    from s3gaussian_amd import sky
    a, s = R.sky_inputs(29, 37, seed=1)
    bar_v, bar_g, l64, g64 = _bars(a, s)
    w = float(torch.tensor(0.05))                           # the weight the C ABI receives: a float
    loss, grad, _ = sky.sky_loss_raw(a.to(gpu_device), s.to(gpu_device), w)
    ev, eg = _rel(loss.cpu(), w * l64), rel_l2(grad.cpu().numpy(), w * g64.numpy())
    print(f"sky_loss weight {w}: value err {ev:.3e} (bar {bar_v:.3e}), gradient err {eg:.3e} (bar {bar_g:.3e})")
    assert ev <= bar_v and eg <= bar_g


def test_bit_identical_run_to_run(gpu_device):
    from s3gaussian_amd import sky
    a, s = R.sky_inputs(500, 600, seed=2)
    a, s = a.to(gpu_device), s.to(gpu_device)
    first = sky.sky_loss_raw(a, s, 0.3)
    for _ in range(3):
        again = sky.sky_loss_raw(a, s, 0.3)
        assert torch.equal(again[0], first[0]) and torch.equal(again[1], first[1]) and torch.equal(again[2], first[2])


def test_three_views_are_the_mean_over_the_concatenation(gpu_device):
    from s3gaussian_amd import sky
    dev = gpu_device
    views = [R.sky_inputs(29, 37, seed=10 + v) for v in range(3)]
    cat_a, cat_s = torch.cat([a for a, _ in views]), torch.cat([s for _, s in views])
    bar_v, bar_g, l64, g64 = _bars(cat_a, cat_s)
    alphas = [a[None].to(dev).requires_grad_(True) for a, _ in views]
    w = float(torch.tensor(0.75))                           # exact in fp32, and so is w / 3
    loss = sky.sky_opacity_loss(alphas, [s.to(dev) for _, s in views], w)
    assert loss.shape == () and loss.dtype == torch.float32
    (2.0 * loss).backward()                                  # the upstream scalar scales the stored gradient images
    assert _rel(loss.detach().cpu(), w * l64) <= bar_v
    got = torch.cat([x.grad[0].cpu() for x in alphas])
    assert alphas[0].grad.shape == (1, 29, 37)
    eg = rel_l2(got.numpy(), 2.0 * w * g64.numpy())
    print(f"sky_loss three views: gradient err {eg:.3e} (bar {bar_g:.3e})")
    assert eg <= bar_g
    # one view through the same door, and a result dict as the source
    one = sky.sky_opacity_loss({"alpha": views[0][0].to(dev)}, views[0][1].to(dev), 1.0)
    assert torch.equal(one.reshape(1), sky.sky_loss_raw(views[0][0].to(dev), views[0][1].to(dev), 1.0)[0])


def test_refuses_cpu_tensors_and_mismatched_masks(gpu_device):
    from s3gaussian_amd import sky
    a, s = R.sky_inputs(13, 11)
    with pytest.raises(RuntimeError, match="GPU"):
        sky.sky_opacity_loss(a, s)
    with pytest.raises(RuntimeError, match="does not match"):
        sky.sky_opacity_loss(a.to(gpu_device), s[:5].to(gpu_device))
    with pytest.raises(RuntimeError, match="one sky mask per"):
        sky.sky_opacity_loss([a.to(gpu_device)], [s, s])
