"""losses.photometric_loss_views: the image-space loss of a batch of V views as one node, against a float64 torch restatement of
train.py:389-425 on the CONCATENATED batch (oracle.hexplane_ref's l1_loss / ssim / depth_l2 / l2_loss, as tests/step_ref.py
uses them).  Tolerances are the single-view node's (tests/test_losses_gpu.py::test_photometric_loss_value_and_gradients), taken
over unchanged: value 5e-6 * max(1, |v|), image gradient rel-L2 1e-4, depth and feature gradients rel-L2 1e-5, the depth mask
exact -- per view, which is no weaker than over the batch.

H x W = 45 x 70 is ragged against the SSIM kernel's strips of 64 columns x 21 rows (two column strips, the second 6 wide; three
row strips, the last 3 high).  The views have very different counts of valid depth pixels, one has none: the reference's depth
term is the mean over the valid pixels of the whole batch, and a per-view reading is shown to be far outside the tolerance.

The public forms of the module share one node; the bit-for-bit tests below pin them against each other (a batch of one view is
photometric_loss, pixel_terms with every pair is photometric_loss without SSIM, plane_regulation_into is plane_regulation)."""
import pytest
import torch

from tests.util import rel_l2

pytestmark = pytest.mark.gpu
H, W, V = 45, 70, 3
W_SSIM, W_DEPTH, W_FEAT = 0.2, 0.5, 0.001
_CACHE = {}


def _batch():
    if "b" not in _CACHE:
        g = torch.Generator().manual_seed(45070)
        img = torch.rand(V, 3, H, W, generator=g)
        gt = (img + 0.1 * torch.randn(V, 3, H, W, generator=g)).clamp(0, 1)
        # depths straddle every branch (below 0.01, inside, beyond max_depth; predictions below 0 and above max); view 0 is valid
        # almost everywhere with small errors, view 1 on ~10 % of its pixels with large errors, view 2 nowhere
        gdep = 100.0 * torch.rand(V, 1, H, W, generator=g)
        gdep[0, 0, ::7, ::5] = 0.0
        gdep[1, 0][torch.rand(H, W, generator=g) > 0.1] = 0.0
        gdep[2] = 90.0 + gdep[2] / 10.0
        dep = gdep + torch.tensor([3.0, 40.0, 30.0]).view(V, 1, 1, 1) * torch.randn(V, 1, H, W, generator=g)
        ft, gft = torch.randn(V, 3, H, W, generator=g), torch.randn(V, 3, H, W, generator=g)
        _CACHE["b"] = (img, gt, dep, gdep, ft, gft)
    return _CACHE["b"]


def _reference(feat_views, w_ssim, w_depth, w_feat):
    """float64, on the concatenated batch; computed once per variant and shared."""
    key = (tuple(feat_views), w_ssim, w_depth, w_feat)
    if key not in _CACHE:
        from oracle import hexplane_ref as hr
        img, gt, dep, gdep, ft, gft = (t.double() for t in _batch())
        ri, rd, rf = (t.clone().requires_grad_(True) for t in (img, dep, ft))
        loss = hr.l1_loss(ri, gt)
        if w_depth != 0:
            loss = loss + w_depth * hr.depth_l2(rd, gdep)
        if w_ssim != 0:
            loss = loss + w_ssim * (1.0 - hr.ssim(ri, gt))
        if feat_views and w_feat != 0:
            sel = list(feat_views)
            loss = loss + w_feat * hr.l2_loss(rf[sel], gft[sel])
        (2.5 * loss).backward()
        _CACHE[key] = (float(loss.detach()), ri.grad, rd.grad, rf.grad)
    return _CACHE[key]


def _run(dev, feat_views, w_ssim, w_depth, w_feat):
    from s3gaussian_amd.losses import photometric_loss_views
    img, gt, dep, gdep, ft, gft = _batch()
    leaf = lambda t: t.clone().to(dev).requires_grad_(True)
    gi, gd = [leaf(img[v]) for v in range(V)], [leaf(dep[v]) for v in range(V)]
    gf = [leaf(ft[v]) if v in feat_views else None for v in range(V)]
    v = photometric_loss_views(gi, [gt[v].to(dev) for v in range(V)], gd, [gdep[v].to(dev) for v in range(V)], gf,
                               [gft[v].to(dev) if v in feat_views else None for v in range(V)],
                               lambda_dssim=w_ssim, lambda_depth=w_depth, lambda_feat=w_feat)
    (2.5 * v).backward()
    return v, gi, gd, gf


@pytest.mark.parametrize("case", ["last_feat", "all_feat", "no_feat", "no_ssim", "l1_only"])
def test_batch_loss_value_and_gradients_vs_float64_on_the_concatenation(gpu_device, case):
    feat_views = {"last_feat": (V - 1,), "all_feat": tuple(range(V)), "no_feat": (), "no_ssim": (V - 1,), "l1_only": ()}[case]
    w_ssim, w_depth, w_feat = W_SSIM, W_DEPTH, W_FEAT
    if case == "no_ssim":
        w_ssim = 0.0                        # the pixel-loss entry points instead of the fused SSIM pass
    if case == "l1_only":
        w_ssim = w_depth = w_feat = 0.0
    vr, ri, rd, rf = _reference(feat_views, w_ssim, w_depth, w_feat)
    vg, gi, gd, gf = _run(gpu_device, feat_views, w_ssim, w_depth, w_feat)
    print(f"{case}: loss {vg.item():.9g} float64 {vr:.9g}")
    assert abs(vg.item() - vr) < 5e-6 * max(1.0, abs(vr))
    for v in range(V):
        e = rel_l2(gi[v].grad.cpu().numpy(), ri[v].numpy())
        print(f"  view {v}: image gradient rel-L2 {e:.3g}")
        assert e < 1e-4, v
        if w_depth != 0:
            e = rel_l2(gd[v].grad.cpu().numpy(), rd[v].numpy())
            print(f"  view {v}: depth gradient rel-L2 {e:.3g}")
            assert e < 1e-5, v
            assert torch.equal(gd[v].grad.cpu() == 0, rd[v] == 0), v    # mask and clamp pass / stop exactly the same pixels
        else:
            assert gd[v].grad is None
        if v in feat_views and w_feat != 0:
            e = rel_l2(gf[v].grad.cpu().numpy(), rf[v].numpy())
            print(f"  view {v}: feature gradient rel-L2 {e:.3g}")
            assert e < 1e-5, v
    if w_depth != 0:
        assert float(gd[2].grad.abs().max()) == 0.0 and float(gd[1].grad.abs().max()) > 0.0     # the view without a valid pixel


def test_joint_depth_normalisation_is_not_the_mean_of_per_view_means():
    """On this batch the two readings of the depth term differ by orders of magnitude more than the value tolerance, and so do
    their gradients: a per-view normalisation cannot pass the test above."""
    from oracle import hexplane_ref as hr
    _, _, dep, gdep, _, _ = (t.double() for t in _batch())
    joint = float(hr.depth_l2(dep, gdep))
    counts = [int(((gdep[v] > 0.01) & (gdep[v] < 80.0)).sum()) for v in range(V)]
    assert counts[2] == 0 and counts[0] > 5 * counts[1] > 0, counts
    per_view = [float(hr.depth_l2(dep[v:v + 1], gdep[v:v + 1])) for v in range(V) if counts[v]]
    mean_of_means = sum(per_view) / len(per_view)
    total = _reference((V - 1,), W_SSIM, W_DEPTH, W_FEAT)[0]
    assert W_DEPTH * abs(joint - mean_of_means) > 1000 * 5e-6 * max(1.0, abs(total)), (joint, mean_of_means)
    # gradient of view 0's depth: 1/(n0 + n1) under the joint count, 1/(2 n0) under the mean of two per-view means
    assert abs((counts[0] + counts[1]) / (2.0 * counts[0]) - 1.0) > 1000 * 1e-5


def _value_and_grads(fn, leaves):
    ls = [None if t is None else t.clone().requires_grad_(True) for t in leaves]
    v = fn(*ls)
    (2.5 * v).backward()
    return v.detach(), [None if t is None else t.grad for t in ls]


def _assert_same_bits(a, b):
    (va, ga), (vb, gb) = a, b
    assert torch.equal(va, vb), (va.item(), vb.item())
    for k, (x, y) in enumerate(zip(ga, gb)):
        assert (x is None) == (y is None), k
        assert x is None or torch.equal(x, y), (k, (x - y).abs().max().item())


@pytest.mark.parametrize("with_feat", [True, False], ids=["feat", "no_feat"])
@pytest.mark.parametrize("w_ssim", [W_SSIM, 0.0], ids=["ssim", "no_ssim"])
def test_one_view_batch_is_the_single_view_loss_bit_for_bit(gpu_device, w_ssim, with_feat):
    """A batch of one view divides by 1 and by 1.0 where the single-view form does not divide: the same bits, value and gradients,
    and None for the same gradients."""
    from s3gaussian_amd.losses import photometric_loss, photometric_loss_views
    img, gt, dep, gdep, ft, gft = (t[0].to(gpu_device) for t in _batch())
    kw = dict(lambda_dssim=w_ssim, lambda_depth=W_DEPTH, lambda_feat=W_FEAT)
    leaves = [img, dep, ft if with_feat else None]
    tgt = lambda t: None if t is None else gft
    single = _value_and_grads(lambda i, d, t: photometric_loss(i, gt, d, gdep, t, tgt(t), **kw), leaves)
    batch = _value_and_grads(lambda i, d, t: photometric_loss_views([i], [gt], [d], [gdep], [t], [tgt(t)], **kw), leaves)
    assert (single[1][2] is not None) == with_feat and single[1][0] is not None and single[1][1] is not None
    _assert_same_bits(batch, single)


def test_pixel_terms_with_all_pairs_is_the_loss_without_ssim_bit_for_bit(gpu_device):
    from s3gaussian_amd.losses import photometric_loss, pixel_terms
    img, gt, dep, gdep, ft, gft = (t[0].to(gpu_device) for t in _batch())
    leaves = [img, dep, ft]
    terms = _value_and_grads(lambda i, d, t: pixel_terms(i, gt, d, gdep, t, gft, w_l1=1.0, w_depth=W_DEPTH, w_feat=W_FEAT), leaves)
    loss = _value_and_grads(lambda i, d, t: photometric_loss(i, gt, d, gdep, t, gft, lambda_dssim=0.0, lambda_depth=W_DEPTH,
                                                             lambda_feat=W_FEAT), leaves)
    assert all(g is not None for g in loss[1])
    _assert_same_bits(terms, loss)


def test_plane_regulation_into_writes_what_the_node_back_propagates(gpu_device):
    """plane_regulation_into (the gradient lands in the caller's views) against plane_regulation + backward with an upstream
    gradient of 1, on six planes of mixed sizes: one launch either way, the same value and gradients bit for bit."""
    from s3gaussian_amd.losses import plane_regulation, plane_regulation_into
    g = torch.Generator().manual_seed(6)
    sizes = [(2, 3), (3, 5), (5, 2), (2, 2), (5, 5), (3, 2)]
    planes = [torch.randn(1, 32, h, w, generator=g).to(gpu_device).contiguous(memory_format=torch.channels_last) for h, w in sizes]
    weights = (0.01, 0.0001, 0.0002)
    leaves = [p.clone().requires_grad_(True) for p in planes]
    v = plane_regulation([leaves], *weights)
    v.backward()
    views = [torch.full_like(p, float("nan")) for p in planes]
    vi = plane_regulation_into(planes, weights, views)
    assert torch.isfinite(v).item() and torch.equal(vi, v.detach()), (vi.item(), v.item())
    for k, (leaf, view) in enumerate(zip(leaves, views)):
        assert torch.equal(leaf.grad, view), k


def test_refusals(gpu_device):
    from s3gaussian_amd.losses import photometric_loss_views
    img, gt, *_ = _batch()
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        photometric_loss_views([img[0], img[1]], [gt[0], gt[1]])
    d = gpu_device
    with pytest.raises(RuntimeError, match="view 1 is 45x60"):
        photometric_loss_views([img[0].to(d), img[1, :, :, :60].to(d)], [gt[0].to(d), gt[1, :, :, :60].to(d)])
    with pytest.raises(RuntimeError, match="gt_images has 1 entries for 2 views"):
        photometric_loss_views([img[0].to(d), img[1].to(d)], [gt[0].to(d)])
