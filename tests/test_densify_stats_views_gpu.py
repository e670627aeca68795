"""optim.densify_stats_views (csrc/densify_stats.hip::densify_stats_views_kernel): the densification statistics of a batch of V
views that share one optimizer step (train.py:387-388, 435-437, 489-493) in one pass, against optim.densify_stats applied to
what the reference forms first: the torch-summed viewspace gradient (`zeros + g0 + g1 ...`, left to right), any-visibility and
the stacked-max radii.  Same additions in the same order, same sqrt: the accumulators are bit-equal."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _case(P, V, seed, dev):
    g = torch.Generator().manual_seed(seed)
    grads = [torch.randn(P, 3, generator=g) for _ in range(V)]
    radii = [(torch.randint(0, 40, (P,), generator=g) * (torch.rand(P, generator=g) < 0.4)).to(torch.int32) for _ in range(V)]
    if P >= 4 and V >= 2:
        for v in range(V):
            radii[v][0] = 0                       # Gaussian 0: visible in no view (its gradients are not zero: they must not count)
            radii[v][1] = 17 if v == V - 1 else 0   # Gaussian 1: visible in the last view only
            radii[v][2] = 5 + v                   # Gaussian 2: visible in all, the largest radius is the last view's
    for v in range(V):                            # the rasterizer hands back a zero gradient for what a view does not see
        grads[v][radii[v] == 0] = 0.0
    if P >= 4 and V >= 2:
        grads[0][0] = 3.0
    acc = [torch.rand(P, 1, generator=g), torch.randint(0, 9, (P, 1), generator=g).float(), 30.0 * torch.rand(P, generator=g)]
    to = lambda l: [t.to(dev) for t in l]
    return to(grads), to(radii), to(acc)


def _reference(acc, grads, radii):
    from s3gaussian_amd import optim
    acc = [a.clone() for a in acc]
    total = torch.zeros_like(grads[0])
    for g in grads:
        total = total + g
    r = torch.stack(radii).max(dim=0).values
    vis = torch.stack([x > 0 for x in radii]).any(dim=0)
    optim.densify_stats(acc[0], acc[1], acc[2], total, r, visible=vis)
    return acc


@pytest.mark.parametrize("V", [1, 2, 3, 8])
@pytest.mark.parametrize("P", [0, 1, 255, 256, 257, 4001])
def test_batch_statistics_equal_single_view_statistics_of_the_summed_gradient(gpu_device, P, V):
    from s3gaussian_amd import optim
    grads, radii, acc = _case(P, V, 31 * V + P, gpu_device)
    want = _reference(acc, grads, radii)
    got = [a.clone() for a in acc]
    optim.densify_stats_views(got[0], got[1], got[2], grads, radii)
    for a, b, name in zip(got, want, ("xyz_gradient_accum", "denom", "max_radii2D")):
        assert torch.equal(a, b), name
    if P >= 4 and V >= 2:
        assert all(torch.equal(g[0], a[0]) for g, a in zip(got, acc))           # seen by no view: untouched, gradient or not
        assert float(got[1][1]) == float(acc[1][1]) + 1.0                         # seen by one view: counted once
        assert float(got[2][1]) == max(float(acc[2][1]), 17.0)
        assert float(got[1][2]) == float(acc[1][2]) + 1.0                         # seen by all V: still counted once
        assert float(got[2][2]) == max(float(acc[2][2]), 5.0 + V - 1)


def test_norm_of_the_sum_is_not_the_sum_of_norms(gpu_device):
    """What a per-view accumulation (the rasterizer's fused update, once per view) would give differs on this input by far more
    than rounding: the test above cannot be passed by it."""
    from s3gaussian_amd import optim
    grads, radii, acc = _case(4001, 3, 9, gpu_device)
    got = [a.clone() for a in acc]
    optim.densify_stats_views(got[0], got[1], got[2], grads, radii)
    per_view = [a.clone() for a in acc]
    for g, r in zip(grads, radii):
        optim.densify_stats(per_view[0], per_view[1], per_view[2], g, r)
    assert float((got[0] - per_view[0]).abs().max()) > 0.1 and float((got[1] - per_view[1]).abs().max()) >= 1.0
    assert torch.equal(got[2], per_view[2])                                           # the max is the max either way


def test_strided_gradients_and_refusals(gpu_device):
    from s3gaussian_amd import optim
    grads, radii, acc = _case(300, 2, 4, gpu_device)
    want = _reference(acc, grads, radii)
    wide = [torch.cat((g, torch.full((300, 2), float("nan"), device=gpu_device)), dim=1) for g in grads]   # [P,5]: columns 0, 1 used
    got = [a.clone() for a in acc]
    optim.densify_stats_views(got[0], got[1], got[2], wide, radii)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    with pytest.raises(RuntimeError, match="1 .. 8 views"):
        optim.densify_stats_views(got[0], got[1], got[2], grads * 5, radii * 5)
    with pytest.raises(RuntimeError, match="view 1"):
        optim.densify_stats_views(got[0], got[1], got[2], [grads[0], grads[1].cpu()], radii)
    with pytest.raises(RuntimeError, match="xyz_gradient_accum"):
        optim.densify_stats_views(got[0].cpu(), got[1], got[2], grads, radii)


def test_the_guarded_form_with_the_word_set_changes_nothing(gpu_device, monkeypatch):
    """densify_stats_views hands raster_C.async_skip_flag's word to s3g_densify_stats_views_guarded, as densify_stats does: set,
    the launch changes nothing (an asynchronous forward of the batch overflowed: its gradients are zeros, its radii are not);
    clear, it is the plain update."""
    from s3gaussian_amd import optim, raster_C
    dev = gpu_device
    grads, radii, acc = _case(4001, 3, 2, dev)
    word = torch.ones(1, dtype=torch.int32, device=dev)
    monkeypatch.setattr(raster_C, "async_skip_flag", lambda device=None: word)
    got = [a.clone() for a in acc]
    optim.densify_stats_views(got[0], got[1], got[2], grads, radii)
    assert all(torch.equal(a, b) for a, b in zip(got, acc))
    word.zero_()
    optim.densify_stats_views(got[0], got[1], got[2], grads, radii)
    monkeypatch.undo()
    assert all(torch.equal(a, b) for a, b in zip(got, _reference(acc, grads, radii)))
