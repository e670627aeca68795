"""s3gaussian_amd.optim.Adam against a float64 Adam (tests/optim_ref.py) through every optimizer-state event of a training run,
at every kernel shape and alignment, through the guarded step and `rewind_to`, and with `p.data` re-pointed under a cached launch
record.

The bar, per tensor and each of p, m, v (optim_ref.compare):
    max |gpu - f64| <= 4 x max |torch.optim.Adam float32 on the CPU - f64| + one float32 ulp of the tensor's largest magnitude
and equal step counts.  tests/test_optim_ref_cpu.py shows that a float32 restatement of the kernel passes it and that each of seven
wrong readings of the host layer or the kernel lands 10x to 10^7x above it."""
import pytest
import torch

from tests import optim_ref as R

pytestmark = pytest.mark.gpu


def _check(name, dev):
    rows, bufs = R.gpu_rows(name, dev)
    print(f"{name}: largest gpu / cpu32 error ratio {R.largest_ratio(rows):.3g}, worst err / bar {R.worst_over_bar(rows):.3g}")
    assert all(r["ok"] for r in rows), f"{name}\n" + R.table(rows)
    return rows, bufs


@pytest.mark.parametrize("event", R.EVENTS)
def test_event_in_the_middle_of_a_trajectory(gpu_device, event):
    _check(event, gpu_device)


def test_all_events_in_one_trajectory(gpu_device):
    _check("all", gpu_device)


def test_kernel_shapes_in_one_launch(gpu_device):
    """numel 0 ... 1025 and one tensor just past the 2048-workgroup cap (a second and a short third pass of the grid-stride loop),
    one group, so one launch: the big tensor sizes the grid and the small tensors' rows of workgroups have nothing to do."""
    rows, _ = _check("shapes", gpu_device)
    assert {r["tensor"] for r in rows} == {f"n{n}" for n in R.SHAPE_NUMELS + (R.BIG_NUMEL,)}
    assert all(r["steps"] == [3.0, 3.0, 3.0] for r in rows if r["quantity"] == "step")


def test_each_pointer_in_turn_off_the_16_byte_boundary(gpu_device):
    """param, grad, exp_avg, exp_avg_sq in turn the only view at element offset 1, 2, 3 of a flat buffer (then all four, then none),
    numel % 4 in {0, 1, 2, 3}: to the bar, and the rest of every flat buffer bit-unchanged."""
    rows, bufs = _check("align", gpu_device)
    assert len({r["tensor"] for r in rows}) == 4 * (3 * 5 + 1)
    for (name, kind), buf in bufs.bufs.items():          # the views are where the test put them
        off, numel = bufs.live[(name, kind)]
        want = bufs.offsets[name][kind] % 4
        assert (buf[off:].data_ptr() // 4) % 4 == want and numel % 4 == int(name[-1]), (name, kind)
    assert bufs.untouched() == []


@pytest.mark.parametrize("case", ("shrink", "grow", "restride"))
def test_p_data_repointed_at_the_same_address(gpu_device, case):
    """The SAME Parameter, `p.data` moved from buf[:12] to buf[:8] (shrink), from buf[:8] to buf[:12] (grow), from a (6, 2) to a
    (4, 3) view (restride) of a flat buffer the test owns; moments and gradient are views into owned buffers of 12 + 16 elements
    as well, so a step over the old extent stays inside the test's memory.  The step must cover exactly the new extent, to the
    bar, in place, and leave everything else in the four buffers bit-unchanged."""
    rows, bufs = _check(f"repoint_{case}", gpu_device)
    assert bufs.live[("t", "param")][1] == {"shrink": 8, "grow": 12, "restride": 12}[case]
    assert bufs.untouched() == []


def test_moments_of_another_size_are_refused(gpu_device):
    from s3gaussian_amd.optim import Adam
    p = torch.nn.Parameter(torch.zeros(8, device=gpu_device))
    opt = Adam([p], lr=1e-3)
    p.grad = torch.ones_like(p)
    opt.step()
    opt.state[p]["exp_avg"] = torch.zeros(6, device=gpu_device)
    before = p.detach().clone()
    with pytest.raises(RuntimeError, match="exp_avg"):
        opt.step()
    assert torch.equal(p.detach(), before) and float(opt.state[p]["step"]) == 1.0


# ------------------------------------------------------------------------------------------------- guarded step, rewind_to

def _twin(dev, seed):
    """Parameters in two beta groups (two launches per step) and a run of prescribed gradients."""
    gen = torch.Generator().manual_seed(seed)
    shapes = [(67, 3), (1025,), (5, 1), (33,)]
    ps = [torch.nn.Parameter((torch.randn(s, generator=gen) * 1e-3).to(dev)) for s in shapes]
    from s3gaussian_amd.optim import Adam
    opt = Adam([dict(params=ps[:2], lr=1e-3, eps=1e-15), dict(params=ps[2:], lr=2e-3, betas=(0.8, 0.99), eps=1e-15)], lr=0.0)
    return ps, opt


def _grads(seed, n, dev, no_grad=()):
    gen = torch.Generator().manual_seed(seed)
    shapes = [(67, 3), (1025,), (5, 1), (33,)]
    return [[None if (it, k) in no_grad else (torch.randn(s, generator=gen) * 1e-2).to(dev) for k, s in enumerate(shapes)]
            for it in range(n)]


def _issue(ps, opt, grads):
    for p, g in zip(ps, grads):
        p.grad = g
    opt.step()


def _snapshot(ps, opt):
    out = []
    for p in ps:
        st = opt.state[p]
        out.append((p.detach().clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(), float(st["step"])))
    return out


def _same_bits(a, b, steps=True):
    for k, (x, y) in enumerate(zip(a, b)):
        for q in range(3):
            assert torch.equal(x[q].view(torch.int32), y[q].view(torch.int32)), (k, "pmv"[q])
        if steps:
            assert x[3] == y[3], (k, x[3], y[3])


@pytest.fixture
def skip_word(gpu_device, monkeypatch):
    """The device word `step()` hands to s3g_adam_step_guarded, owned by the test (restored afterwards)."""
    from s3gaussian_amd import raster_C
    word = torch.zeros(1, dtype=torch.int32, device=gpu_device)
    monkeypatch.setattr(raster_C, "async_skip_flag", lambda device=None: word)
    return word


@pytest.mark.parametrize("dropped,no_grad", [(1, ()), (2, ()), (1, ((3, 3),)), (2, ((3, 3), (4, 0)))],
                         ids=("one", "two_in_a_row", "one_without_a_gradient", "two_each_without_a_gradient"))
def test_guarded_step_dropped_then_rewound_equals_uninterrupted_twin(gpu_device, skip_word, dropped, no_grad):
    dev = gpu_device
    grads = _grads(7, 3 + dropped + 2, dev, no_grad)
    (pa, a), (pb, b) = _twin(dev, 5), _twin(dev, 5)
    for g in grads:                                   # the twin that is never interrupted
        _issue(pb, b, g)
    for g in grads[:3]:
        _issue(pa, a, g)
    before = _snapshot(pa, a)
    assert a.step_calls == 3
    skip_word.fill_(1)
    for g in grads[3:3 + dropped]:                    # dropped ON THE DEVICE
        _issue(pa, a, g)
    after = _snapshot(pa, a)
    _same_bits(before, after, steps=False)            # every p, m, v bit-identical
    for k, (x, y) in enumerate(zip(before, after)):   # ... while the host went on counting, per parameter
        stepped = sum((3 + d, k) not in no_grad for d in range(dropped))
        assert y[3] == x[3] + stepped, (k, x[3], y[3])
    assert a.step_calls == 3 + dropped and [c for c, _ in a._journal][-dropped:] == list(range(4, 4 + dropped))
    assert a.rewind_to(3) == dropped and a.step_calls == 3
    _same_bits(before, _snapshot(pa, a))              # the step counts are back as well
    skip_word.fill_(0)
    for g in grads[3:]:                               # the same iterations issued again
        _issue(pa, a, g)
    _same_bits(_snapshot(pb, b), _snapshot(pa, a))
    assert a.step_calls == b.step_calls == len(grads)


def test_guarded_step_with_the_word_clear_is_the_plain_step(gpu_device, skip_word):
    from s3gaussian_amd import raster_C
    grads = _grads(9, 3, gpu_device)
    (pa, a), (pb, b) = _twin(gpu_device, 6), _twin(gpu_device, 6)
    for g in grads:
        _issue(pa, a, g)
    with pytest.MonkeyPatch.context() as mp:          # no word at all: s3g_adam_step_guarded(..., NULL, ...)
        mp.setattr(raster_C, "async_skip_flag", lambda device=None: None)
        for g in grads:
            _issue(pb, b, g)
    _same_bits(_snapshot(pa, a), _snapshot(pb, b))
    assert int(skip_word.item()) == 0
