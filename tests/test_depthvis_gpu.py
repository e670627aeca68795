"""GPU: the coloured depth frames (s3gaussian_amd/depthvis.py, csrc/depthvis.hip) against tests/depthvis_ref.py -- the weighted
percentiles to the last bit of the float64, the colours byte for byte -- against the reference's recorded bytes
(tests/golden/depthvis.npz), and behind pipeline.evaluate_video(depth_keys=("depth_colors",))."""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import depthvis_ref as dr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 7), (3, 5), (37, 53), (64, 64), (96, 144)]
POISON = 0xA5


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "depthvis.npz")))


def _bits(u32):
    return np.asarray(u32, dtype=np.uint32).view(np.float32)


def percentile_cases(H, W):
    """name -> (depth, alpha), fp32 [H,W]: every input of the issue's list at this shape."""
    n = H * W
    rng = np.random.default_rng(7000 + 1000 * H + W)
    w = lambda: rng.uniform(0.0, 1.0, n).astype(np.float32)
    distinct = rng.permutation(np.linspace(0.5, 150.0, n)).astype(np.float32)
    cases = {}
    cases["all_equal"] = (np.full(n, 7.5, np.float32), w())
    cases["two_values"] = (rng.choice([3.5, 77.25], n).astype(np.float32), w())
    cases["eight_values"] = (rng.choice(np.linspace(2.0, 90.0, 8), n).astype(np.float32), w())          # the group's first pixel decides
    cases["negative_and_positive"] = ((distinct - 60.0).astype(np.float32), w())
    cases["lowest_digit_only"] = (_bits(np.float32(10.0).view(np.uint32) + rng.integers(0, 256, n).astype(np.uint32)), w())
    cases["highest_digit_only"] = (_bits((rng.integers(0x3E, 0x46, n).astype(np.uint32) << 24) | np.uint32(0x00345678)), w())
    cases["all_weights_zero"] = (distinct, rng.choice([0.0, -1.0, np.nan], n).astype(np.float32))
    for name, at in (("single_weight_first", 0), ("single_weight_last", n - 1)):
        a = np.zeros(n, np.float32)
        a[at] = 0.75
        cases[name] = (distinct, a)
    m = min(n, 200)                       # 200 distinct depths of weight 1.0: q of p = 0.5 is S_0 exactly
    d = np.full(n, np.nan, np.float32)
    d[:m] = rng.permutation(np.linspace(1.0, 100.0, m)).astype(np.float32)
    cases["unit_weights_q_on_S0"] = (d, np.ones(n, np.float32))
    cases["tiny_and_full_opacities"] = (cases["eight_values"][0] if n > 8 else distinct,
                                        rng.choice([2.0 ** -31, 2.0 ** -32, 1.5 * 2.0 ** -30, 2.0 ** -29, 0.5, 1.0, 3.0], n).astype(np.float32))
    d = distinct.copy()
    d[rng.uniform(size=n) < 0.2] = np.nan
    cases["nan_depths_scattered"] = (d, w())
    cases["all_nan"] = (np.full(n, np.nan, np.float32), w())
    cases["negative_zero"] = (rng.choice(np.array([-0.0, 0.0, 1.0, -1.0], np.float32), n), w())
    cases["street"] = tuple(x.reshape(-1) for x in dr.street(H, W, 90 + H))
    return {k: (d.reshape(H, W), a.reshape(H, W)) for k, (d, a) in cases.items()}


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_percentiles_equal_the_restatement_to_the_last_bit(gpu_device, shape):
    from s3gaussian_amd import depthvis
    H, W = shape
    for name, (d, a) in percentile_cases(H, W).items():
        want = dr.weighted_percentiles(d, a)
        td, ta = torch.from_numpy(d).to(gpu_device), torch.from_numpy(a).to(gpu_device)
        got = depthvis.weighted_percentiles(td, ta)
        again = depthvis.weighted_percentiles(td[None], ta[None])
        assert got.dtype == torch.float64 and got.is_cuda and got.shape == (2,)
        assert torch.equal(got.view(torch.int64), again.view(torch.int64)), (name, got, again)          # two runs: the same bits
        g = got.cpu().numpy()
        print(f"{H}x{W} {name}: {g} (restatement {want})")
        assert np.array_equal(g, want, equal_nan=True), (name, g, want, g - want)
    if H * W >= 200:                                            # the case is what it says
        d, a = percentile_cases(H, W)["unit_weights_q_on_S0"]
        assert np.count_nonzero(~np.isnan(d)) == 200 and dr.weighted_percentiles(d, a)[0] == np.nanmin(d)


def test_full_grids_walk_by_stride(gpu_device):
    """600 x 901: more pixels than the 256 histogram workgroups and the 2048 colour workgroups (byte path) cover in one step, so
    every image-sized kernel walks by grid stride; percentiles of a tie-free and a tie-heavy frame, colours with automatic bounds."""
    from s3gaussian_amd import depthvis
    H, W = 600, 901
    d, a = dr.street(H, W, 77)
    q = (np.round(d / 8.0) * 8.0 + 1.0).astype(np.float32)
    td, ta, tq = (torch.from_numpy(x).to(gpu_device) for x in (d, a, q))
    for name, (x, tx) in (("street", (d, td)), ("quantised", (q, tq))):
        got = depthvis.weighted_percentiles(tx, ta).cpu().numpy()
        want = dr.weighted_percentiles(x, a)
        assert np.array_equal(got, want), (name, got, want)
    got = depthvis.depth_colors(td, ta, None, None).cpu().numpy()
    x = dr.u256(d, a, None, None)
    flagged = dr.near_step(x)
    want = dr.colors(d, a, None, None, depthvis.TABLE)
    differ = np.any(got != want, axis=-1)
    assert flagged.sum() <= 1e-5 * flagged.size and not (differ & ~flagged).any(), (int(flagged.sum()), int(differ.sum()))
    if differ.any():           # flagged pixels may sit one table step apart
        assert dr.steps_apart(got[differ], want[differ], depthvis.TABLE).max() <= 1


def test_percentile_refusals(gpu_device):
    from s3gaussian_amd import depthvis
    d = torch.rand(4, 6, device=gpu_device)
    with pytest.raises(RuntimeError, match="shape"):
        depthvis.weighted_percentiles(d, torch.rand(4, 5, device=gpu_device))
    with pytest.raises(RuntimeError, match="GPU"):
        depthvis.weighted_percentiles(d, torch.rand(4, 6))
    with pytest.raises(RuntimeError, match="2\\^23"):
        depthvis.weighted_percentiles(torch.empty(2048, 4097, device=gpu_device), torch.empty(2048, 4097, device=gpu_device))


# ---- colours -------------------------------------------------------------------------------------------------------------------------
def check_colors(got, depth, alpha, lo, hi, what):
    """The issue's rule: the restatement flags no pixel near a table step (asserted first), and then every byte is equal."""
    x = dr.u256(depth, alpha, lo, hi)
    assert not dr.near_step(x).any(), (what, int(dr.near_step(x).sum()))
    want = dr.colors(depth, alpha, lo, hi, dr_table())
    differ = np.any(got != want, axis=-1)
    assert not differ.any(), (what, int(differ.sum()), np.argwhere(differ)[:5], got[differ][:5], want[differ][:5], x[differ][:5])


def dr_table():
    from s3gaussian_amd import depthvis
    return depthvis.TABLE


def special_frame(H, W, seed):
    """A street frame with the values the curve and the weighting treat specially written into its first two rows' worth of pixels."""
    d, a = dr.street(H, W, seed)
    d, a = d.reshape(-1).copy(), a.reshape(-1).copy()
    vals = [0.0, -0.0, -3.0, -1e-6, np.inf, -np.inf, np.nan, 1e-30, 1e30]
    d[:len(vals)] = vals[:d.size]
    k = len(vals)
    if a.size > k + 8:
        a[k:k + 8] = [1.5, np.nan, np.inf, -0.2, 0.0, 1.0, 7.0, np.nan]
        a[1], a[6] = np.nan, 0.5
    return d.reshape(H, W), a.reshape(H, W)


BOUNDS = {"fixed": (4.0, 120.0), "reversed": (120.0, 4.0), "equal": (10.0, 10.0), "zero_lo": (0.0, 50.0), "auto": (None, None),
          "auto_lo": (None, 120.0), "auto_hi": (4.0, None)}


@pytest.mark.parametrize("kind", sorted(BOUNDS))
@pytest.mark.parametrize("shape", [(37, 53), (33, 52), (3, 5), (1, 4)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_colors_equal_the_restatement(gpu_device, shape, kind):
    """37 x 53 and 3 x 5 take the byte path, 33 x 52 and 1 x 4 the packed one (W % 4 == 0, aligned tensors); the 33 x 52 frame is also
    sent through the byte path from a misaligned copy, and both must give the same bytes.  Camera 0, 1 and 2 of a poisoned strip."""
    from s3gaussian_amd import depthvis
    H, W = shape
    lo, hi = BOUNDS[kind]
    for seed, (d, a) in ((1, dr.street(H, W, 300 + H)), (2, special_frame(H, W, 400 + H))):
        if (lo is None or hi is None) and seed == 2:
            d = np.where(np.isinf(d), np.float32(3.0), d)          # percentiles of infinite depths: not part of the contract's cases
        td, ta = torch.from_numpy(d).to(gpu_device), torch.from_numpy(a).to(gpu_device)
        for cam in range(3):
            strip = torch.full((H, 3 * W, 3), POISON, dtype=torch.uint8, device=gpu_device)
            back = depthvis.depth_colors(td, ta, lo, hi, out=strip, cam=cam, num_cams=3)
            assert back is strip
            got = strip.cpu().numpy()
            check_colors(got[:, cam * W:(cam + 1) * W], d, a, lo, hi, (shape, kind, seed, cam))
            outside = np.delete(got, np.s_[cam * W:(cam + 1) * W], axis=1)
            assert np.all(outside == POISON), (shape, kind, seed, cam)
        alone = depthvis.depth_colors(td[None], ta[None], lo, hi)
        assert alone.shape == (H, W, 3) and np.array_equal(alone.cpu().numpy(), got[:, 2 * W:])
        if W % 4 == 0:             # the same frame from storage that is 4 bytes off a 16-byte boundary: the byte path
            off_d = torch.empty(H * W + 1, device=gpu_device)[1:].view(H, W).copy_(td)
            off_a = torch.empty(H * W + 1, device=gpu_device)[1:].view(H, W).copy_(ta)
            assert off_d.data_ptr() % 16 == 4 and td.data_ptr() % 16 == 0
            assert torch.equal(depthvis.depth_colors(off_d, off_a, lo, hi), alone)


def test_colors_without_alpha_and_refusals(gpu_device):
    from s3gaussian_amd import depthvis
    for H, W in ((37, 53), (33, 52)):
        d, _ = special_frame(H, W, 500 + H)
        td = torch.from_numpy(d).to(gpu_device)
        got = depthvis.depth_colors(td)                       # lo = 4, hi = 120: the reference's depth_visualizer
        check_colors(got.cpu().numpy(), d, None, 4.0, 120.0, (H, W, "no alpha"))
    a = torch.rand(37, 53, device=gpu_device)
    with pytest.raises(RuntimeError, match="alpha=None needs both"):
        depthvis.depth_colors(td.new_zeros(37, 53), None, None, 120.0)
    with pytest.raises(RuntimeError, match="NaN bound"):
        depthvis.depth_colors(a, a, float("nan"), 120.0)
    with pytest.raises(RuntimeError, match="cam = 3"):
        depthvis.depth_colors(a, a, cam=3, num_cams=3)
    with pytest.raises(RuntimeError, match="out must be"):
        depthvis.depth_colors(a, a, out=torch.zeros(37, 53, 3, dtype=torch.uint8, device=gpu_device), num_cams=2)
    with pytest.raises(RuntimeError, match="shape"):
        depthvis.depth_colors(a, a[:, :-1])
    with pytest.raises(RuntimeError, match="GPU"):
        depthvis.depth_colors(a, a.cpu())


@pytest.mark.parametrize("kind", ["fixed", "auto"])
@pytest.mark.parametrize("name", ["s37x53", "s96x144"])
def test_colors_against_the_reference_bytes(gpu_device, golden, name, kind):
    """The fixture's frames against what the reference's own visualize_depth + to8b gave, on the CPU test's bars."""
    from s3gaussian_amd import depthvis
    assert np.array_equal(depthvis.TABLE, golden["table"])
    d, a = golden[f"{name}_depth"], golden[f"{name}_alpha"]
    lo, hi = (4.0, 120.0) if kind == "fixed" else (None, None)
    got = depthvis.depth_colors(torch.from_numpy(d).to(gpu_device), torch.from_numpy(a).to(gpu_device), lo, hi).cpu().numpy()
    dr.check_against_reference(got, golden, name, kind)
    check_colors(got, d, a, lo, hi, (name, kind))
    ref = golden[f"{name}_percentiles"]
    p = depthvis.weighted_percentiles(torch.from_numpy(d).to(gpu_device), torch.from_numpy(a).to(gpu_device)).cpu().numpy()
    assert np.all(np.abs(p - ref) / np.abs(ref) <= 4 * float(golden[f"{name}_percentile_rel"])), (p, ref)


# ---- evaluate_video ------------------------------------------------------------------------------------------------------------------
P_SCENE, W_SCENE, H_SCENE = 2000, 96, 64


@pytest.fixture(scope="module")
def scene(gpu_device):
    """The scene of tests/test_frames_gpu.py: about 2 000 Gaussians, 96 x 64, 3 timestamps x 3 cameras."""
    from s3gaussian_amd import synth
    from s3gaussian_amd.pipeline import GaussianParams, default_hyper
    dev = gpu_device
    scn = synth.street_scene(P=P_SCENE, seed=4, width=W_SCENE, height=H_SCENE, n_frames=3)
    gs = scn["gaussians"]
    torch.manual_seed(0)
    pc = GaussianParams(3, default_hyper())
    pc.init_from_tensors(gs["xyz"], gs["log_scales"] + math.log(12.0), gs["rotations_raw"], gs["opacity_logit"], gs["shs"], dev)
    pc._deformation.deformation_net.set_aabb(*scn["aabb"])
    with torch.no_grad():
        for p in pc._deformation.deformation_net.pos_deform.parameters():
            p.add_(0.05 * torch.randn_like(p))
        for p in pc._deformation.deformation_net.grid.grids.parameters():
            p.add_(0.2 * torch.randn_like(p))
    cams = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in cam.items()} for cam in scn["cameras"]]
    g = torch.Generator().manual_seed(21)
    gts = [torch.rand(3, H_SCENE, W_SCENE, generator=g).to(dev) for _ in range(9)]
    masks = [(torch.rand(H_SCENE, W_SCENE, generator=g) > 0.7).to(dev) for _ in range(9)]
    pipe = SimpleNamespace(convert_SHs_python=True, compute_cov3D_python=False, debug=False)
    return SimpleNamespace(pc=pc, cams=cams, gts=gts, masks=masks, pipe=pipe, bg=torch.tensor([0.1, 0.2, 0.3], device=dev), dev=dev)


@pytest.fixture(scope="module")
def without_key(scene):
    """evaluate_video without the depth key, and the depth / opacity images of render(return_alpha=True): computed once."""
    from s3gaussian_amd.pipeline import evaluate_video, render
    s = scene
    base = evaluate_video(s.pc, s.cams, s.gts, s.pipe, s.bg, masks=s.masks, keys=("rgbs", "depths"), sky_keys=("opacities",))
    with torch.no_grad():
        pkgs = [render(cam, s.pc, s.pipe, s.bg, return_alpha=True) for cam in s.cams]
    planes = [(p["depth"].clone(), p["alpha"].clone()) for p in pkgs]
    assert all(0.0 < float(a.mean()) for _, a in planes)
    return SimpleNamespace(base=base, planes=planes)


def _want_strips(planes, lo, hi):
    from s3gaussian_amd import depthvis
    strips = []
    for t in range(3):
        strip = torch.empty((H_SCENE, 3 * W_SCENE, 3), dtype=torch.uint8, device=planes[0][0].device)
        for c in range(3):
            depthvis.depth_colors(*planes[3 * t + c], lo, hi, out=strip, cam=c, num_cams=3)
        strips.append(strip)
    return strips


@pytest.mark.parametrize("bounds", [(4.0, 120.0), (None, None), (None, 120.0)], ids=["fixed", "auto", "auto_lo"])
def test_evaluate_video_depth_colors(scene, without_key, bounds):
    from s3gaussian_amd import depthvis, frames
    from s3gaussian_amd.pipeline import evaluate_video
    s, base = scene, without_key.base
    c0, f0 = depthvis.calls, frames.calls
    res = evaluate_video(s.pc, s.cams, s.gts, s.pipe, s.bg, masks=s.masks, keys=("rgbs", "depths"), sky_keys=("opacities",),
                         depth_keys=("depth_colors",), depth_bounds=bounds)
    assert depthvis.calls - c0 == 9 and frames.calls - f0 == 9
    assert tuple(res["frames"]) == ("rgbs", "depths", "opacities", "depth_colors") and res["num_timestamps"] == 3
    want = _want_strips(without_key.planes, *bounds)
    assert not torch.equal(want[0], want[1]) and len(torch.unique(want[1])) > 16              # a picture, not a constant
    for t in range(3):
        got = res["frames"]["depth_colors"][t]
        assert got.is_cuda and got.dtype == torch.uint8 and got.shape == (H_SCENE, 3 * W_SCENE, 3)
        assert torch.equal(got, want[t]), (t, int((got != want[t]).sum()))
    assert torch.equal(res["middle"]["depth_colors"], want[1])
    # the frame's bytes are the restatement's (camera 1 of timestamp 1), where it flags no pixel near a step
    d, a = (x.cpu().numpy() for x in without_key.planes[4])
    x = dr.u256(d, a, *bounds)
    if not dr.near_step(x).any():
        assert np.array_equal(want[1][:, W_SCENE:2 * W_SCENE].cpu().numpy(), dr.colors(d, a, *bounds, depthvis.TABLE))
    # every other strip and the metrics: as without the key
    for k in ("rgbs", "depths", "opacities"):
        assert all(torch.equal(x, y) for x, y in zip(res["frames"][k], base["frames"][k])), k
        assert torch.equal(res["middle"][k], base["middle"][k])
    assert torch.equal(res["per_frame"], base["per_frame"])
    for k in ("psnr", "ssim", "masked_psnr", "masked_ssim"):
        assert res[k] == base[k], k
    # host=True: the same bytes as numpy arrays; the depth key alone, through a sink
    host = evaluate_video(s.pc, s.cams, s.gts, s.pipe, s.bg, masks=s.masks, keys=("rgbs",), depth_keys=("depth_colors",),
                          depth_bounds=bounds, host=True, compute_metrics=False)
    for t in range(3):
        arr = host["frames"]["depth_colors"][t]
        assert isinstance(arr, np.ndarray) and arr.dtype == np.uint8 and np.array_equal(arr, want[t].cpu().numpy()), t
    assert np.array_equal(host["middle"]["depth_colors"], want[1].cpu().numpy())
    seen = []
    alone = evaluate_video(s.pc, s.cams, s.gts, s.pipe, s.bg, keys=(), depth_keys=("depth_colors",), depth_bounds=bounds,
                           compute_metrics=False, sink=lambda k, t, strip: seen.append((k, t, strip.clone())))
    assert [(k, t) for k, t, _ in seen] == [("depth_colors", t) for t in range(3)] and alone["frames"] == {"depth_colors": []}
    assert all(torch.equal(strip, want[t]) for _, t, strip in seen)


def test_evaluate_video_depth_key_refusals(scene):
    from s3gaussian_amd.pipeline import evaluate_video
    s = scene
    args = (s.pc, s.cams, s.gts, s.pipe, s.bg)
    with pytest.raises(RuntimeError, match="turbo_depths"):
        evaluate_video(*args, keys=("rgbs",), depth_keys=("turbo_depths",))
    with pytest.raises(RuntimeError, match=r"depth_colors.*depth_keys="):
        evaluate_video(*args, keys=("rgbs", "depth_colors"))
    with pytest.raises(RuntimeError, match="depth_keys must be distinct"):
        evaluate_video(*args, keys=("rgbs",), depth_keys=("depth_colors", "depth_colors"))
