"""Evaluation video frames on the GPU: s3gaussian_amd.frames.compose against the bytes the reference's own save_seperate_videos
handed to its writers (tests/golden/video_frames.npz) and against the numpy restatement (tests/frames_ref.py), and
pipeline.evaluate_video against strips restated from separate render() / render_flows / evaluate calls.

The bar is equality everywhere: every operation between the fp32 image and the byte is one correctly rounded fp32 operation (clip,
one multiply, for depths one division before them) or an integer one, and a maximum does not depend on the order of its operands."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import frames_ref as fr

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 5), (5, 8), (7, 64), (9, 67), (33, 260)]     # W % 4 != 0: byte path; 33 x 260: several workgroups in both passes
FILL = 0xA5
MARGIN = 64


@pytest.fixture(scope="module")
def fixture():
    return fr.load_fixture()


def _image(rng, C, H, W, normalize):
    if normalize:
        return rng.uniform(0.0, 50.0, size=(C, H, W)).astype(np.float32)
    return rng.uniform(-0.2, 1.2, size=(C, H, W)).astype(np.float32)


def _sources(img, dev):
    """The same image as an aligned contiguous tensor, as a [C,H,W] view that starts one float into a larger buffer (planes not
    16-byte aligned) and as a non-contiguous tensor (the binding makes it contiguous)."""
    t = torch.from_numpy(img).to(dev)
    buf = torch.zeros(t.numel() + 8, dtype=torch.float32, device=dev)
    buf[1:1 + t.numel()] = t.reshape(-1)
    view = buf[1:1 + t.numel()].view(t.shape)
    assert view.is_contiguous() and view.data_ptr() % 16 != 0
    wide = torch.zeros((t.shape[0], t.shape[1], 2 * t.shape[2] + 1), dtype=torch.float32, device=dev)
    wide[:, :, ::2][:, :, :t.shape[2]] = t
    strided = wide[:, :, ::2][:, :, :t.shape[2]]
    assert not strided.is_contiguous() or t.shape[2] == 1
    return {"aligned": t, "unaligned view": view, "non-contiguous": strided}


def _guarded_strip(H, W, C, n, dev, shift=0):
    """A strip inside a buffer filled with 0xA5, MARGIN + shift bytes in front and at least MARGIN behind; shift = 1 makes every
    destination address odd (byte path at any W)."""
    size = H * n * W * C
    buf = torch.full((MARGIN + shift + size + MARGIN,), FILL, dtype=torch.uint8, device=dev)
    return buf, buf[MARGIN + shift:MARGIN + shift + size].view(H, n * W, C)


@pytest.mark.parametrize("H,W", SHAPES)
def test_every_shape_tile_is_exact_and_nothing_else_is_touched(gpu_device, H, W):
    """Shapes x C x num_cams x every cam x three kinds of source x an aligned and an odd destination: the tile equals frames_ref,
    every byte outside the tile's columns and both margins keep their fill (W * C not a multiple of 4 included: a packed dword store at
    a tile edge would show here)."""
    from s3gaussian_amd import frames
    rng = np.random.default_rng(1000 * H + W)
    for C, normalize in ((3, False), (1, True), (1, False), (3, True)):
        img = _image(rng, C, H, W, normalize)
        want_tile = fr.tile(img, normalize)
        assert want_tile.shape == (H, W, C)
        for kind, src in _sources(img, gpu_device).items():
            for n in (1, 3):
                for cam in range(n):
                    for shift in (0, 1):
                        buf, strip = _guarded_strip(H, W, C, n, gpu_device, shift)
                        assert frames.strip_shape(H, W, C, n) == tuple(strip.shape)
                        out = frames.compose(src, strip, cam, normalize=normalize)
                        assert out is strip
                        want = np.full((H, n * W, C), FILL, np.uint8)
                        want[:, cam * W:(cam + 1) * W, :] = want_tile
                        got = buf.cpu().numpy()
                        where = (C, normalize, kind, n, cam, shift)
                        assert (got[:MARGIN + shift] == FILL).all() and (got[-MARGIN:] == FILL).all(), where
                        assert np.array_equal(got[MARGIN + shift:-MARGIN].reshape(H, n * W, C), want), where


def test_fixture_strips_equal_the_reference_recordings(gpu_device, fixture):
    """All seven keys, both sizes: one compose call per camera with one job per key, exactly the reference's recorded bytes."""
    from s3gaussian_amd import frames
    n, T = fr.NUM_CAMS, fr.NUM_TIMESTAMPS
    for (H, W), case in fixture.items():
        dev_in = {k: torch.from_numpy(case["inputs"][k]).to(gpu_device) for k in fr.KEYS}
        for t in range(T):
            strips = [torch.full(frames.strip_shape(H, W, 1 if k == "depths" else 3, n), FILL, dtype=torch.uint8, device=gpu_device)
                      for k in fr.KEYS]
            for cam in range(n):
                frames.compose([dev_in[k][t * n + cam] for k in fr.KEYS], strips, cam, normalize=[k == "depths" for k in fr.KEYS])
            for k, s in zip(fr.KEYS, strips):
                assert np.array_equal(s.cpu().numpy(), case["frames"][k][t]), (H, W, k, t)
                if t == T // 2:
                    assert np.array_equal(s.cpu().numpy(), case["middle"][k]), (H, W, k)


def test_to8b_of_one_image(gpu_device, fixture):
    from s3gaussian_amd import frames
    img = fixture[(6, 8)]["inputs"]["rgbs"][0]
    got = frames.to8b(torch.from_numpy(img).to(gpu_device))
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), fr.tile(img))
    with pytest.raises(RuntimeError, match=r"\[C,H,W\]"):
        frames.to8b(torch.zeros(2, 4, 4, device=gpu_device))


def test_depth_maximum_division_and_defined_corner_cases(gpu_device, fixture):
    from s3gaussian_amd import frames
    dev = gpu_device
    # the fixture's planted pixels: the byte x / m gives, which x * (1 / m) does not
    for (H, W), case in fixture.items():
        for d in case["inputs"]["depths"]:
            planted = fr.reciprocal_differs(d)
            assert planted.sum() >= 3
            mx = torch.zeros(1, device=dev)
            got = frames.compose(torch.from_numpy(d).to(dev), torch.zeros((H, W, 1), dtype=torch.uint8, device=dev), 0, normalize=True,
                                 maxima=mx).cpu().numpy()
            assert np.array_equal(got, fr.tile(d, True))
            wrong = fr.to8b(fr.normalise_depth(d, "reciprocal"))
            assert (got[planted] != wrong[planted]).all()
            assert mx.cpu().numpy().view(np.uint32)[0] == np.array(d.max(), np.float32).view(np.uint32)
    # the maximum in the first element, the last one and the middle, over several workgroups, aligned and not; twice: bit-identical
    rng = np.random.default_rng(77)
    H, W = 67, 132
    for place in (0, H * W - 1, (H * W) // 2 + 3):
        d = rng.uniform(4.0, 80.0, size=(1, H, W)).astype(np.float32)
        d.reshape(-1)[place] = np.float32(81.37)
        for kind, src in _sources(d, dev).items():
            mx = torch.zeros(2, device=dev)
            strips = [torch.zeros((H, W, 1), dtype=torch.uint8, device=dev) for _ in range(2)]
            frames.compose([src, src], strips, 0, normalize=[True, False], maxima=mx)
            again, mx2 = torch.zeros((H, W, 1), dtype=torch.uint8, device=dev), torch.zeros(1, device=dev)
            frames.compose(src, again, 0, normalize=True, maxima=mx2)
            assert torch.equal(strips[0], again) and torch.equal(mx[:1], mx2), (place, kind)
            assert float(mx[0]) == float(np.float32(81.37)) and float(mx[1]) == 0.0            # entry of a job without normalize: left alone
            assert np.array_equal(again.cpu().numpy(), fr.tile(d, True)), (place, kind)
            assert np.array_equal(strips[1].cpu().numpy(), fr.tile(d, False)), (place, kind)
    # an all-zero image, a negative one and one with a NaN maximum give all-zero tiles; a NaN pixel gives 0
    for H, W in ((5, 7), (6, 8)):
        for value in (0.0, -3.0):
            z = torch.full((1, H, W), value, device=dev)
            out = frames.compose(z, torch.full((H, W, 1), FILL, dtype=torch.uint8, device=dev), 0, normalize=True)
            assert int(out.max()) == 0
        img = rng.uniform(0.1, 0.9, size=(3, H, W)).astype(np.float32)
        want = fr.tile(img)
        img[1, H // 2, W - 1] = np.nan
        want[H // 2, W - 1, 1] = 0
        t = torch.from_numpy(img).to(dev)
        assert np.array_equal(frames.to8b(t).cpu().numpy(), want)
        mx = torch.zeros(1, device=dev)
        out = frames.compose(t, torch.full((H, W, 3), FILL, dtype=torch.uint8, device=dev), 0, normalize=True, maxima=mx)
        assert int(out.max()) == 0 and bool(torch.isnan(mx[0]))                             # numpy's max() of it is NaN, too
        assert np.isnan(img.max())


def test_eight_jobs_in_one_call_equal_eight_calls(gpu_device):
    from s3gaussian_amd import frames
    dev = gpu_device
    rng = np.random.default_rng(5)
    for H, W in ((9, 67), (12, 64)):
        chans = [3, 1, 3, 1, 3, 3, 1, 3]
        norm = [False, True, False, False, True, False, True, False]
        imgs = [torch.from_numpy(_image(rng, c, H, W, f)).to(dev) for c, f in zip(chans, norm)]
        n, cam = 3, 1
        before = frames.calls
        together = [torch.full(frames.strip_shape(H, W, c, n), FILL, dtype=torch.uint8, device=dev) for c in chans]
        mx = torch.zeros(8, device=dev)
        frames.compose(imgs, together, cam, normalize=norm, maxima=mx)
        assert frames.calls == before + 1
        for k in range(8):
            alone = torch.full(frames.strip_shape(H, W, chans[k], n), FILL, dtype=torch.uint8, device=dev)
            m1 = torch.zeros(1, device=dev)
            frames.compose(imgs[k], alone, cam, normalize=norm[k], maxima=m1)
            assert torch.equal(alone, together[k]) and float(m1[0]) == float(mx[k]), k
            want = np.full(alone.shape, FILL, np.uint8)
            want[:, cam * W:(cam + 1) * W] = fr.tile(imgs[k].cpu().numpy(), norm[k])
            assert np.array_equal(alone.cpu().numpy(), want), k
        with pytest.raises(RuntimeError, match="1..8"):
            frames.compose(imgs + imgs[:1], together + together[:1], cam)
    with pytest.raises(RuntimeError, match="1 or 3"):
        frames.compose(torch.zeros(2, 4, 4, device=dev), torch.zeros(4, 4, 2, dtype=torch.uint8, device=dev), 0)
    with pytest.raises(RuntimeError, match="strip 0"):
        frames.compose(torch.zeros(3, 4, 4, device=dev), torch.zeros(4, 12, 3, dtype=torch.uint8, device=dev), 3)
    with pytest.raises(RuntimeError, match="strip 0"):
        frames.compose(torch.zeros(3, 4, 4, device=dev), torch.zeros(4, 12, 3, dtype=torch.uint8, device=dev)[:, ::2], 0)


# ---- evaluate_video ------------------------------------------------------------------------------------------------------------------
P_SCENE, W_SCENE, H_SCENE = 2000, 96, 64


@pytest.fixture(scope="module")
def scene(gpu_device):
    """About 2 000 Gaussians, 96 x 64, 3 timestamps x 3 cameras, enlarged so that the small image is covered, with a position head that
    moves them (the scene of tests/test_flow_gpu.py), random ground-truth images and dynamic masks."""
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
    assert len(cams) == 9 and sorted({c["time"] for c in cams}) == [0.0, 0.5, 1.0]
    g = torch.Generator().manual_seed(21)
    gts = [torch.rand(3, H_SCENE, W_SCENE, generator=g).to(dev) for _ in range(10)]
    masks = [(torch.rand(H_SCENE, W_SCENE, generator=g) > 0.7).to(dev) for _ in range(10)]
    pipe = SimpleNamespace(convert_SHs_python=True, compute_cov3D_python=False, debug=False)
    return SimpleNamespace(pc=pc, cams=cams, gts=gts, masks=masks, pipe=pipe, bg=torch.tensor([0.1, 0.2, 0.3], device=dev), dev=dev)


@pytest.fixture(scope="module")
def restated(scene):
    """The strips of all seven keys restated with frames_ref from separate render(return_decomposition=True) calls and render_flows'
    lists, and evaluate()'s metrics -- computed once, left unchanged."""
    from s3gaussian_amd.pipeline import evaluate, render, render_flows
    s = scene
    images = {k: [] for k in fr.KEYS}
    with torch.no_grad():
        for i, cam in enumerate(s.cams):
            pkg = render(cam, s.pc, s.pipe, s.bg, return_decomposition=True)
            for k, name in (("rgbs", "render"), ("depths", "depth"), ("dynamic_rgbs", "render_d"), ("static_rgbs", "render_s")):
                images[k].append(pkg[name].cpu().numpy().copy())
            images["gt_rgbs"].append(s.gts[i].cpu().numpy())
    flows = render_flows(s.pc, s.cams, s.pipe, s.bg, num_cams=3)
    for k in ("forward_flows", "backward_flows"):
        images[k] = [img.cpu().numpy().copy() for img in flows[k]]
    strips = {k: [fr.strip(images[k][3 * t:3 * t + 3], normalize=(k == "depths")) for t in range(3)] for k in fr.KEYS}
    assert all(not np.array_equal(strips[k][0], strips[k][1]) for k in fr.KEYS)
    assert not np.array_equal(strips["dynamic_rgbs"][1], strips["static_rgbs"][1])
    metrics = evaluate(s.pc, s.cams, s.gts[:9], s.pipe, s.bg, masks=s.masks[:9])
    return SimpleNamespace(strips=strips, metrics=metrics, images=images)


def _counted(run):
    """Runs run() with pipeline.render and deformation.deform_infer counted."""
    from s3gaussian_amd import deformation, pipeline, raster_C
    raster_C.invalidate_geometry_cache()
    calls = {"render": 0, "infer": 0}
    real_render, real_infer = pipeline.render, deformation.deform_infer

    def render(*a, **k):
        calls["render"] += 1
        return real_render(*a, **k)

    def infer(*a, **k):
        calls["infer"] += 1
        return real_infer(*a, **k)

    pipeline.render, deformation.deform_infer = render, infer
    try:
        out = run()
    finally:
        pipeline.render, deformation.deform_infer = real_render, real_infer
    return out, calls


def _same_metrics(got, want):
    assert torch.equal(got["per_frame"], want["per_frame"])
    for k in ("psnr", "ssim", "masked_psnr", "masked_ssim"):
        assert got[k] == want[k], k


def test_evaluate_video_all_seven_keys_from_one_render_per_camera(scene, restated):
    from s3gaussian_amd import frames
    from s3gaussian_amd.pipeline import evaluate_video
    s = scene
    c0 = frames.calls
    res, calls = _counted(lambda: evaluate_video(s.pc, s.cams, s.gts[:9], s.pipe, s.bg, masks=s.masks[:9], num_cams=3, keys=fr.KEYS))
    assert calls == {"render": 9, "infer": 3}, calls            # three deformation evaluations for nine frames, one render each
    assert frames.calls - c0 == 9                               # one compose call per camera for all seven keys
    assert res["num_timestamps"] == 3 and sorted(res["frames"]) == sorted(fr.KEYS)
    for k in fr.KEYS:
        assert len(res["frames"][k]) == 3
        for t in range(3):
            got = res["frames"][k][t]
            assert got.is_cuda and got.dtype == torch.uint8
            assert np.array_equal(got.cpu().numpy(), restated.strips[k][t]), (k, t)
        assert torch.equal(res["middle"][k], res["frames"][k][1])
    _same_metrics(res, restated.metrics)


def test_evaluate_video_default_keys_sink_host_and_leftover_cameras(scene, restated):
    from s3gaussian_amd.pipeline import evaluate_video
    s = scene
    keys = ("gt_rgbs", "rgbs", "depths", "dynamic_rgbs", "static_rgbs")
    res, calls = _counted(lambda: evaluate_video(s.pc, s.cams, s.gts[:9], s.pipe, s.bg, masks=s.masks[:9]))
    assert calls == {"render": 9, "infer": 3}, calls
    assert tuple(res["frames"]) == keys
    for k in keys:
        for t in range(3):
            assert np.array_equal(res["frames"][k][t].cpu().numpy(), restated.strips[k][t]), (k, t)
    _same_metrics(res, restated.metrics)
    # sink: the same strips in (timestamp, key) order, nothing kept
    got = []
    back = evaluate_video(s.pc, s.cams, s.gts[:9], s.pipe, s.bg, masks=s.masks[:9], sink=lambda k, t, strip: got.append((t, k, strip)))
    assert [(t, k) for t, k, _ in got] == [(t, k) for t in range(3) for k in keys]
    assert all(back["frames"][k] == [] for k in keys)
    for t, k, strip in got:
        assert strip.is_cuda and torch.equal(strip, res["frames"][k][t]), (k, t)
    assert all(torch.equal(back["middle"][k], res["frames"][k][1]) for k in keys)
    _same_metrics(back, restated.metrics)
    # host: numpy arrays, through the pinned ring; with a sink (a view, copied here) and without
    host = evaluate_video(s.pc, s.cams, s.gts[:9], s.pipe, s.bg, masks=s.masks[:9], host=True, compute_metrics=False)
    assert host["psnr"] == -1 and host["per_frame"] is None
    seen = []
    hsink = evaluate_video(s.pc, s.cams, s.gts[:9], s.pipe, s.bg, masks=s.masks[:9], host=True,
                           sink=lambda k, t, strip: seen.append((t, k, strip.copy())))
    assert [(t, k) for t, k, _ in seen] == [(t, k) for t in range(3) for k in keys]
    for k in keys:
        for t in range(3):
            arr = host["frames"][k][t]
            assert isinstance(arr, np.ndarray) and arr.dtype == np.uint8 and np.array_equal(arr, restated.strips[k][t]), (k, t)
        assert np.array_equal(host["middle"][k], restated.strips[k][1]) and np.array_equal(hsink["middle"][k], restated.strips[k][1])
    for t, k, arr in seen:
        assert isinstance(arr, np.ndarray) and np.array_equal(arr, restated.strips[k][t]), (k, t)
    # ten cameras: three timestamps of strips, ten metric rows
    ten = evaluate_video(s.pc, s.cams + s.cams[:1], s.gts, s.pipe, s.bg, masks=s.masks)
    assert ten["num_timestamps"] == 3 and ten["per_frame"].shape == (10, 5)
    assert torch.equal(ten["per_frame"][:9], restated.metrics["per_frame"])
    for k in keys:
        assert len(ten["frames"][k]) == 3 and all(torch.equal(a, b) for a, b in zip(ten["frames"][k], res["frames"][k]))
        assert torch.equal(ten["middle"][k], res["frames"][k][1])


def test_evaluate_video_refusals(scene):
    from s3gaussian_amd.pipeline import evaluate_video
    s = scene
    args = (s.pc, s.cams, s.gts[:9], s.pipe, s.bg)
    with pytest.raises(RuntimeError, match="resize_five_views"):
        evaluate_video(*args, num_cams=5)
    with pytest.raises(RuntimeError, match="keys"):
        evaluate_video(*args, keys=("rgbs", "opacities"))
    with pytest.raises(RuntimeError, match="per camera"):
        evaluate_video(s.pc, s.cams, s.gts[:8], s.pipe, s.bg)
    with pytest.raises(RuntimeError, match=r"gt_images\[0\]"):
        evaluate_video(s.pc, s.cams, [g[:, :-1] for g in s.gts[:9]], s.pipe, s.bg, keys=("rgbs",))
    with pytest.raises(RuntimeError, match="fused deformation route"):
        evaluate_video(*args, keys=("rgbs", "dynamic_rgbs"), stage="coarse")
    with pytest.raises(RuntimeError, match="fused deformation route"):
        evaluate_video(s.pc, s.cams, s.gts[:9], SimpleNamespace(convert_SHs_python=True, fused_glue=False), s.bg,
                       keys=("forward_flows",))
    small = dict(s.cams[1])
    small["image_height"] = H_SCENE - 16
    with pytest.raises(RuntimeError, match="one strip holds images of one size"):
        evaluate_video(s.pc, [s.cams[0], small, s.cams[2]], [s.gts[0], s.gts[1][:, :-16], s.gts[2]], s.pipe, s.bg, keys=("rgbs",),
                       compute_metrics=False)
