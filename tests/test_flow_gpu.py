"""Scene-flow colours and flow renders on the GPU: s3gaussian_amd.flow.scene_flow_colors against the reference's recorded colours
(tests/golden/scene_flow.npz) and the table-form restatement (tests/flow_ref.py), pipeline.render(extra_colors=...) against the
rasterizer called by hand, pipeline.render_flows against render(override_color=...) the way utils/video_utils.py:252-299 does it.

Colour bar: flow_ref.COLOR_BAR = 7.15e-07, four times the measured |restatement - reference| (tests/test_flow_cpu.py).
Image bar: 1e-4 abs, the project's bar for the fused against the unfused route (tests/test_reference_py_gpu.py); colours enter the
blend linearly with weights that sum to at most one."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import flow_ref as fr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture():
    return fr.load_fixture()


def _uniform_flow(P, seed, dev):
    """dx_a random, dx_b - dx_a uniform in a 0.01 wide range: rows on both sides of r = 1."""
    g = torch.Generator().manual_seed(seed)
    a = 0.05 * torch.randn(P, 3, generator=g)
    b = a + (0.01 * torch.rand(P, 3, generator=g) - 0.004)
    return a.to(dev), b.to(dev)


def test_colours_match_the_reference_at_every_fixture_size(gpu_device, fixture):
    from s3gaussian_amd.flow import scene_flow_colors
    cases, _, _ = fixture
    for c in cases:
        a, b = torch.from_numpy(c["dx_a"]).to(gpu_device), torch.from_numpy(c["dx_b"]).to(gpu_device)
        got, rng = scene_flow_colors(a, b, return_range=True)
        assert got.shape == a.shape and got.dtype == torch.float32
        dev = float(np.abs(got.cpu().numpy() - c["colors"]).max())
        print(f"{c['name']}: |kernel - reference| max {dev:.4e} (bar {fr.COLOR_BAR:.4e})")
        assert dev <= fr.COLOR_BAR, (c["name"], dev)
        assert rng.cpu().numpy().tolist() == [float(c["min"]), float(c["max"])], c["name"]


def test_zero_flow_is_exactly_white(gpu_device):
    from s3gaussian_amd.flow import scene_flow_colors
    a = torch.randn(777, 3, device=gpu_device)
    got, rng = scene_flow_colors(a, a.clone(), return_range=True)
    assert torch.equal(got, torch.ones_like(got)) and rng.tolist() == [0.0, 0.0]


def test_no_gaussians_give_an_empty_tensor(gpu_device):
    from s3gaussian_amd.flow import scene_flow_colors
    e = torch.empty(0, 3, device=gpu_device)
    got, rng = scene_flow_colors(e, e, return_range=True)
    assert got.shape == (0, 3) and got.is_cuda and rng.shape == (2,) and bool(torch.isnan(rng).all())
    assert scene_flow_colors(e, e).shape == (0, 3)


@pytest.mark.parametrize("P", [1, 63, 64, 65, 1025, 70_001])
def test_range_equals_torch_min_max_bit_for_bit(gpu_device, P):
    """The extreme value in the first element, in the last one and in the last element of a full workgroup trip (1024 floats: 256
    lanes x one 16-byte load); 70 001 Gaussians are 52 workgroups with a tail.  Each placement once as the maximum and once as the
    minimum, on 16-byte aligned tensors (wide loads) and on a view that starts 12 bytes into its allocation (scalar loads)."""
    from s3gaussian_amd.flow import scene_flow_colors
    n = 3 * P
    places = {"first": 0, "last": n - 1, "workgroup_end": (n // 1024) * 1024 - 1 if n >= 1024 else n - 1}
    base_a, base_b = _uniform_flow(P + 1, 11 + P, gpu_device)
    for aligned in (True, False):
        for name, k in places.items():
            for sign in (1.0, -1.0):
                if aligned:
                    a, b = base_a[:P].clone(), base_b[:P].clone()
                else:
                    a, b = base_a.clone()[1:], base_b.clone()[1:]
                    assert a.is_contiguous() and a.data_ptr() % 16 != 0
                a.view(-1)[k], b.view(-1)[k] = 0.0, sign * 5.0
                d = b - a
                want = torch.stack([d.min(), d.max()])
                got, rng = scene_flow_colors(a, b, return_range=True)
                assert torch.equal(rng, want), (aligned, name, sign, rng.tolist(), want.tolist())
                assert float(want[1] if sign > 0 else want[0]) == sign * 5.0
    if P == 70_001:     # multi-workgroup grid and tails of both passes: the colours against the table-form restatement
        a, b = base_a[:P].contiguous(), base_b[:P].contiguous()
        got = scene_flow_colors(a, b).cpu().numpy()
        ref = fr.colors(a.cpu().numpy(), b.cpu().numpy())
        r = np.hypot(*fr.normalise(a.cpu().numpy(), b.cpu().numpy())[:, :2].T)
        assert (r > 1).mean() > 0.05 and (r < 0.3).mean() > 0.02
        dev = float(np.abs(got - ref).max())
        print(f"P = {P}: |kernel - restatement| max {dev:.4e} (bar {fr.COLOR_BAR:.4e})")
        assert dev <= fr.COLOR_BAR, dev


def test_two_runs_are_bit_identical_and_out_is_written_in_place(gpu_device):
    from s3gaussian_amd.flow import scene_flow_colors
    a, b = _uniform_flow(70_001, 3, gpu_device)
    one, r1 = scene_flow_colors(a, b, return_range=True)
    out = torch.empty_like(a)
    two, r2 = scene_flow_colors(a, b, out=out, return_range=True)
    assert two is out and torch.equal(one, two) and torch.equal(r1, r2)
    with pytest.raises(RuntimeError, match="out must be"):
        scene_flow_colors(a, b, out=torch.empty(5, 3, device=gpu_device))


def test_strided_and_view_inputs_are_accepted(gpu_device):
    from s3gaussian_amd.flow import scene_flow_colors
    a, b = _uniform_flow(2 * 1000, 5, gpu_device)
    want, wr = scene_flow_colors(a[::2].contiguous(), b[::2].contiguous(), return_range=True)
    got, gr = scene_flow_colors(a[::2], b[::2], return_range=True)                      # strided rows
    assert torch.equal(got, want) and torch.equal(gr, wr)
    wide_a, wide_b = torch.zeros(1000, 7, device=gpu_device), torch.zeros(1000, 7, device=gpu_device)
    wide_a[:, 2:5], wide_b[:, 2:5] = a[::2], b[::2]
    got, gr = scene_flow_colors(wide_a[:, 2:5], wide_b[:, 2:5].double(), return_range=True)   # [P,3] view of a wider tensor, fp64
    assert torch.equal(got, want) and torch.equal(gr, wr)
    packed = torch.stack([a[::2], b[::2]])                                                # two [P,3] views of one allocation
    assert torch.equal(scene_flow_colors(packed[0], packed[1]), want)
    with pytest.raises(RuntimeError, match=r"\[P,3\]"):
        scene_flow_colors(a[:, :2], b[:, :2])


# ---- renders -------------------------------------------------------------------------------------------------------------------------
P_SCENE, W, H = 2000, 96, 64


@pytest.fixture(scope="module")
def scene(gpu_device):
    """About 2 000 Gaussians, 96 x 64, 3 timestamps x 3 cameras; enlarged so that the small image is covered, with a position head
    that moves them."""
    from s3gaussian_amd import synth
    from s3gaussian_amd.pipeline import GaussianParams, default_hyper
    dev = gpu_device
    scn = synth.street_scene(P=P_SCENE, seed=4, width=W, height=H, n_frames=3)
    gs = scn["gaussians"]
    torch.manual_seed(0)
    pc = GaussianParams(3, default_hyper())
    pc.init_from_tensors(gs["xyz"], gs["log_scales"] + math.log(12.0), gs["rotations_raw"], gs["opacity_logit"], gs["shs"], dev)
    pc._deformation.deformation_net.set_aabb(*scn["aabb"])
    with torch.no_grad():
        for p in pc._deformation.deformation_net.pos_deform.parameters():
            p.add_(0.05 * torch.randn_like(p))
        for p in pc._deformation.deformation_net.grid.grids.parameters():      # the time planes start at exactly 1: as they are,
            p.add_(0.2 * torch.randn_like(p))                                  # dx would not depend on the timestamp at all
    cams = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in cam.items()} for cam in scn["cameras"]]
    assert len(cams) == 9 and sorted({c["time"] for c in cams}) == [0.0, 0.5, 1.0]
    pipe = SimpleNamespace(convert_SHs_python=True, compute_cov3D_python=False, debug=False)
    return SimpleNamespace(pc=pc, cams=cams, pipe=pipe, bg=torch.tensor([0.1, 0.2, 0.3], device=dev), dev=dev)


def _by_hand(scene, cam, colors):
    """The rasterizer called directly on geometry tensors built the way render() builds them on the fused route."""
    from s3gaussian_amd.glue import activations_and_colors
    from s3gaussian_amd.pipeline import _uniform_time
    from s3gaussian_amd.rasterizer import GaussianRasterizationSettings, GaussianRasterizer
    pc = scene.pc
    dx, dshs, _ = pc._deformation.deformation_net.deform_heads(pc.get_xyz, _uniform_time(cam["time"], scene.dev), uniform_time=True,
                                                                need_feat=False)
    _, scales, rotations, opacity = activations_and_colors(pc.active_sh_degree, pc._features_dc, pc._features_rest, dshs, pc.get_xyz,
                                                           cam["campos"], pc._scaling, pc._rotation, pc._opacity)
    rs = GaussianRasterizationSettings(image_height=H, image_width=W, tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], bg=scene.bg,
                                       scale_modifier=1.0, viewmatrix=cam["viewmatrix"], projmatrix=cam["projmatrix"],
                                       sh_degree=pc.active_sh_degree, campos=cam["campos"], prefiltered=False, debug=False)
    means = pc.get_xyz + dx
    return GaussianRasterizer(raster_settings=rs)(means3D=means, means2D=torch.zeros_like(means), opacities=opacity,
                                                  colors_precomp=colors, scales=scales, rotations=rotations)[0]


def test_extra_colors_blend_on_the_frames_own_geometry(scene):
    from s3gaussian_amd import raster_C
    from s3gaussian_amd.pipeline import render
    g = torch.Generator().manual_seed(8)
    c1, c2 = (torch.rand(P_SCENE, 3, generator=g).to(scene.dev) for _ in range(2))
    cam = scene.cams[4]
    with pytest.raises(RuntimeError, match="no_grad"):
        render(cam, scene.pc, scene.pipe, scene.bg, extra_colors=[c1])
    with torch.no_grad():
        raster_C.invalidate_geometry_cache()
        plain = render(cam, scene.pc, scene.pipe, scene.bg)
        assert "extra" not in plain
        base = plain["render"].clone()
        raster_C.invalidate_geometry_cache()
        h0 = raster_C._geom_cache_hits
        out = render(cam, scene.pc, scene.pipe, scene.bg, extra_colors=[c1, c2])
        assert raster_C._geom_cache_hits == h0 + 2
        assert torch.equal(out["render"], base) and len(out["extra"]) == 2
        covered = (base - scene.bg[:, None, None]).abs().amax(0) > 1e-3
        assert covered.float().mean() > 0.1                                  # the small image is not mostly background
        hand = [_by_hand(scene, cam, c) for c in (c1, c2)]
        for img, want in zip(out["extra"], hand):
            assert img.shape == (3, H, W) and torch.equal(img, want)
        assert not torch.equal(hand[0], hand[1])
        dec = render(cam, scene.pc, scene.pipe, scene.bg, return_decomposition=True, extra_colors=[c2])
        assert torch.equal(dec["render"], base) and "render_d" in dec and torch.equal(dec["extra"][0], hand[1])
        with pytest.raises(RuntimeError, match="extra_colors"):
            render(cam, scene.pc, scene.pipe, scene.bg, extra_colors=[c1[:-1]])


@pytest.fixture(scope="module")
def flows(scene):
    """One render_flows run over the nine frames, with the deformation and colour evaluations counted."""
    from s3gaussian_amd import deformation, flow, raster_C
    from s3gaussian_amd.pipeline import render_flows
    raster_C.invalidate_geometry_cache()
    calls = {"infer": 0}
    real = deformation.deform_infer

    def counted(*a, **k):
        calls["infer"] += 1
        return real(*a, **k)

    deformation.deform_infer = counted
    try:
        e0, h0 = flow.evaluations, deformation.infer_cache_hits
        res = render_flows(scene.pc, scene.cams, scene.pipe, scene.bg, num_cams=3, with_rgb=True)
        counts = SimpleNamespace(infer=calls["infer"], colors=flow.evaluations - e0, hits=deformation.infer_cache_hits - h0)
    finally:
        deformation.deform_infer = real
    return res, counts


def test_render_flows_evaluates_each_timestamp_and_each_pair_once(flows):
    res, counts = flows
    assert counts.infer == 3, counts           # three timestamps: the nine frame renders all hit the inference cache
    assert counts.hits == 9, counts
    assert counts.colors == 2, counts          # (t0, t1) and (t1, t2)
    assert [len(res[k]) for k in ("forward_flows", "backward_flows", "rgbs")] == [9, 9, 9]
    for k in ("forward_flows", "backward_flows", "rgbs"):
        assert all(img.shape == (3, H, W) and img.is_cuda for img in res[k])


def test_render_flows_edge_frames_copy_the_other_list(flows):
    res, _ = flows
    for i in range(3):
        assert torch.equal(res["backward_flows"][i], res["forward_flows"][i])
    for i in range(6, 9):
        assert torch.equal(res["forward_flows"][i], res["backward_flows"][i])
    for i in range(3, 6):
        assert not torch.equal(res["forward_flows"][i], res["backward_flows"][i])


def test_render_flows_matches_override_color_renders_of_the_restated_colours(scene, flows):
    """What utils/video_utils.py:252-299 does: flow_visualizer on the host (tests/flow_ref.py), then render(override_color=...)."""
    from s3gaussian_amd.flow import frame_plan
    from s3gaussian_amd.pipeline import _uniform_time, render
    res, _ = flows
    pc = scene.pc
    net = pc._deformation.deformation_net
    forward, backward = frame_plan(9, 3)
    with torch.no_grad():
        dx = {}
        for cam in scene.cams:
            if cam["time"] not in dx:
                dx[cam["time"]] = net.deform_heads(pc.get_xyz, _uniform_time(cam["time"], scene.dev), uniform_time=True,
                                                   need_feat=False)[0].cpu().numpy().copy()
        t0, t1, t2 = sorted(dx)                  # the scene moves, and not by the same amount in both intervals
        assert np.abs(dx[t1] - dx[t0]).max() > 1e-3 and np.abs((dx[t2] - dx[t1]) - (dx[t1] - dx[t0])).max() > 1e-3
        worst = 0.0
        for kind, plan in (("forward_flows", forward), ("backward_flows", backward)):
            for i, p in enumerate(plan):
                c_ref = fr.colors(dx[scene.cams[p.from_frame]["time"]], dx[scene.cams[p.to_frame]["time"]])
                want = render(scene.cams[i], pc, scene.pipe, scene.bg, override_color=torch.from_numpy(c_ref).to(scene.dev))["render"]
                dev = float((res[kind][i] - want).abs().max())
                worst = max(worst, dev)
                assert dev <= 1e-4, (kind, i, dev)
                assert float((want - scene.bg[:, None, None]).abs().amax(0).gt(1e-3).float().mean()) > 0.1
        print(f"|render_flows - override_color render| max {worst:.4e} over 18 images")
        rgb = render(scene.cams[4], pc, scene.pipe, scene.bg)["render"]
        assert torch.equal(res["rgbs"][4], rgb)


def test_render_flows_sink_and_repeatability(scene, flows):
    from s3gaussian_amd.pipeline import render_flows
    res, _ = flows
    again = render_flows(scene.pc, scene.cams, scene.pipe, scene.bg, num_cams=3)
    assert "rgbs" not in again
    got = {}
    back = render_flows(scene.pc, scene.cams, scene.pipe, scene.bg, num_cams=3, sink=lambda kind, i, img: got.__setitem__((kind, i), img))
    assert back == {"forward_flows": [], "backward_flows": []}
    assert sorted(got) == sorted((kind, i) for kind in ("forward", "backward") for i in range(9))
    for i in range(9):
        for kind in ("forward", "backward"):
            assert torch.equal(res[f"{kind}_flows"][i], again[f"{kind}_flows"][i]), (kind, i)
            assert torch.equal(res[f"{kind}_flows"][i], got[(kind, i)]), (kind, i)
    with pytest.raises(ValueError):
        render_flows(scene.pc, scene.cams[:5], scene.pipe, scene.bg, num_cams=3)
