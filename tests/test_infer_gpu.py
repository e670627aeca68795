"""Fused inference kernel HexPlane sampler (+) MLP heads (include/s3g_mlp.h::s3g_deform_infer) vs the two separate kernels it
replaces under torch.no_grad(): same arithmetic in the same order, so dx / dshs must be BIT-IDENTICAL; and through
pipeline.render() the image must not change.  (The two-kernel path itself is oracle-checked in test_hexplane_gpu.py,
test_mlp_gpu.py and at BASELINE size in test_parity_fullsize_gpu.py; scene/deformation.py:108-166.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture
def exact_chain(monkeypatch):
    """The bit-identity claims below are claims about the EXACT fp32 chain (training kernels and inference kernel share one
    arithmetic there); since round 6 both default to the split arithmetic (mlp.DEFAULT_ARITHMETIC, deformation.INFER_ARITHMETIC)."""
    import s3gaussian_amd.deformation as dm
    from s3gaussian_amd import mlp
    mlp.set_mlp_arithmetic("f32")
    monkeypatch.setattr(dm, "INFER_ARITHMETIC", "f32")
    yield
    mlp.set_mlp_arithmetic(mlp.DEFAULT_ARITHMETIC)


def _net(dev, aabb, seed=0):
    from s3gaussian_amd.deformation import deform_network
    from s3gaussian_amd.pipeline import default_hyper
    torch.manual_seed(seed)
    net = deform_network(default_hyper())
    net.deformation_net.set_aabb(*aabb)
    d = net.deformation_net
    with torch.no_grad():
        for p in d.grid.grids.parameters():
            p.add_(0.2 * torch.randn_like(p))
        for m in d.modules():
            if isinstance(m, torch.nn.Linear):
                torch.nn.init.normal_(m.bias, std=0.1)
    return net.to(dev).deformation_net


@pytest.mark.parametrize("tmode", ["uniform", "per_point"])
@pytest.mark.parametrize("P", [1, 7, 31, 32, 33, 255, 257, 5000, 70_001, 1_200_000])
def test_fused_inference_is_bit_identical_to_the_two_kernels(gpu_device, P, tmode, exact_chain):
    from s3gaussian_amd import synth
    from s3gaussian_amd.mlp import deform_infer, deform_mlp
    dev = gpu_device
    sc = synth.street_scene(P=max(P, 64), seed=1, n_frames=2)
    d = _net(dev, sc["aabb"], seed=P % 7)
    g = torch.Generator().manual_seed(P)
    xyz = sc["gaussians"]["xyz"][:P].to(dev).contiguous()
    xyz[::5] += (torch.rand(xyz[::5].shape, generator=g).to(dev) - 0.5) * torch.tensor([200.0, 80.0, 30.0], device=dev)   # some outside the aabb
    time = (torch.rand(P, 1, generator=g).to(dev) * 1.2 - 0.1) if tmode == "per_point" else torch.full((P, 1), 0.41, device=dev)
    ut = tmode == "uniform"
    with torch.no_grad():
        feats = d.grid(xyz, time, uniform_time=ut)
        dx0, dshs0, none = deform_mlp(feats, d.feature_out, d.pos_deform, d.shs_deform, d.dino_head, need_feat=False)
        assert none is None
        dx1, dshs1 = deform_infer(d.grid, xyz, time, d.feature_out, d.pos_deform, d.shs_deform, d.dino_head, uniform_time=ut)
        assert torch.equal(dx0, dx1) and torch.equal(dshs0, dshs1)
        if P >= 5000:   # and again in the blocked processing order a backward leaves behind
            with torch.enable_grad():
                x = xyz.clone().requires_grad_(True)
                d.grid(x, time, uniform_time=ut).sum().backward()
            assert d.grid._order_cache.get("order") is not None
            dx2, dshs2 = deform_infer(d.grid, xyz, time, d.feature_out, d.pos_deform, d.shs_deform, d.dino_head, uniform_time=ut)
            assert torch.equal(dx0, dx2) and torch.equal(dshs0, dshs2)


def _heads_fp64(d, feats):
    """The reference's Linear stacks (scene/deformation.py:53-76, 126-160) in fp64 on the fp32 features the sampler produced."""
    f = feats.double()
    lin = lambda m, x: x @ m.weight.double().t() + m.bias.double()
    hidden = lin(d.feature_out[0], f)
    h = torch.relu(hidden)
    dx = lin(d.pos_deform[3], torch.relu(lin(d.pos_deform[1], h)))
    dshs = lin(d.shs_deform[3], torch.relu(lin(d.shs_deform[1], h)))
    return dx, dshs


@pytest.mark.parametrize("tmode", ["uniform", "per_point"])
@pytest.mark.parametrize("P", [1, 33, 5000, 70_001, 1_200_000])
def test_split_bf16_inference_has_fp32_accuracy(gpu_device, P, tmode):
    """s3g_deform_infer_split: the GEMM layers on the bf16 matrix pipe with every operand split exactly into three bf16 pieces.  Its
    distance from the fp64 evaluation of the same layers must be that of the exact fp32 kernel (rounding noise of an fp32 chain),
    not that of a bf16 network (1e-2): both distances are measured here on the same inputs and recorded."""
    import json
    import os
    from s3gaussian_amd import synth
    from s3gaussian_amd.mlp import deform_infer
    dev = gpu_device
    sc = synth.street_scene(P=max(P, 64), seed=3, n_frames=2)
    d = _net(dev, sc["aabb"], seed=P % 5)
    with torch.no_grad():   # heads with outputs of order 1 (the default init of the last layers is tiny)
        for m in (d.pos_deform[3], d.shs_deform[3]):
            m.weight.mul_(30.0)
    g = torch.Generator().manual_seed(P + 1)
    xyz = sc["gaussians"]["xyz"][:P].to(dev).contiguous()
    time = (torch.rand(P, 1, generator=g).to(dev) * 1.2 - 0.1) if tmode == "per_point" else torch.full((P, 1), 0.63, device=dev)
    ut = tmode == "uniform"
    with torch.no_grad():
        feats = d.grid(xyz, time, uniform_time=ut)
        dx64, dshs64 = _heads_fp64(d, feats)
        args = (d.grid, xyz, time, d.feature_out, d.pos_deform, d.shs_deform, d.dino_head)
        dx_e, dshs_e = deform_infer(*args, uniform_time=ut)
        dx_s, dshs_s = deform_infer(*args, uniform_time=ut, arithmetic="bf16x3")
        again = [deform_infer(*args, uniform_time=ut, arithmetic="bf16x3") for _ in range(3)]
    out_s = torch.cat([dx_s, dshs_s], 1)
    bad_rows = sorted({int(r) for dx2, dshs2 in again for r in (torch.cat([dx2, dshs2], 1) != out_s).any(1).nonzero().flatten()[:64]})
    rel = lambda a, b: float((a.double() - b).norm() / b.norm().clamp_min(1e-300))
    mx = lambda a, b: float((a.double() - b).abs().max() / b.abs().max().clamp_min(1e-300))
    st = dict(what="deform_infer arithmetic", P=P, tmode=tmode, rows_that_differ_between_runs=bad_rows[:32],
              exact=dict(dx_rel_l2=rel(dx_e, dx64), dshs_rel_l2=rel(dshs_e, dshs64), dx_max=mx(dx_e, dx64), dshs_max=mx(dshs_e, dshs64)),
              bf16x3=dict(dx_rel_l2=rel(dx_s, dx64), dshs_rel_l2=rel(dshs_s, dshs64), dx_max=mx(dx_s, dx64), dshs_max=mx(dshs_s, dshs64)))
    os.makedirs("gpurun_out", exist_ok=True)
    with open("gpurun_out/infer_arithmetic_stats.jsonl", "a") as fh:
        fh.write(json.dumps(st) + "\n")
    assert not bad_rows, st          # deterministic: four runs, bit-identical
    for k in ("dx_rel_l2", "dshs_rel_l2"):
        assert st["bf16x3"][k] <= max(3.0 * st["exact"][k], 3e-7), st
    for k in ("dx_max", "dshs_max"):     # max error over the array, relative to its largest entry
        assert st["bf16x3"][k] <= max(4.0 * st["exact"][k], 1e-6), st


@pytest.mark.parametrize("tmode,launches", [("uniform", 1000), ("per_point", 200)])
def test_split_inference_is_bit_reproducible_1000_launches(gpu_device, tmode, launches):
    """The split kernel's staging store once read stale registers for the last quarter of a wave (packed-fp32 VALU result -> DS store
    data while the other wave of the SIMD issues bf16 MFMAs; csrc/deform_infer.hip, profiles/r04_split_hazard_isa.txt): two wrong rows about
    once per thousand (level, round) steps, different rows every launch -- ~800 rows per launch at 1.2 M points, which four launches
    catch only sometimes at small P.  The stress form: 1000 launches at BASELINE size, each compared with the first ON THE DEVICE, bit
    for bit (profiles/r04_split_hazard.jsonl: the unprotected build fails this with 110 872 wrong rows; the tree: 0).  The same
    1000 launches also stay within the fp32 tolerance of the exact kernel."""
    from s3gaussian_amd import synth
    from s3gaussian_amd.mlp import deform_infer
    dev = gpu_device
    P = 1_200_000
    sc = synth.street_scene(P=P, seed=3, n_frames=2)
    d = _net(dev, sc["aabb"], seed=2)
    xyz = sc["gaussians"]["xyz"].to(dev).contiguous()
    g = torch.Generator().manual_seed(9)
    time = (torch.rand(P, 1, generator=g).to(dev) * 1.2 - 0.1) if tmode == "per_point" else torch.full((P, 1), 0.63, device=dev)
    ut = tmode == "uniform"
    args = (d.grid, xyz, time, d.feature_out, d.pos_deform, d.shs_deform, d.dino_head)
    with torch.no_grad():
        exact = torch.cat(deform_infer(*args, uniform_time=ut), 1)
        first = torch.cat(deform_infer(*args, uniform_time=ut, arithmetic="bf16x3"), 1)
        wrong = torch.zeros((), dtype=torch.int64, device=dev)
        for _ in range(launches - 1):
            r = torch.cat(deform_infer(*args, uniform_time=ut, arithmetic="bf16x3"), 1)
            wrong += (r != first).any(1).sum()
        torch.cuda.synchronize()
    assert int(wrong) == 0, f"{int(wrong)} rows differed from the first launch over {launches} launches"
    assert float((first - exact).abs().max() / exact.abs().max()) < 5e-6


def test_render_uses_the_fused_inference_path_and_is_unchanged(gpu_device, monkeypatch, exact_chain):
    from types import SimpleNamespace
    import s3gaussian_amd.deformation as dm
    from s3gaussian_amd import synth
    from s3gaussian_amd.pipeline import GaussianParams, default_hyper, render
    dev = gpu_device
    scn = synth.street_scene(P=40_000, seed=2, width=320, height=208, n_frames=2)
    torch.manual_seed(0)
    pc = GaussianParams(3, default_hyper())
    gs = scn["gaussians"]
    pc.init_from_tensors(gs["xyz"], gs["log_scales"], gs["rotations_raw"], gs["opacity_logit"], gs["shs"], dev)
    pc._deformation.deformation_net.set_aabb(*scn["aabb"])
    with torch.no_grad():
        for p in pc._deformation.deformation_net.pos_deform.parameters():
            p.add_(0.05 * torch.randn_like(p))
    cam = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in scn["cameras"][1].items()}
    pipe = SimpleNamespace(convert_SHs_python=True, compute_cov3D_python=False, debug=False)
    calls = []
    real = dm.deform_infer
    monkeypatch.setattr(dm, "deform_infer", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with torch.no_grad():
        a = render(cam, pc, pipe, scn["bg"].to(dev), stage="fine", return_dx=True)
        assert len(calls) == 1
        monkeypatch.setattr(dm, "FUSED_INFERENCE", False)
        b = render(cam, pc, pipe, scn["bg"].to(dev), stage="fine", return_dx=True)
        assert len(calls) == 1
    for k in ("render", "depth", "radii", "dx", "dshs"):
        assert torch.equal(a[k], b[k]), k
    # with autograd on (training) or the feature image requested the fused path is not taken
    render(cam, pc, pipe, scn["bg"].to(dev), stage="fine", render_feat=True)
    with torch.no_grad():
        render(cam, pc, pipe, scn["bg"].to(dev), stage="fine", render_feat=True)
    assert len(calls) == 1


def test_render_with_split_arithmetic_is_the_same_picture(gpu_device, monkeypatch, exact_chain):
    """pipeline.render() with deformation.INFER_ARITHMETIC = "bf16x3": the deformation differs from the exact kernel's by fp32
    rounding noise, so the picture may differ only where a splat sits on a discrete threshold (radius rounding, alpha < 1/255)."""
    from types import SimpleNamespace
    import s3gaussian_amd.deformation as dm
    from s3gaussian_amd import synth
    from s3gaussian_amd.pipeline import GaussianParams, default_hyper, render
    dev = gpu_device
    scn = synth.street_scene(P=60_000, seed=4, width=320, height=208, n_frames=2)
    torch.manual_seed(1)
    pc = GaussianParams(3, default_hyper())
    gs = scn["gaussians"]
    pc.init_from_tensors(gs["xyz"], gs["log_scales"], gs["rotations_raw"], gs["opacity_logit"], gs["shs"], dev)
    pc._deformation.deformation_net.set_aabb(*scn["aabb"])
    with torch.no_grad():
        for p in pc._deformation.deformation_net.pos_deform.parameters():
            p.add_(0.05 * torch.randn_like(p))
        for p in pc._deformation.deformation_net.shs_deform.parameters():
            p.add_(0.02 * torch.randn_like(p))
    cam = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in scn["cameras"][1].items()}
    pipe = SimpleNamespace(convert_SHs_python=True, compute_cov3D_python=False, debug=False)
    with torch.no_grad():
        a = render(cam, pc, pipe, scn["bg"].to(dev), stage="fine", return_dx=True)
        monkeypatch.setattr(dm, "INFER_ARITHMETIC", "bf16x3")
        b = render(cam, pc, pipe, scn["bg"].to(dev), stage="fine", return_dx=True)
    assert not torch.equal(a["dx"], b["dx"])                                  # the other kernel really ran
    assert float((a["dx"] - b["dx"]).abs().max()) <= 2e-6 * float(a["dx"].abs().max()) + 1e-7
    diff = (a["render"] - b["render"]).abs()
    assert float(diff.mean()) < 1e-5 and float((diff > 1e-3).float().mean()) < 1e-4, (float(diff.mean()), float(diff.max()))
    assert float((a["radii"] != b["radii"]).float().mean()) < 1e-4


def test_the_cameras_of_one_timestamp_share_one_evaluation_of_the_deformation_field(gpu_device, monkeypatch):
    """VERDICT r5 next #5.  The deformation depends on (xyz, t), not on the camera; utils/video_utils.py:116-349 renders the cameras
    of one frame back to back.  Under no_grad the heads' outputs are kept keyed on (xyz, t, every parameter's version): the 2nd and
    3rd camera of a timestamp reuse them, bit-identical images; another timestamp, an optimizer step, an in-place edit of a parameter
    or of the returned dx, and raster_C.invalidate_geometry_cache() (the documented call after `.data` writes) all miss."""
    from types import SimpleNamespace
    import s3gaussian_amd.deformation as dm
    from s3gaussian_amd import raster_C, synth
    from s3gaussian_amd.pipeline import GaussianParams, default_hyper, default_opt, render
    dev = gpu_device
    scn = synth.street_scene(P=40_000, seed=3, width=320, height=208, n_frames=3)
    torch.manual_seed(0)
    pc = GaussianParams(3, default_hyper())
    gs = scn["gaussians"]
    pc.init_from_tensors(gs["xyz"], gs["log_scales"], gs["rotations_raw"], gs["opacity_logit"], gs["shs"], dev)
    pc._deformation.deformation_net.set_aabb(*scn["aabb"])
    with torch.no_grad():
        for p in pc._deformation.deformation_net.pos_deform.parameters():
            p.add_(0.05 * torch.randn_like(p))
    pc.training_setup(default_opt())
    cams = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in c.items()} for c in scn["cameras"]]
    assert cams[0]["time"] == cams[1]["time"] == cams[2]["time"] != cams[3]["time"]
    pipe = SimpleNamespace(convert_SHs_python=True, compute_cov3D_python=False, debug=False)
    bg = scn["bg"].to(dev)
    calls = []
    real = dm.deform_infer
    monkeypatch.setattr(dm, "deform_infer", lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    def frames(idx, **kw):
        with torch.no_grad():
            return [render(cams[i], pc, pipe, bg, stage="fine", return_dx=True, **kw) for i in idx]

    monkeypatch.setattr(dm, "INFER_CACHE", False)
    ref = frames(range(6))
    assert len(calls) == 6
    monkeypatch.setattr(dm, "INFER_CACHE", True)
    calls.clear()
    hits = dm.infer_cache_hits
    out = frames(range(6))
    assert len(calls) == 2 and dm.infer_cache_hits == hits + 4           # one evaluation per timestamp
    for a, b in zip(ref, out):
        for k in ("render", "depth", "radii", "dx", "dshs"):
            assert torch.equal(a[k], b[k]), k
    # decomposition renders (the evaluation path proper) and renders with the feature image go through the same entry
    d0 = frames([3], return_decomposition=True)[0]
    d1 = frames([4], return_decomposition=True)[0]
    assert len(calls) == 2 and torch.equal(d0["render"], out[3]["render"]) and torch.equal(d1["render_d"], frames([4], return_decomposition=True)[0]["render_d"])
    f0, f1 = frames([0, 1], render_feat=True)       # (two-kernel path: the training kernels' arithmetic, fp32-close to the fused kernel's)
    assert len(calls) == 2 and torch.allclose(f0["dx"], ref[0]["dx"], rtol=1e-5, atol=1e-6) and f1["feat"] is not None and f1["dx"] is f0["dx"]
    # what must miss
    n = len(calls)
    frames([0])
    assert len(calls) == n + 1                                            # (the entry held the feature-image form of timestamp 0)
    frames([1])
    assert len(calls) == n + 1
    with torch.no_grad():
        pc._deformation.deformation_net.pos_deform[3].bias.add_(1e-3)    # in-place edit of a parameter: version bump
    x = frames([2])[0]
    assert len(calls) == n + 2 and not torch.equal(x["dx"], ref[2]["dx"])
    x["dx"].mul_(2.0)                                                     # a consumer scribbles over what it was handed
    y = frames([0])[0]
    assert len(calls) == n + 3 and not torch.equal(y["dx"], x["dx"])
    pc._xyz.data.add_(0.01)                                               # no version bump: the documented invalidation call
    raster_C.invalidate_geometry_cache()
    z = frames([1])[0]
    assert len(calls) == n + 4 and not torch.equal(z["dx"], y["dx"])
    # a training step in between (autograd on: never cached; Adam bumps every version and drops the entry)
    from s3gaussian_amd.pipeline import training_step
    H, W = cams[0]["image_height"], cams[0]["image_width"]
    gts = (torch.rand(3, H, W, device=dev), torch.rand(1, H, W, device=dev) * 50, torch.rand(3, H, W, device=dev))
    training_step(pc, cams[0], *gts, default_hyper(), default_opt(), bg, stage="fine")
    assert "_infer_cache" not in pc._deformation.deformation_net.__dict__
    frames([1, 2])
    assert len(calls) == n + 5
