"""Bit-level checksums of whole training steps and of one evaluation render through the Python stack above the C ABI (pipeline.render /
training_step / training_step_views -> rasterizer nodes -> raster_C) -- one JSON line, so that two trees can be compared bit for bit
across processes (a refactor of that stack must print the same line):  python tools/step_checksum.py
Only public entry points; the cases are those of tests/step_ref.py and tests/step_ref_views.py (P = 4001, 128 x 96).  Runs with
hexplane.set_deterministic(True): the plane gradients' atomics aside, a step is bit-reproducible."""
import json
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from s3gaussian_amd import hexplane, synth  # noqa: E402
from s3gaussian_amd.pipeline import (GaussianParams, default_hyper, default_opt, render, training_step,  # noqa: E402
                                     training_step_views)
from tests import alpha_ref, step_ref as sr, step_ref_views as srv  # noqa: E402

LAMBDA_SKY = 0.05
dev = torch.device("cuda", 0)
hexplane.set_deterministic(True)


def bits(t):
    t = t.detach().contiguous()
    t = t.float() if t.dtype in (torch.bool, torch.float64) else t
    return int(t.view(torch.int32).to(torch.int64).sum())


def on_dev(d):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}


def pipe(**over):
    return SimpleNamespace(convert_SHs_python=True, compute_cov3D_python=False, debug=False, **over)


def load(case, lambda_sky=None):
    L = case["leaves"]
    opt = SimpleNamespace(**vars(case["opt"]), **({} if lambda_sky is None else {"lambda_sky": lambda_sky}))
    pc = GaussianParams(3, case["hyper"])
    pc.init_from_tensors(L["_xyz"], L["_scaling"], L["_rotation"], L["_opacity"], torch.cat([L["_features_dc"], L["_features_rest"]], 1), dev)
    pc._deformation.load_state_dict(case["state"])
    pc.training_setup(opt)
    return pc, opt


def summary(pc, loss, pkgs, grads):
    return {"loss": bits(loss.reshape(1)), "grads": grads, "params": {k: bits(p) for k, p in pc.named_parameters()},
            "stats": [bits(pc.xyz_gradient_accum), bits(pc.denom), bits(pc.max_radii2D)],
            "radii": [int(p["radii"].to(torch.int64).sum()) for p in pkgs]}


def hook_into(grads):
    def hook(pc, _pkgs):
        grads.update({k: bits(p.grad) for k, p in pc.named_parameters() if p.grad is not None})
    return hook


def step(name, pipe_=None, sky=False):
    case = sr.build_case(name)
    pc, opt = load(case, LAMBDA_SKY if sky else None)
    gt, gtd, gtf = (t.to(dev) for t in case["targets"])
    grads = {}
    kw = dict(sky_mask=alpha_ref.sky_mask_for(sr.H, sr.W).to(dev)) if sky else {}
    loss, pkg = training_step(pc, on_dev(case["camera"]), gt, gtd, gtf if case["stage"] == "fine" else None, case["hyper"], opt,
                              case["bg"].to(dev), stage=case["stage"], pipe=pipe_, grad_hook=hook_into(grads), densify_stats=True, **kw)
    return summary(pc, loss, [pkg], grads)


def step_views(name, sky=False):
    case = srv.build_case(name)
    pc, opt = load(case, LAMBDA_SKY if sky else None)
    gts = [tuple(t.to(dev) for t in tv) for tv in case["targets_views"]]
    V = len(gts)
    grads = {}
    kw = dict(sky_masks=[alpha_ref.sky_mask_for(sr.H, sr.W, seed=v).to(dev) for v in range(V)]) if sky else {}
    loss, pkgs = training_step_views(pc, [on_dev(c) for c in case["cameras"]], [g[0] for g in gts], [g[1] for g in gts],
                                     [g[2] for g in gts], case["hyper"], opt, case["bg"].to(dev), stage=case["stage"],
                                     grad_hook=hook_into(grads), densify_stats=True, **kw)
    return summary(pc, loss, pkgs, grads)


def library_model():
    """A grid_pe=2 network (the library deformation route), its heads off their zero initialisation."""
    scn = synth.street_scene(P=sr.P, seed=sr.SEED, width=sr.W, height=sr.H, n_frames=3)
    hyper, opt = default_hyper(kplanes_config=sr.PLANES["kplanes_config"], grid_pe=2), default_opt(lambda_dx=0.05, lambda_dshs=0.05)
    gs = scn["gaussians"]
    torch.manual_seed(0)
    pc = GaussianParams(3, hyper)
    pc.init_from_tensors(gs["xyz"], gs["log_scales"] + 0.9, gs["rotations_raw"], gs["opacity_logit"], gs["shs"], dev)
    pc._deformation.deformation_net.set_aabb(*scn["aabb"])
    with torch.no_grad():
        gen = torch.Generator().manual_seed(2)
        for p in pc._deformation.parameters():
            p.add_((0.05 * torch.randn(p.shape, generator=gen)).to(dev))
    pc.training_setup(opt)
    return scn, pc, hyper, opt


def step_views_library():
    scn, pc, hyper, opt = library_model()
    cams = [on_dev(scn["cameras"][i]) for i in (3, 4, 5)]
    g = torch.Generator().manual_seed(11)
    gts = [(torch.rand(3, sr.H, sr.W, generator=g).to(dev), (60 * torch.rand(1, sr.H, sr.W, generator=g)).to(dev),
            torch.rand(3, sr.H, sr.W, generator=g).to(dev)) for _ in cams]
    grads = {}
    loss, pkgs = training_step_views(pc, cams, [t[0] for t in gts], [t[1] for t in gts], [t[2] for t in gts], hyper, opt,
                                     scn["bg"].to(dev), pipe=pipe(), grad_hook=hook_into(grads), densify_stats=True)
    return summary(pc, loss, pkgs, grads)


def evaluation_render():
    case = sr.build_case("default")
    pc, _ = load(case)
    with torch.no_grad():
        out = render(on_dev(case["camera"]), pc, pipe(), case["bg"].to(dev), stage="fine", return_decomposition=True, return_alpha=True)
    keys = ("render", "depth", "alpha", "render_d", "depth_d", "render_s", "depth_s")
    return {"images": {k: bits(out[k]) for k in keys}, "radii": int(out["radii"].to(torch.int64).sum()), "keys": sorted(out.keys())}


out = {
    "step_default": step("default"),
    "step_coarse": step("coarse"),
    "step_default_two_nodes": step("default", pipe_=pipe(fused_pair=False)),
    "step_default_sky": step("default", sky=True),
    "views_rig": step_views("rig"),
    "views_mixed": step_views("mixed"),
    "views_rig_sky": step_views("rig", sky=True),
    "views_grid_pe": step_views_library(),
    "render_decomposition_alpha": evaluation_render(),
}
print(json.dumps(out, sort_keys=True))
