"""One training step's loss and gradients by the reference's algorithm on the CPU, in float64 or float32: the checker of
`pipeline.training_step` tensor by tensor (tests/test_step_gradients_gpu.py); tests/test_step_gradients_cpu.py checks the checker.

TEST INFRASTRUCTURE ONLY.  It imports oracle/ and s3gaussian_amd.synth and nothing else of the product.  The chain is the one
tests/test_psnr_parity_gpu.py::oracle_step assembles -- oracle/hexplane_ref.py (HexPlane field, deformation heads, SH glue, losses,
plane regulariser; pinned by goldens of the reference's own modules) and the C rasterizer oracle forward / backward called twice
(RGB + depth, feature image), train.py:395-425 loss assembly -- evaluated ONCE, with no optimizer step, and returned per tensor
under the PRODUCT's parameter names.  With `dtype=torch.float64` every stage runs in double (liboracle_f64.so, modules .double()):
that is the reference value.  With float32 it is the same chain in the reference's own precision: the distance between the two is
the yardstick, the only thing the GPU bar is derived from (BAR_MARGIN x the largest per-tensor distance of the case).

`mutate` switches ONE seam of the step to a plausible wrong reading (MUTANTS).  At the reference's default weights several of them
move no tensor by more than the bar (tests/test_step_gradients_cpu.py records which); the `loud` case raises the weights of the
terms that ride on other nodes until every one of them lands far outside it.

Cases (build_case):
  default  fine stage, the reference's default loss weights and plane-regulariser weights
  loud     fine stage, lambda_feat = 1, lambda_dx = lambda_dshs = 0.05, l1_time_planes = plane_tv_weight = 0.01
  coarse   stage "coarse": no deformation, no regularisers, no feature image
P = 4001 leaves a ragged last block in every per-Gaussian kernel (block sizes 64 / 128 / 256)."""
import json
import os
from types import SimpleNamespace

import numpy as np
import torch

from oracle import hexplane_ref as hr
from oracle.oracle import RasterOracle
from s3gaussian_amd import synth

RECORD = os.environ.get("S3G_STEP_RECORD")     # record() appends to the file this names; unset: nothing is written
P, W, H, VIEW = 4001, 128, 96, 4
# Scene seed.  At P = 4001, seed 3 (the PSNR test's) puts ONE pixel on a blend skip test's threshold: the float32 and float64 chains
# take different sides there and every tensor downstream differs by 3e-4.  Such a pixel measures nothing about a gradient, so the
# scene is the next seed whose chains take the same side everywhere; the yardstick test asserts that they do.
SEED = 4
CASES = ("default", "loud", "coarse")
PLANES = dict(kplanes_config=dict(grid_dimensions=2, input_coordinate_dim=4, output_coordinate_dim=32, resolution=[16, 16, 16, 8]))
# OptimizationParams the step reads (arguments/__init__.py:100-158); tests/test_step_gradients_cpu.py holds it against pipeline.default_opt()
DEFAULT_OPT = dict(position_lr_init=0.00016, deformation_lr_init=0.000016, grid_lr_init=0.00016, feature_lr=0.0025, opacity_lr=0.05,
                   scaling_lr=0.005, rotation_lr=0.001, lambda_dssim=0.2, lambda_depth=0.5, lambda_feat=0.001, lambda_dx=0.001,
                   lambda_dshs=0.001)
LOUD_OPT = dict(lambda_feat=1.0, lambda_dx=0.05, lambda_dshs=0.05)
LOUD_HYPER = dict(l1_time_planes=0.01, plane_tv_weight=0.01)
YARDSTICK_MAX = 2.5e-5      # largest float32-chain distance from the float64 chain a case may show, over all its tensors
BAR_MARGIN = 4.0            # GPU bar = BAR_MARGIN x the case's yardstick <= 1e-4, the rasterizer-gradient bar of test_raster_gpu.py
LOSS_YARDSTICK_MAX = 1e-6   # largest relative distance of the float32 chain's loss from the float64 chain's
# |loss_gpu - loss_f64| / loss_f64 the GPU test allows.  The rule is 4 x the gap of the first run on the MI355X; until such a run is
# recorded in profiles/step_gradient_parity.jsonl (rows `gpu_step`: rel_loss_gap) the bar is formed like the per-tensor one, from the
# reference alone: BAR_MARGIN x the bound on the float32 chain's own loss error.  A tenth of the smallest loss shift of a wrong
# reading is 4.4e-4 (test_step_gradients_cpu.py asserts the factor of ten).
LOSS_BAR = {k: BAR_MARGIN * LOSS_YARDSTICK_MAX for k in ("default", "loud", "coarse", "loud_scale_1.7")}
# wrong reading -> does it change the reported loss?
MUTANTS = {
    "no_dx_l1": True,                 # lambda_dx * mean|dx| dropped (_WeightedTerms)
    "no_dshs_l1": True,               # lambda_dshs * mean|dshs| dropped (glue kernel, with_dshs_l1)
    "dshs_mean_over_16P": True,       # mean|dshs| divided by 16 P instead of 48 P
    "no_time_smoothness": True,       # the three plane weights, one at a time (render: reg_weights)
    "no_l1_time_planes": True,
    "no_plane_tv": True,
    "feat_loss_x2": True,
    "no_depth": True,
    "no_ssim": True,
    "sh_direction_detached": False,   # the SH view direction gives xyz no gradient
    "feat_pass_no_means3D": False,    # the feature image's backward contributes no dL/dmeans3D
    "feat_pass_no_opacity": False,    # ... no dL/dopacity
}
LEAVES = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity")


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def build_case(name):
    """-> dict: name, stage, scene, camera (CPU tensors), bg, targets (image, depth, feature image), opt, hyper, leaves (the six
    per-Gaussian tensors under the product's names) and state (the deformation network's state_dict: loads into the product's
    `_deformation` and into oracle.hexplane_ref.deform_network alike)."""
    if name not in CASES:
        raise KeyError(name)
    scn = synth.street_scene(P=P, seed=SEED, width=W, height=H, n_frames=3)
    gs = scn["gaussians"]
    opt, over = dict(DEFAULT_OPT), dict(PLANES)
    if name == "loud":
        opt.update(LOUD_OPT)
        over.update(LOUD_HYPER)
    hyper = hr.default_hyper(**over)
    with torch.random.fork_rng():
        torch.manual_seed(0)
        net = hr.deform_network(hyper)
        net.deformation_net.grid.set_aabb(*scn["aabb"])
        with torch.no_grad():      # planes off their initial values: time planes at exactly 1 have no |1 - p| derivative to compare
            for p in net.deformation_net.grid.grids.parameters():
                p.add_(0.1 * torch.randn_like(p))
    state = {k: v.detach().clone() for k, v in net.state_dict().items()}
    leaves = {"_xyz": gs["xyz"], "_features_dc": gs["shs"][:, :1], "_features_rest": gs["shs"][:, 1:],
              "_scaling": gs["log_scales"] + 0.9, "_rotation": gs["rotations_raw"], "_opacity": gs["opacity_logit"]}
    leaves = {k: v.float().contiguous().clone() for k, v in leaves.items()}
    g = torch.Generator().manual_seed(9)
    targets = (torch.rand(3, H, W, generator=g), 60 * torch.rand(1, H, W, generator=g), torch.rand(3, H, W, generator=g))
    return dict(name=name, stage="coarse" if name == "coarse" else "fine", scene=scn, camera=scn["cameras"][VIEW], bg=scn["bg"],
                targets=targets, opt=SimpleNamespace(**opt), hyper=hyper, hyper_over=over, leaves=leaves, state=state)


def reference_step(case, dtype=torch.float64, mutate=None):
    """-> dict: loss (float), grads {product parameter name: float64 array, or None where no gradient arrives}, dL_dmeans2D ([P,3],
    the two raster passes summed), radii ([P] int32), num_rendered.  No optimizer step."""
    if mutate is not None and mutate not in MUTANTS:
        raise KeyError(mutate)
    dt = dtype
    npdt = np.float32 if dt == torch.float32 else np.float64
    opt, hy, cam, fine = case["opt"], case["hyper"], case["camera"], case["stage"] == "fine"
    w = dict(dx=opt.lambda_dx, dshs=opt.lambda_dshs, feat=opt.lambda_feat, depth=opt.lambda_depth, dssim=opt.lambda_dssim,
             ts=hy.time_smoothness_weight, l1t=hy.l1_time_planes, tv=hy.plane_tv_weight)
    for m, key in (("no_dx_l1", "dx"), ("no_dshs_l1", "dshs"), ("no_time_smoothness", "ts"), ("no_l1_time_planes", "l1t"),
                   ("no_plane_tv", "tv"), ("no_depth", "depth"), ("no_ssim", "dssim")):
        if mutate == m:
            w[key] = 0.0
    if mutate == "feat_loss_x2":
        w["feat"] *= 2.0
    with torch.random.fork_rng():      # (the constructor draws initial weights; the state dict replaces them)
        net = hr.deform_network(hy)
    net.load_state_dict(case["state"])
    net = net.to(dt)
    L = {k: v.clone().to(dt).requires_grad_(True) for k, v in case["leaves"].items()}
    xyz = L["_xyz"]
    shs0 = torch.cat([L["_features_dc"], L["_features_rest"]], 1)
    if fine:
        time_t = torch.full((P, 1), cam["time"], dtype=dt)
        m3, s, r, o, shs, dx, feat, dshs = net(xyz, L["_scaling"], L["_rotation"], L["_opacity"], shs0, time_t)
    else:
        m3, s, r, o, shs, dx, feat, dshs = xyz, L["_scaling"], L["_rotation"], L["_opacity"], shs0, None, None, None
    scales, rots, opac = torch.exp(s), torch.nn.functional.normalize(r), torch.sigmoid(o)
    cols = hr.shs_to_colors(3, shs, xyz.detach() if mutate == "sh_direction_detached" else xyz, cam["campos"].to(dt))
    n = lambda t_: t_.detach().numpy()
    kw = dict(bg=case["bg"].numpy().astype(npdt), viewmatrix=cam["viewmatrix"].numpy().astype(npdt),
              projmatrix=cam["projmatrix"].numpy().astype(npdt), campos=cam["campos"].numpy().astype(npdt), tanfovx=cam["tanfovx"],
              tanfovy=cam["tanfovy"], image_height=H, image_width=W, scale_modifier=case.get("scale_modifier", 1.0))
    orc = RasterOracle(npdt)
    fwd = [orc.forward(means3D=n(m3), opacities=n(opac), scales=n(scales), rotations=n(rots), colors_precomp=n(c), sh_degree=0, **kw)
           for c in ((cols, feat) if fine else (cols,))]
    gt, gtd, gtf = (t_.to(dt) for t_ in case["targets"])
    img = torch.from_numpy(fwd[0]["color"]).requires_grad_(True)
    dep = torch.from_numpy(fwd[0]["depth"]).requires_grad_(True)
    loss = hr.l1_loss(img[None], gt[None]) + w["dssim"] * (1 - hr.ssim(img[None], gt[None])) + w["depth"] * hr.depth_l2(dep, gtd)
    if fine:
        fimg = torch.from_numpy(fwd[1]["color"]).requires_grad_(True)
        loss = loss + w["feat"] * hr.l2_loss(fimg, gtf)
    loss.backward()
    t = torch.from_numpy
    zero_depth = np.zeros((1, H, W), npdt)
    g = [orc.backward(fwd[0], img.grad.numpy(), dep.grad.numpy() if dep.grad is not None else zero_depth)]
    regs = torch.zeros((), dtype=dt)
    if fine:
        g.append(orc.backward(fwd[1], fimg.grad.numpy(), zero_depth))
        if mutate == "feat_pass_no_means3D":
            g[1]["dL_dmeans3D"] = np.zeros_like(g[1]["dL_dmeans3D"])
        if mutate == "feat_pass_no_opacity":
            g[1]["dL_dopacity"] = np.zeros_like(g[1]["dL_dopacity"])
        dshs_l1 = dshs.abs().sum() / (16 * P) if mutate == "dshs_mean_over_16P" else dshs.abs().mean()
        regs = (w["dx"] * dx.abs().mean() + w["dshs"] * dshs_l1
                + hr.plane_regulation(net.deformation_net.grid.grids, w["ts"], w["l1t"], w["tv"]))
    tot = lambda key: t(sum(gi[key] for gi in g))
    surrogate = ((m3 * tot("dL_dmeans3D")).sum() + (scales * tot("dL_dscales")).sum() + (rots * tot("dL_drotations")).sum()
                 + (opac * tot("dL_dopacity")).sum() + (cols * t(g[0]["dL_dcolors"])).sum() + regs)
    if fine:
        surrogate = surrogate + (feat * t(g[1]["dL_dcolors"])).sum()
    surrogate.backward()
    grads = {k: v.grad.double().numpy() for k, v in L.items()}
    for name, p in net.named_parameters():
        if p.requires_grad:
            grads["_deformation." + name] = None if p.grad is None else p.grad.double().numpy()
    return dict(loss=float(loss.detach() + regs.detach()), grads=grads, dL_dmeans2D=sum(gi["dL_dmeans2D"] for gi in g).astype(np.float64),
                radii=fwd[0]["radii"].copy(), num_rendered=int(fwd[0]["num_rendered"]))


def distances(a, b):
    """{tensor name: rel_l2(a, b)} over every gradient of two reference_step results that b holds, "viewspace" among them."""
    d = {k: rel_l2(a["grads"][k], v) for k, v in b["grads"].items() if v is not None}
    d["viewspace"] = rel_l2(a["dL_dmeans2D"], b["dL_dmeans2D"])
    return d


def densify_stats(dL_dmeans2D, radii):
    """train.py:489-493 from zeroed accumulators for one view: (xyz_gradient_accum [P,1], denom [P,1], max_radii2D [P])."""
    vis = radii > 0
    accum = np.where(vis, np.linalg.norm(np.asarray(dL_dmeans2D, np.float64)[:, :2], axis=1), 0.0)[:, None]
    return accum, vis.astype(np.float64)[:, None], np.where(vis, radii, 0).astype(np.float64)


def record(row):
    """Appends one JSON line of measured numbers to the file S3G_STEP_RECORD names (committed copy of a run:
    profiles/step_gradient_parity.jsonl); writes nothing when it is unset."""
    if RECORD:
        os.makedirs(os.path.dirname(os.path.abspath(RECORD)), exist_ok=True)
        with open(RECORD, "a") as f:
            f.write(json.dumps(row) + "\n")
