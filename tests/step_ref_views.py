"""One training step over a BATCH of views by the reference's algorithm on the CPU (train.py:365-437, 489-493), in float64 or
float32: the checker of `pipeline.training_step_views` (tests/test_step_views_gpu.py); tests/test_step_views_cpu.py checks the
checker.  A helper, not a test.  Built from tests/step_ref.py's pieces -- same scene, oracle.hexplane_ref, RasterOracle, the same
weights and parameter names -- and like it evaluated once, with no optimizer step.

The batch semantics restated here are the reference's, quirks included: L1 and SSIM over the concatenated [V,3,H,W] images; the
depth term over the valid pixels of the whole batch; lambda_dx * mean|dx|, lambda_dshs * mean|dshs| and lambda_feat * l2(feat,
gt_feat) from the LAST view's package only (`render_pkg` is read after the loop); the plane regulariser once; the densification
statistics from the SUMMED viewspace gradient, any-visibility and the largest radius.  feat_views="all" is the product's extension:
every view's feature image is supervised, mean over V*3*H*W.

Cases:
  rig      the three cameras of frame 1 (one timestamp), fine stage, step_ref's `loud` weights
  mixed    two views of different timestamps (the front camera of frame 1, a side camera of frame 2), `loud`: "the last view" is not "any view"
  coarse   the three cameras of frame 1, stage "coarse"
Every view has its own targets; their depth maps have different numbers of valid pixels, so the joint count matters."""
import numpy as np
import torch

from oracle import hexplane_ref as hr
from oracle.oracle import RasterOracle
from tests import step_ref as sr

CASES = {"rig": ("loud", (3, 4, 5)), "mixed": ("loud", (3, 7)), "coarse": ("coarse", (3, 4, 5))}
# wrong reading of a batch seam -> does it change the reported loss?
MUTANTS = {
    "depth_per_view": True,           # mean of per-view depth means instead of one joint count
    "last_view_terms_from_first": True,   # dx / dshs / feat terms from the first view's package
    "feat_on_all_views": True,        # every view's feature image supervised although feat_views="last"
    "sum_of_view_norms": False,       # xyz_gradient_accum += sum_v ||grad_v|| instead of ||sum_v grad_v||
    "plane_reg_per_view": True,       # the plane regulariser applied V times
}


def build_case(name, views=None, base=None):
    """step_ref.build_case(base) plus `cameras` (CPU dicts), `views` (their indices in the scene) and one `targets` triple per
    view.  A single view with step_ref's own camera gets step_ref's own targets: that batch must reproduce step_ref.reference_step."""
    if views is None:
        base, views = CASES[name]
    case = sr.build_case(base)
    case["name"], case["base"], case["views"] = name, base, tuple(views)
    case["cameras"] = [case["scene"]["cameras"][i] for i in views]
    if tuple(views) == (sr.VIEW,):
        case["targets_views"] = [case["targets"]]
    else:
        tv = []
        for k, i in enumerate(views):
            g = torch.Generator().manual_seed(900 + i)
            gtd = 60 * torch.rand(1, sr.H, sr.W, generator=g)
            gtd[:, ::k + 2] = 0.0       # every (k + 2)-th row has no ground-truth depth: 1/2, 1/3, 1/4 of the view's pixels
            tv.append((torch.rand(3, sr.H, sr.W, generator=g), gtd, torch.rand(3, sr.H, sr.W, generator=g)))
        case["targets_views"] = tv
    return case


def reference_step_views(case, dtype=torch.float64, mutate=None, feat_views="last"):
    """-> dict: loss, grads {product parameter name: float64 array or None}, dL_dmeans2D ([P,3], summed over views and raster
    passes), dL_dmeans2D_views, radii (list of [P] int32), num_rendered (list), stats = (xyz_gradient_accum [P,1], denom [P,1],
    max_radii2D [P]) from zeroed accumulators."""
    if mutate is not None and mutate not in MUTANTS:
        raise KeyError(mutate)
    dt = dtype
    npdt = np.float32 if dt == torch.float32 else np.float64
    P, H, W = sr.P, sr.H, sr.W
    opt, hy, cams, fine = case["opt"], case["hyper"], case["cameras"], case["stage"] == "fine"
    V = len(cams)
    pick = 0 if mutate == "last_view_terms_from_first" else V - 1      # the view whose package gives the dx / dshs / feat terms
    every = feat_views == "all" or mutate == "feat_on_all_views"
    sup = [fine and (every or v == pick) for v in range(V)]            # views whose feature image is rasterized and supervised
    with torch.random.fork_rng():      # (the constructor draws initial weights; the state dict replaces them)
        net = hr.deform_network(hy)
    net.load_state_dict(case["state"])
    net = net.to(dt)
    L = {k: v.clone().to(dt).requires_grad_(True) for k, v in case["leaves"].items()}
    xyz = L["_xyz"]
    shs0 = torch.cat([L["_features_dc"], L["_features_rest"]], 1)
    field = {}                         # the field depends on (xyz, t) only: one evaluation per timestamp serves its views
    for cam in cams:
        if fine and cam["time"] not in field:
            field[cam["time"]] = net(xyz, L["_scaling"], L["_rotation"], L["_opacity"], shs0, torch.full((P, 1), cam["time"], dtype=dt))
    n = lambda t_: t_.detach().numpy()
    orc = RasterOracle(npdt)
    views = []
    for v, cam in enumerate(cams):
        if fine:
            m3, s, r, o, shs, dx, feat, dshs = field[cam["time"]]
        else:
            m3, s, r, o, shs, dx, feat, dshs = xyz, L["_scaling"], L["_rotation"], L["_opacity"], shs0, None, None, None
        scales, rots, opac = torch.exp(s), torch.nn.functional.normalize(r), torch.sigmoid(o)
        cols = hr.shs_to_colors(3, shs, xyz, cam["campos"].to(dt))
        kw = _camera_kw(case, cam, npdt)
        fwd = [orc.forward(means3D=n(m3), opacities=n(opac), scales=n(scales), rotations=n(rots), colors_precomp=n(c), sh_degree=0, **kw)
               for c in ((cols, feat) if sup[v] else (cols,))]
        img = torch.from_numpy(fwd[0]["color"]).requires_grad_(True)
        dep = torch.from_numpy(fwd[0]["depth"]).requires_grad_(True)
        fimg = torch.from_numpy(fwd[1]["color"]).requires_grad_(True) if sup[v] else None
        views.append(dict(m3=m3, scales=scales, rots=rots, opac=opac, cols=cols, feat=feat, dx=dx, dshs=dshs, fwd=fwd, img=img, dep=dep,
                          fimg=fimg))
    gts = [tuple(t_.to(dt) for t_ in tv) for tv in case["targets_views"]]
    imgs, gt = torch.stack([vw["img"] for vw in views]), torch.stack([g[0] for g in gts])
    deps, gtd = torch.stack([vw["dep"] for vw in views]), torch.stack([g[1] for g in gts])
    loss = hr.l1_loss(imgs, gt) + opt.lambda_dssim * (1 - hr.ssim(imgs, gt))
    if mutate == "depth_per_view":
        loss = loss + opt.lambda_depth * sum(hr.depth_l2(deps[v], gtd[v]) for v in range(V)) / V
    else:
        loss = loss + opt.lambda_depth * hr.depth_l2(deps, gtd)
    if any(sup):
        if every:
            loss = loss + opt.lambda_feat * hr.l2_loss(torch.stack([vw["fimg"] for vw in views]), torch.stack([g[2] for g in gts]))
        else:
            loss = loss + opt.lambda_feat * hr.l2_loss(views[pick]["fimg"], gts[pick][2])
    loss.backward()
    t = torch.from_numpy
    zero_depth = np.zeros((1, H, W), npdt)
    regs = torch.zeros((), dtype=dt)
    surrogate = torch.zeros((), dtype=dt)
    g2d_views = []
    for vw in views:
        g = [orc.backward(vw["fwd"][0], vw["img"].grad.numpy(), vw["dep"].grad.numpy() if vw["dep"].grad is not None else zero_depth)]
        if vw["fimg"] is not None:
            g.append(orc.backward(vw["fwd"][1], vw["fimg"].grad.numpy(), zero_depth))
        tot = lambda key: t(sum(gi[key] for gi in g))
        surrogate = (surrogate + (vw["m3"] * tot("dL_dmeans3D")).sum() + (vw["scales"] * tot("dL_dscales")).sum()
                     + (vw["rots"] * tot("dL_drotations")).sum() + (vw["opac"] * tot("dL_dopacity")).sum()
                     + (vw["cols"] * t(g[0]["dL_dcolors"])).sum())
        if vw["fimg"] is not None:
            surrogate = surrogate + (vw["feat"] * t(g[1]["dL_dcolors"])).sum()
        g2d_views.append(sum(gi["dL_dmeans2D"] for gi in g).astype(np.float64))
    if fine:
        times = V if mutate == "plane_reg_per_view" else 1
        regs = (opt.lambda_dx * views[pick]["dx"].abs().mean() + opt.lambda_dshs * views[pick]["dshs"].abs().mean()
                + times * hr.plane_regulation(net.deformation_net.grid.grids, hy.time_smoothness_weight, hy.l1_time_planes,
                                              hy.plane_tv_weight))
    (surrogate + regs).backward()
    grads = {k: v.grad.double().numpy() for k, v in L.items()}
    for name, p in net.named_parameters():
        if p.requires_grad:
            grads["_deformation." + name] = None if p.grad is None else p.grad.double().numpy()
    radii = [vw["fwd"][0]["radii"].copy() for vw in views]
    total = np.zeros_like(g2d_views[0])
    for g2d in g2d_views:              # train.py:435-437: zeros + grad_0 + grad_1 + ...
        total = total + g2d
    return dict(loss=float(loss.detach() + regs.detach()), grads=grads, dL_dmeans2D=total, dL_dmeans2D_views=g2d_views, radii=radii,
                num_rendered=[int(vw["fwd"][0]["num_rendered"]) for vw in views],
                stats=densify_stats_views(g2d_views, radii, sum_of_norms=mutate == "sum_of_view_norms"))


def _camera_kw(case, cam, npdt):
    return dict(bg=case["bg"].numpy().astype(npdt), viewmatrix=cam["viewmatrix"].numpy().astype(npdt),
                projmatrix=cam["projmatrix"].numpy().astype(npdt), campos=cam["campos"].numpy().astype(npdt), tanfovx=cam["tanfovx"],
                tanfovy=cam["tanfovy"], image_height=sr.H, image_width=sr.W, scale_modifier=1.0)


def densify_stats_views(g2d_views, radii, sum_of_norms=False):
    """train.py:387-388, 435-437, 489-493 from zeroed accumulators: (xyz_gradient_accum [P,1], denom [P,1], max_radii2D [P])."""
    vis = np.any([r > 0 for r in radii], axis=0)
    r = np.max(radii, axis=0)
    if sum_of_norms:
        norm = sum(np.where(rv > 0, np.linalg.norm(g[:, :2], axis=1), 0.0) for g, rv in zip(g2d_views, radii))
    else:
        norm = np.linalg.norm(sum(g[:, :2] for g in g2d_views), axis=1)
    return np.where(vis, norm, 0.0)[:, None], vis.astype(np.float64)[:, None], np.where(vis, r, 0).astype(np.float64)


def distances(a, b):
    """step_ref.distances plus the batch's xyz_gradient_accum."""
    d = sr.distances(a, b)
    d["xyz_gradient_accum"] = sr.rel_l2(a["stats"][0], b["stats"][0])
    return d
