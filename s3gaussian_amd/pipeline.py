"""Host-side mirror of the reference's hot path around the accelerated operators (GPU only):

  GaussianParams      <- the tensors/optimizer groups of scene/gaussian_model.py:30-201 that the path touches
  render()            <- gaussian_renderer/__init__.py:23-210 (same arguments, same result-dict keys)
  training_loss()     <- train.py:395-425 loss assembly (L1 + dx/dshs reg + depth L2 + plane regulation + DSSIM + feat L2)
  training_step()     <- train.py:372-437,521-522 for one view (batch_size = 1)
  render_views(), training_loss_views(), training_step_views()
                      <- the same for a batch of views (opt.batch_size, train.py:286, 327-437): one deformation pass and one glue
                         pass per TIMESTAMP of the batch, one loss node, one backward, one Adam step; rig_batches() groups a rig's
                         cameras by timestamp
  evaluate()          <- the metric part of utils/video_utils.py:169-241 (PSNR, SSIM and their masked forms per frame, metrics.py)
  render_flows()      <- the flow part of utils/video_utils.py:203-209, 252-299 (forward / backward scene-flow images, flow.py)
  evaluate_video()    <- utils/video_utils.py:116-349 + 439-499 in one pass: metrics, decomposition, flows and the uint8 strips the
                         reference hands to its video writer, from ONE render per camera (frames.py)
  scene_from_lidar()  <- the LiDAR part of readWaymoInfo (scene/dataset_readers.py:752-779, 824-977): per-camera depth maps at any
                         image size, the camera-frustum aabb and the voxel-sampled initial cloud (lidar.py)

Adaptive density control -- GaussianParams.densify / prune / reset_opacity and the schedule of train.py:494-516 -- lives in
density.py on kernels of its own (include/s3g_density.h).  Everything else outside that path (data readers, checkpoints'
surroundings, LPIPS and the video encoder of the evaluation -- its frames are built here --, logging) stays with the reference and
is NOT rebuilt here (DESIGN.md "out of scope").  The losses are plain PyTorch on the GPU exactly like the
reference's utils/loss_utils.py; the operators underneath are the HIP library.
"""
from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Dict, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import lpips as _lpips
from . import lpips_vgg as _lpips_vgg
from . import metrics as _metrics
from . import sky as _sky
from .deformation import deform_network
from .glue import activations_and_colors
from .knn import distCUDA2
from .losses import photometric_loss as fused_photometric_loss
from .losses import plane_regulation as fused_plane_regulation
from .losses import ssim as fused_ssim
from .rasterizer import GaussianRasterizationSettings, GaussianRasterizer


def default_hyper(**over) -> SimpleNamespace:
    """ModelHiddenParams defaults (arguments/__init__.py:204-233)."""
    h = dict(net_width=64, timebase_pe=4, defor_depth=1, posebase_pe=10, scale_rotation_pe=2, opacity_pe=2,
             timenet_width=64, timenet_output=32, bounds=1.6, plane_tv_weight=0.0001, time_smoothness_weight=0.01,
             l1_time_planes=0.0001,
             kplanes_config=dict(grid_dimensions=2, input_coordinate_dim=4, output_coordinate_dim=32,
                                 resolution=[64, 64, 64, 25]),
             multires=[1, 2, 4, 8], no_dx=False, no_grid=False, no_ds=True, no_dr=True, no_do=True, no_dshs=False,
             feat_head=True, empty_voxel=False, grid_pe=0, static_mlp=False, apply_rotation=False)
    h.update(over)
    return SimpleNamespace(**h)


def default_opt(**over) -> SimpleNamespace:
    """The OptimizationParams the path reads (arguments/__init__.py:100-158).  One extension rides in through `over`:
    default_opt(lambda_sky=w), the weight of sky.sky_opacity_loss in training_step / training_step_views.  The reference has no such
    field (its sky masks feed nothing), so the defaults carry none either: an absent lambda_sky is 0, the term is off."""
    o = dict(position_lr_init=0.00016, deformation_lr_init=0.000016, grid_lr_init=0.00016, feature_lr=0.0025,
             opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001, lambda_dssim=0.2, lambda_depth=0.5,
             lambda_feat=0.001, lambda_dx=0.001, lambda_dshs=0.001)
    o.update(over)
    return SimpleNamespace(**o)


def inverse_sigmoid(x):
    return torch.log(x / (1 - x))


class GaussianParams(nn.Module):
    """Parameter store with the reference's attribute names (`_xyz`, `_features_dc`, ..., `_deformation`)."""

    percent_dense = 0.01     # scene/gaussian_model.py:171 takes it from the optimization arguments; training_setup does too

    def __init__(self, sh_degree: int, hyper: SimpleNamespace):
        super().__init__()
        self.max_sh_degree = sh_degree
        self.active_sh_degree = sh_degree
        self._deformation = deform_network(hyper)
        self.spatial_lr_scale = 1.0
        self.scaling_activation = torch.exp
        self.opacity_activation = torch.sigmoid
        self.rotation_activation = F.normalize

    @torch.no_grad()
    def init_from_tensors(self, xyz, log_scales, rotations, opacity_logit, shs, device):
        self._xyz = nn.Parameter(xyz.float().to(device).contiguous())
        shs = shs.float().to(device)
        self._features_dc = nn.Parameter(shs[:, :1].contiguous())
        self._features_rest = nn.Parameter(shs[:, 1:].contiguous())
        self._scaling = nn.Parameter(log_scales.float().to(device).contiguous())
        self._rotation = nn.Parameter(rotations.float().to(device).contiguous())
        self._opacity = nn.Parameter(opacity_logit.float().to(device).contiguous())
        self._deformation = self._deformation.to(device)
        self._deformation_table = torch.ones(xyz.shape[0], dtype=torch.bool, device=device)
        self.max_radii2D = torch.zeros(xyz.shape[0], device=device)
        return self

    @torch.no_grad()
    def create_from_points(self, points: torch.Tensor, colors: torch.Tensor, device):
        """scene/gaussian_model.py:142-169: scales from the 3-NN distance (distCUDA2), identity rotations, opacity 0.1."""
        pts = points.float().to(device)
        dist2 = torch.clamp_min(distCUDA2(pts), 0.0000001)
        log_scales = torch.log(torch.sqrt(dist2))[..., None].repeat(1, 3)
        rots = torch.zeros((pts.shape[0], 4), device=device)
        rots[:, 0] = 1
        op = inverse_sigmoid(0.1 * torch.ones((pts.shape[0], 1), device=device))
        shs = torch.zeros((pts.shape[0], (self.max_sh_degree + 1) ** 2, 3), device=device)
        shs[:, 0] = (colors.float().to(device) - 0.5) / 0.28209479177387814
        return self.init_from_tensors(pts, log_scales, rots, op, shs, device)

    @property
    def get_xyz(self):
        return self._xyz

    @property
    def get_features(self):
        return torch.cat((self._features_dc, self._features_rest), dim=1)

    def training_setup(self, opt: SimpleNamespace):
        """Adam groups of scene/gaussian_model.py:177-189 (eps 1e-15)."""
        s = self.spatial_lr_scale
        self.percent_dense = getattr(opt, "percent_dense", self.percent_dense)
        groups = [
            {"params": [self._xyz], "lr": opt.position_lr_init * s, "name": "xyz"},
            {"params": list(self._deformation.get_mlp_parameters()), "lr": opt.deformation_lr_init * s, "name": "deformation"},
            {"params": list(self._deformation.get_grid_parameters()), "lr": opt.grid_lr_init * s, "name": "grid"},
            {"params": [self._features_dc], "lr": opt.feature_lr, "name": "f_dc"},
            {"params": [self._features_rest], "lr": opt.feature_lr / 20.0, "name": "f_rest"},
            {"params": [self._opacity], "lr": opt.opacity_lr, "name": "opacity"},
            {"params": [self._scaling], "lr": opt.scaling_lr, "name": "scaling"},
            {"params": [self._rotation], "lr": opt.rotation_lr, "name": "rotation"},
        ]
        # same update rule and state layout as the reference's torch.optim.Adam(l, lr=0.0, eps=1e-15); on the GPU the whole
        # step is one kernel launch over all groups (optim.Adam) instead of ~10 foreach passes per group
        P = self._xyz.shape[0]   # densification accumulators, scene/gaussian_model.py:172-174
        self.xyz_gradient_accum = torch.zeros((P, 1), device=self._xyz.device)
        self.denom = torch.zeros((P, 1), device=self._xyz.device)
        if self._xyz.is_cuda:
            from .optim import Adam as FusedAdam
            self.optimizer = FusedAdam(groups, lr=0.0, eps=1e-15)
        else:
            self.optimizer = torch.optim.Adam(groups, lr=0.0, eps=1e-15)
        return self.optimizer

    def attach_sky_model(self, model, lr: float = 0.0025):
        """Adds the sky colour model's six parameters to `self.optimizer` as ONE param group named "sky_model" (lr: the reference's
        bg_model_lr), after training_setup.  The group then shares the optimizer's overflow guard, its rewind under
        run_training_steps and the data-parallel reducers; density control skips it (a multi-parameter group).  The model is moved to
        the Gaussians' device; it does not become a submodule (checkpoints of the Gaussians keep their keys)."""
        from . import skymodel as _skymodel
        opt = getattr(self, "optimizer", None)
        if opt is None:
            raise RuntimeError("attach_sky_model: call training_setup first (there is no optimizer to add the group to)")
        if any(g.get("name") == "sky_model" for g in opt.param_groups):
            raise RuntimeError('attach_sky_model: the optimizer already has a "sky_model" group')
        if not isinstance(model, _skymodel.SkyModel):
            raise TypeError("attach_sky_model: an s3gaussian_amd.skymodel.SkyModel")
        model.to(self._xyz.device)
        opt.add_param_group({"params": model.tensors(), "lr": float(lr), "name": "sky_model"})
        return model

    # ---- adaptive density control (density.py; the reference's argument order, its unused trailing arguments accepted and ignored) ----
    def densify(self, max_grad, min_opacity, extent, max_screen_size, density_threshold=None, displacement_scale=None,
                model_path=None, iteration=None, stage=None, **kw):
        """scene/gaussian_model.py:673-678.  kw: noise / seed / return_noise / percent_dense of density.densify."""
        from . import density
        return density.densify(self, max_grad, extent, **kw)

    def prune(self, max_grad, min_opacity, extent, max_screen_size):
        """scene/gaussian_model.py:661-670."""
        from . import density
        return density.prune(self, min_opacity, extent, max_screen_size)

    def reset_opacity(self):
        """scene/gaussian_model.py:350-353."""
        from . import density
        return density.reset_opacity(self)

    # ---- optional maintenance: keep the Gaussians in a spatially coherent order ------------------------------------------
    @torch.no_grad()
    def reorder_spatially(self, cells: int = 1024):
        """Permute the Gaussians into the Morton (3-D blocked) order of their positions: every per-Gaussian parameter, its Adam
        moments, the densification accumulators and the deformation table move together, the Parameter objects stay the same
        (optimizer groups and data-parallel reducers keep working).  The index of a Gaussian has no meaning in the reference
        (densify / prune reshuffle them, scene/gaussian_model.py:397-494), so this changes no result beyond the tie-break of
        exactly equal depths; what it buys is locality: neighbouring lanes then read neighbouring texels, tiles and rows
        WITHOUT a processing-order indirection.  Not called by training_step / bench.py.
        Returns the permutation: new[i] = old[perm[i]]."""
        xyz = self._xyz.detach()
        lo, hi = xyz.min(dim=0).values, xyz.max(dim=0).values
        q = ((xyz - lo) / (hi - lo).clamp_min(1e-12) * (cells - 1)).long().clamp_(0, cells - 1)

        def spread(v):   # 10 bits -> every third bit
            v = (v | (v << 16)) & 0x030000FF
            v = (v | (v << 8)) & 0x0300F00F
            v = (v | (v << 4)) & 0x030C30C3
            return (v | (v << 2)) & 0x09249249

        key = spread(q[:, 0]) | (spread(q[:, 1]) << 1) | (spread(q[:, 2]) << 2)
        perm = torch.argsort(key, stable=True)
        params = [self._xyz, self._features_dc, self._features_rest, self._scaling, self._rotation, self._opacity]
        opt = getattr(self, "optimizer", None)
        for p in params:
            p.data = p.data[perm].contiguous()
            if p.grad is not None:      # a pending gradient (called between backward and step) follows its Gaussian
                p.grad = p.grad[perm].contiguous()
            torch.autograd.graph.increment_version(p)
            st = opt.state.get(p) if opt is not None else None
            if st:
                for name in ("exp_avg", "exp_avg_sq"):
                    if name in st:
                        st[name] = st[name][perm].contiguous()
        for name in ("max_radii2D", "xyz_gradient_accum", "denom", "_deformation_table"):
            t_ = getattr(self, name, None)
            if isinstance(t_, torch.Tensor) and t_.shape[:1] == perm.shape:
                setattr(self, name, t_[perm].contiguous())
        # cached spatial orders of the sampler hold point indices of the old order; the rasterizer's geometry cache likewise
        grid = getattr(self._deformation.deformation_net, "grid", None)
        if grid is not None and hasattr(grid, "_order_cache"):
            grid._order_cache.clear()
        if self._xyz.is_cuda:
            from . import raster_C
            raster_C.invalidate_geometry_cache()
        return perm

    # ---- checkpoint / point-cloud I/O with the reference's formats -------------------------------------
    def capture(self):
        """The 14-tuple of scene/gaussian_model.py:71-88 (what train.py saves with torch.save)."""
        return (self.active_sh_degree, self._xyz, self._deformation.state_dict(), self._deformation_table,
                self._features_dc, self._features_rest, self._scaling, self._rotation, self._opacity, self.max_radii2D,
                self.xyz_gradient_accum, self.denom, self.optimizer.state_dict(), self.spatial_lr_scale)

    def restore(self, model_args, training_args):
        """scene/gaussian_model.py:90-111: accepts a tuple captured here or by the reference's GaussianModel."""
        (self.active_sh_degree, xyz, deform_state, self._deformation_table, f_dc, f_rest, scaling, rotation, opacity,
         self.max_radii2D, xyz_gradient_accum, denom, opt_dict, self.spatial_lr_scale) = model_args
        dev = xyz.device
        as_param = lambda t_: nn.Parameter(t_.detach().clone().float().contiguous().to(dev))
        self._xyz, self._features_dc, self._features_rest = as_param(xyz), as_param(f_dc), as_param(f_rest)
        self._scaling, self._rotation, self._opacity = as_param(scaling), as_param(rotation), as_param(opacity)
        self._deformation.load_state_dict(deform_state)
        self._deformation = self._deformation.to(dev)
        self.training_setup(training_args)
        self.xyz_gradient_accum, self.denom = xyz_gradient_accum, denom
        self.optimizer.load_state_dict(opt_dict)
        for st in self.optimizer.state.values():   # torch.load(map_location="cuda") puts the step counters on the GPU, where
            if torch.is_tensor(st.get("step")):    # reading them would cost one host sync per parameter and step
                st["step"] = st["step"].cpu()

    def construct_list_of_attributes(self):
        """scene/gaussian_model.py:220-234."""
        l = ['x', 'y', 'z', 'nx', 'ny', 'nz']
        l += [f'f_dc_{i}' for i in range(self._features_dc.shape[1] * self._features_dc.shape[2])]
        l += [f'f_rest_{i}' for i in range(self._features_rest.shape[1] * self._features_rest.shape[2])]
        l += ['opacity'] + [f'scale_{i}' for i in range(self._scaling.shape[1])] + [f'rot_{i}' for i in range(self._rotation.shape[1])]
        return l

    @torch.no_grad()
    def save_ply(self, path):
        """scene/gaussian_model.py:258-275: same attribute order and layout (SH coefficients channel-major).  On the GPU the table is
        built by one launch (split.pack_ply_rows) and crosses to the host in one copy; the file is the same, byte for byte."""
        import numpy as np
        from .plyio import write_vertices
        if self._xyz.is_cuda:
            from . import split
            write_vertices(path, self.construct_list_of_attributes(), split.model_rows(self).cpu().numpy())
            return
        n = lambda t_: t_.detach().cpu().numpy()
        xyz = n(self._xyz)
        cols = [xyz, np.zeros_like(xyz), n(self._features_dc.transpose(1, 2).flatten(start_dim=1).contiguous()),
                n(self._features_rest.transpose(1, 2).flatten(start_dim=1).contiguous()), n(self._opacity), n(self._scaling),
                n(self._rotation)]
        write_vertices(path, self.construct_list_of_attributes(), np.concatenate(cols, axis=1))

    @torch.no_grad()
    def save_ply_split(self, dynamic_pcd_path, static_pcd_path, dx_list, visibility_filter=None, index=24):
        """scene/gaussian_model.py:277-348: the Gaussians whose displacement dx = dx_list[index] exceeds the mean, max|dx_i| >
        mean_j max|dx_j|, go to `dynamic_pcd_path`, the others to `static_pcd_path`, both at their deformed positions xyz + dx and in
        source order.  The reference hard-codes entry 24 (a shorter list raises the same IndexError) and never looks at
        `visibility_filter`; neither does this.
        One deliberate difference: the reference rebinds `self._xyz = self._xyz + dx` on the way, which leaves a non-Parameter tensor
        behind the optimizer's back; here the model is left untouched.  The files are the same.
        -> {"n_dynamic", "n_static", "thre"} (the reference returns None)."""
        from . import split
        return split.export_split(self, dx_list[index], dynamic_pcd_path, static_pcd_path)

    @torch.no_grad()
    def load_ply(self, path, device=None):
        """scene/gaussian_model.py:355-395."""
        import numpy as np
        from .plyio import read_vertices
        device = device if device is not None else (self._xyz.device if hasattr(self, "_xyz") else "cuda")
        names, v = read_vertices(path)
        col = lambda prefix: sorted((k for k in names if k.startswith(prefix)), key=lambda x: int(x.split('_')[-1]))
        xyz = np.stack((v["x"], v["y"], v["z"]), axis=1)
        f_dc = np.stack([v[f"f_dc_{k}"] for k in range(3)], axis=1)[:, :, None]
        extra = col("f_rest_")
        assert len(extra) == 3 * (self.max_sh_degree + 1) ** 2 - 3
        f_rest = np.stack([v[k] for k in extra], axis=1).reshape(xyz.shape[0], 3, (self.max_sh_degree + 1) ** 2 - 1)
        scales = np.stack([v[k] for k in col("scale_")], axis=1)
        rots = np.stack([v[k] for k in col("rot")], axis=1)
        tt = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float, device=device)
        self._xyz = nn.Parameter(tt(xyz))
        self._features_dc = nn.Parameter(tt(f_dc).transpose(1, 2).contiguous())
        self._features_rest = nn.Parameter(tt(f_rest).transpose(1, 2).contiguous())
        self._opacity = nn.Parameter(tt(v["opacity"][:, None]))
        self._scaling = nn.Parameter(tt(scales))
        self._rotation = nn.Parameter(tt(rots))
        self.active_sh_degree = self.max_sh_degree
        self._deformation_table = torch.ones(xyz.shape[0], dtype=torch.bool, device=device)
        self.max_radii2D = torch.zeros(xyz.shape[0], device=device)

    def compute_regulation(self, time_smoothness_weight, l1_time_planes_weight, plane_tv_weight):
        """scene/gaussian_model.py:710-749."""
        grids = self._deformation.deformation_net.grid.grids
        if self._xyz.is_cuda:
            return fused_plane_regulation(grids, time_smoothness_weight, l1_time_planes_weight, plane_tv_weight)
        sp = sum(_plane_smoothness(g[i]) for g in grids for i in (0, 1, 3))
        tm = sum(_plane_smoothness(g[i]) for g in grids for i in (2, 4, 5))
        l1 = sum(torch.abs(1 - g[i]).mean() for g in grids for i in (2, 4, 5))
        return plane_tv_weight * sp + time_smoothness_weight * tm + l1_time_planes_weight * l1


# ---- SH evaluation (utils/sh_utils.py:57-112), used on the default convert_SHs_python=True path ----------------
_C0 = 0.28209479177387814
_C1 = 0.4886025119029199
_C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
_C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
       1.445305721320277, -0.5900435899266435]


def eval_sh(deg, sh, dirs):
    result = _C0 * sh[..., 0]
    if deg > 0:
        x, y, z = dirs[..., 0:1], dirs[..., 1:2], dirs[..., 2:3]
        result = result - _C1 * y * sh[..., 1] + _C1 * z * sh[..., 2] - _C1 * x * sh[..., 3]
        if deg > 1:
            xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
            result = (result + _C2[0] * xy * sh[..., 4] + _C2[1] * yz * sh[..., 5] + _C2[2] * (2.0 * zz - xx - yy) * sh[..., 6]
                      + _C2[3] * xz * sh[..., 7] + _C2[4] * (xx - yy) * sh[..., 8])
            if deg > 2:
                result = (result + _C3[0] * y * (3 * xx - yy) * sh[..., 9] + _C3[1] * xy * z * sh[..., 10]
                          + _C3[2] * y * (4 * zz - xx - yy) * sh[..., 11] + _C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * sh[..., 12]
                          + _C3[4] * x * (4 * zz - xx - yy) * sh[..., 13] + _C3[5] * z * (xx - yy) * sh[..., 14]
                          + _C3[6] * x * (xx - 3 * yy) * sh[..., 15])
    return result


def covariance_from_scaling_rotation(scaling, scaling_modifier, rotation):
    """GaussianModel.get_covariance (scene/gaussian_model.py:33-37,135-136; utils/general_utils.py:231-277): Sigma = L L^T with
    L = R(q / |q|) diag(modifier * s), returned as the six upper-triangular entries [P,6] the rasterizer takes as cov3D_precomp."""
    q = rotation / torch.sqrt((rotation * rotation).sum(dim=1, keepdim=True))
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).view(-1, 3, 3)
    Lm = R * (scaling_modifier * scaling)[:, None, :]          # R @ diag(s)
    cov = Lm @ Lm.transpose(1, 2)
    return torch.stack([cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]], dim=1)


_time_cache: Dict = {}


def _uniform_time(t: float, device) -> torch.Tensor:
    """[1,1] device tensor holding the camera timestamp.  With `uniform_time` the sampler reads time[0] only
    (include/s3g_hexplane.h), so the reference's `torch.full((P,1), time)` -- a 4.8 MB fill per render -- shrinks to one cached
    element per distinct timestamp (a clip has tens of them)."""
    key = (t, device)
    v = _time_cache.get(key)
    if v is None:
        if len(_time_cache) > 4096:
            _time_cache.clear()
        v = _time_cache[key] = torch.full((1, 1), t, dtype=torch.float32, device=device)
    return v


class _LazyResult(dict):
    """render()'s result dict with entries that are only computed when somebody reads them.  The reference returns
    `visibility_filter_d = radii_d > 0` for the masked subsets (gaussian_renderer/__init__.py:199-203): variable-size results of
    boolean indexing, i.e. two host synchronisations per evaluation frame for values its callers (utils/video_utils.py:185,193)
    read into a variable and never use.  Same keys, same values, evaluated on first access."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self._lazy = {}

    def set_lazy(self, key, thunk):
        self._lazy[key] = thunk
        super().__setitem__(key, None)

    def _force(self, key):
        thunk = self._lazy.pop(key, None)
        if thunk is not None:
            super().__setitem__(key, thunk())

    def __getitem__(self, key):
        self._force(key)
        return super().__getitem__(key)

    def get(self, key, default=None):
        self._force(key)
        return super().get(key, default)

    def _force_all(self):
        for key in list(self._lazy):
            self._force(key)

    def items(self):
        self._force_all()
        return super().items()

    def values(self):
        self._force_all()
        return super().values()

    def __setitem__(self, key, value):
        self._lazy.pop(key, None)
        super().__setitem__(key, value)

    # dict(out), {**out}, out | other: CPython copies a dict SUBCLASS through the fast path (raw table, placeholders and all)
    # unless the subclass overrides __iter__; with it overridden they go through keys() + __getitem__, which force the entries
    def __iter__(self):
        self._force_all()
        return super().__iter__()

    def keys(self):
        self._force_all()
        return super().keys()

    def copy(self):
        self._force_all()
        return dict(super().items())

    def pop(self, key, *default):
        self._force(key)
        return super().pop(key, *default)

    def setdefault(self, key, default=None):
        self._force(key)
        return super().setdefault(key, default)

    def __or__(self, other):
        return dict(self) | other

    def __ror__(self, other):
        return other | dict(self)


def _default_pipe(pipe: Optional[SimpleNamespace]) -> SimpleNamespace:
    return pipe or SimpleNamespace(convert_SHs_python=True, compute_cov3D_python=False, debug=False)


def _raster_settings(cam: Dict, pc: GaussianParams, pipe: SimpleNamespace, bg: torch.Tensor, scale_modifier=1.0):
    return GaussianRasterizationSettings(
        image_height=int(cam["image_height"]), image_width=int(cam["image_width"]), tanfovx=cam["tanfovx"],
        tanfovy=cam["tanfovy"], bg=bg, scale_modifier=scale_modifier, viewmatrix=cam["viewmatrix"],
        projmatrix=cam["projmatrix"], sh_degree=pc.active_sh_degree, campos=cam["campos"], prefiltered=False,
        debug=getattr(pipe, "debug", False))


def _glue_route(pc: GaussianParams, pipe: SimpleNamespace, stage: str) -> bool:
    """The fused glue (+ in a fine stage the fused deformation) route serves this model: GPU tensors, SH degree 3,
    convert_SHs_python and fused_glue on (pipe.fused_glue=False: torch glue, tests), and in a fine stage a network on
    Deformation._fused_any.  render() further asks for no override_color, render_views() for no compute_cov3D_python."""
    return bool(pc.get_xyz.is_cuda and getattr(pipe, "convert_SHs_python", True) and pc.max_sh_degree == 3
                and getattr(pipe, "fused_glue", True) and ("coarse" in stage or pc._deformation.deformation_net._fused_any()))


def _deform_fused(pc: GaussianParams, t: float, stage: str, need_feat: bool, with_plane_reg: bool):
    """The fused route's deformation of one timestamp -> (means3D_final, scales, rotations, opacity, dx, dshs, feat, plane_reg);
    scales / rotations / opacity are still RAW (the glue kernel activates them) and in a coarse stage everything is the model's own.
    By default only dx / dshs / feat come from the network (scales, rotations, opacity pass through, deformation.py:126-152) and
    `shs + dshs` is folded into the glue kernel.  `time` is one timestamp repeated; with_plane_reg: the plane regulariser
    (compute_regulation) rides on the sampler's node, so its gradient is the seed the sampler's backward accumulates onto."""
    means3D, scales, rotations, opacity = pc.get_xyz, pc._scaling, pc._rotation, pc._opacity
    if "coarse" in stage:
        return means3D, scales, rotations, opacity, None, None, None, None
    net = pc._deformation.deformation_net
    hy = net.args
    regw = (hy.time_smoothness_weight, hy.l1_time_planes, hy.plane_tv_weight) if with_plane_reg else None
    heads = net.deform_heads(means3D, _uniform_time(float(t), means3D.device), uniform_time=True, reg_weights=regw, need_feat=need_feat,
                             with_geometry=True)
    dx, dshs, feat = heads[:3]
    means3D_final = means3D if dx is None else means3D + dx     # dx is None: a static model (no_dx) has no position head
    if heads[3] is not None:
        # scale / rotation / opacity deformation (no_ds / no_dr / no_do off): the raw parameters plus the geometry heads' outputs
        # go into the glue kernel in place of the raw ones (deformation.py:126-152, then the activations of :99-101)
        scales, rotations, opacity = net.apply_geometry(scales, rotations, opacity, *heads[3])
    return means3D_final, scales, rotations, opacity, dx, dshs, feat, heads[4] if with_plane_reg else None


def _rasterize_view(rasterizer, means3D, means2D, opacity, scales, rotations, cov3D_precomp, shs, colors, want_feat, feat_colors,
                    fused_pair, return_alpha, densify_accum=None):
    """One view: the main render, then (want_feat) the feature render -- both from one node with fused_pair (RGB + feature image:
    shared geometry forward, ONE fused backward, rasterizer.forward_pair), else the feature image from a plain node of its own.
    -> (image, radii, depth, image2 | None, alpha | None)"""
    geometry = dict(scales=scales, rotations=rotations, cov3D_precomp=cov3D_precomp)
    if want_feat and fused_pair:
        image, radii, depth, image2, *alpha = rasterizer.forward_pair(
            means3D=means3D, means2D=means2D, opacities=opacity, colors_a=colors, colors_b=feat_colors, densify_accum=densify_accum,
            **geometry, **({"with_alpha": True} if return_alpha else {}))
    else:
        image, radii, depth, *alpha = (rasterizer.forward_alpha if return_alpha else rasterizer)(
            means3D=means3D, means2D=means2D, shs=shs, colors_precomp=colors, opacities=opacity, **geometry)
        image2 = None
        if want_feat:
            image2, _, _ = rasterizer(means3D=means3D, means2D=means2D, shs=None, colors_precomp=feat_colors, opacities=opacity,
                                      **geometry)
    return image, radii, depth, image2, alpha[0] if alpha else None


def _view_result(image, means2D, radii, depth, image2, alpha, want_feat, return_alpha, with_dx, dx, dshs, dshs_l1, plane_reg):
    """The keys render() and render_views() share; which key appears when is the reference's (plus the extensions' "alpha",
    "dshs_l1", "plane_reg")."""
    out = _LazyResult({"render": image, "viewspace_points": means2D, "visibility_filter": radii > 0, "radii": radii, "depth": depth})
    if want_feat:
        out["feat"] = image2
    if return_alpha:
        out["alpha"] = alpha
    if with_dx:
        out.update({"dx": dx, "dshs": dshs})
        if dshs_l1 is not None:
            out["dshs_l1"] = dshs_l1
    if plane_reg is not None:
        out["plane_reg"] = plane_reg
    return out


def _sky_refusals(where: str, sky_model, pose=None, override_color=None) -> None:
    """What a sky model does not go together with, refused by name."""
    if pose is not None:
        raise RuntimeError(f"{where}(sky_model=..., pose=...): the refined pose lives on the device, the sky model's directions take "
                           "host camera values; render the sky model without pose refinement")
    if override_color is not None:
        raise RuntimeError(f"{where}(sky_model=..., override_color=...): an override colour is not a radiance the sky is composited behind")


def _sky_attached(where: str, pc, sky_model) -> None:
    from . import skymodel as _skymodel
    if _skymodel.attached_group(getattr(pc, "optimizer", None), sky_model) is None:
        raise RuntimeError(f'{where}(sky_model=...): the model is not attached: pc.attach_sky_model(model) adds its "sky_model" '
                           "param group to pc.optimizer")


def _sky_compose(out: Dict, sky_model, cam: Dict) -> Dict:
    """out["render"] <- out["render"] + (1 - out["alpha"]) * sky; the render over black stays as out["render_fg"]."""
    from . import skymodel as _skymodel
    out["render_fg"] = out["render"]
    out["render"] = _skymodel.sky_composite(sky_model, cam, out["render_fg"], out["alpha"])
    return out


def render(viewpoint_camera: Dict, pc: GaussianParams, pipe: SimpleNamespace, bg_color: torch.Tensor,
           scaling_modifier=1.0, override_color=None, stage="fine", return_decomposition=False, return_dx=False,
           render_feat=False, densify_accum=None, extra_colors=None, return_alpha=False, pose=None, cam_index=None, sky_model=None):
    """Mirror of gaussian_renderer/__init__.py::render.  `viewpoint_camera` is a dict with the fields the reference
    reads from a Camera (image_height/width, FoVx/FoVy or tanfovx/tanfovy, world_view_transform=viewmatrix,
    full_proj_transform=projmatrix, camera_center=campos, time).
    densify_accum (extension): (xyz_gradient_accum, denom, max_radii2D) updated by the rasterizer's backward itself when the
    RGB + feature pair runs as one node (train.py:489-493 otherwise does it in separate passes); the result dict then carries
    "densify_stats_fused": True.
    extra_colors (extension, no_grad only): a sequence of [P,3] colour tensors.  After the frame's own rasterisation each one is
    blended on the SAME geometry tensors, so the rasterizer's geometry cache serves it without another preprocess / binning / sort
    (s3g_raster_forward_reuse); the images come back as out["extra"], a list of [3,H,W].  What the reference does with one more
    `render(..., override_color=c)` per image (utils/video_utils.py:267,284), on the fused route and the frame's own geometry.
    return_alpha (extension): out["alpha"] = the accumulated opacity [1,H,W] of the main render, 1 - the final transmittance of
    each pixel (rasterizer.forward_alpha); differentiable, zeros for a model without Gaussians.  False launches nothing new.
    pose (extension): a pose.PoseRefiner; the camera is then rendered at its refined pose, pose.corrected(camera, cam_index), and
    under autograd the loss back-propagates to the refiner's correction of that camera.  None launches nothing new.
    sky_model (extension): a skymodel.SkyModel on the Gaussians' device.  Implies return_alpha; the Gaussians are rendered over a
    ZERO background of the call's own and `bg_color` is NOT used.  out["render"] = render_fg + (1 - alpha) * sky is the composite
    (skymodel.sky_composite, differentiable w.r.t. the model, the render and the opacity), out["render_fg"] the Gaussians over
    black, out["alpha"] the opacity image; the decomposition's render_d / render_s and out["extra"] stay over black.  Refused
    together with pose= and with override_color.  The directions take the camera's rotation as host values: with `viewmatrix` on
    the device that is one blocking read-back per call (the host waits for the rasterizer forward); a camera dict that also carries
    "viewmatrix_host", a CPU copy of viewmatrix, avoids it (skymodel.camera_intrinsics).  None launches nothing new."""
    if sky_model is not None:
        _sky_refusals("render", sky_model, pose, override_color)
        bg_color = torch.zeros(3, dtype=torch.float32, device=pc.get_xyz.device)
        return_alpha = True
    if pose is not None:
        if cam_index is None:
            raise RuntimeError("render(pose=...): cam_index says which of the refiner's cameras this is")
        viewpoint_camera = pose.corrected(viewpoint_camera, cam_index)
    if extra_colors is not None and torch.is_grad_enabled():
        raise RuntimeError("render(extra_colors=...) is an inference extension: call it under torch.no_grad()")
    dev = pc.get_xyz.device
    # the reference builds `zeros_like(xyz, requires_grad=True) + 0` and retain_grad()s it (:31-35): a fill, an add and a
    # non-leaf whose .grad its caller reads.  Nothing ever reads the VALUES of means2D (it only carries the viewspace gradient),
    # so a fresh uninitialised leaf serves the same contract -- `.grad` populated by backward -- without the two launches.
    screenspace_points = torch.empty_like(pc.get_xyz).requires_grad_(True)
    means3D = pc.get_xyz
    cam = viewpoint_camera
    rs = _raster_settings(cam, pc, pipe, bg_color, scaling_modifier)
    rasterizer = GaussianRasterizer(raster_settings=rs)
    time = None   # built where it is needed: [P,1] for the reference's module, ONE element for the fused sampler (uniform time)
    means2D = screenspace_points
    opacity = pc._opacity
    scales, rotations, cov3D_precomp = pc._scaling, pc._rotation, None
    dx = feat = dshs = shs_final = dshs_l1 = plane_reg = None
    fused_glue = override_color is None and _glue_route(pc, pipe, stage)
    if "coarse" in stage:
        means3D_final, scales_final, rotations_final, opacity_final = means3D, scales, rotations, opacity
        if not fused_glue:
            shs_final = pc.get_features
    elif "fine" in stage:
        if fused_glue:
            # under autograd the plane regulariser is a term of the fine stage's loss
            hy = pc._deformation.deformation_net.args
            means3D_final, scales, rotations, opacity, dx, dshs, feat, plane_reg = _deform_fused(
                pc, cam["time"], stage, render_feat or torch.is_grad_enabled(),
                stage == "fine" and torch.is_grad_enabled() and hy.time_smoothness_weight != 0)
            scales_final, rotations_final, opacity_final = scales, rotations, opacity
        else:
            time = torch.full((means3D.shape[0], 1), float(cam["time"]), device=dev)
            (means3D_final, scales_final, rotations_final, opacity_final, shs_final, dx, feat, dshs) = pc._deformation(
                means3D, scales, rotations, opacity, pc.get_features, time)
    else:
        raise NotImplementedError
    colors_precomp = None
    if fused_glue:
        # one kernel per direction for exp / normalize / sigmoid / (shs + dshs) / eval_sh / clamp (include/s3g_glue.h)
        want_l1 = dshs is not None and torch.is_grad_enabled()  # mean|dshs| for the lambda_dshs regulariser, same pass
        glue_out = activations_and_colors(pc.active_sh_degree, pc._features_dc, pc._features_rest, dshs, pc.get_xyz,
                                          cam["campos"], scales, rotations, opacity, with_dshs_l1=want_l1)
        colors_precomp, scales_final, rotations_final, opacity = glue_out[:4]
        dshs_l1 = glue_out[4] if want_l1 else None
    else:
        scales_final = pc.scaling_activation(scales_final)
        rotations_final = pc.rotation_activation(rotations_final)
        opacity = pc.opacity_activation(opacity_final)
        if override_color is None:
            if getattr(pipe, "convert_SHs_python", True):
                shs_view = shs_final.transpose(1, 2).view(-1, 3, (pc.max_sh_degree + 1) ** 2)
                dir_pp = pc.get_xyz - cam["campos"].repeat(pc.get_features.shape[0], 1)  # NB: un-deformed xyz (reference :110)
                dir_pp_normalized = dir_pp / dir_pp.norm(dim=1, keepdim=True)
                colors_precomp = torch.clamp_min(eval_sh(pc.active_sh_degree, shs_view, dir_pp_normalized) + 0.5, 0.0)
        else:
            colors_precomp = override_color
    if colors_precomp is not None:
        shs_final = None
    if getattr(pipe, "compute_cov3D_python", False):
        # gaussian_renderer/__init__.py:76-77: the 3-D covariance built in Python from the UNDEFORMED scaling / rotation and handed
        # to the rasterizer in place of the (scale, rotation) pair.  (The reference's own render() goes on to call
        # torch.exp(None) with this switch; here the switch simply does what its comment says.)
        cov3D_precomp = covariance_from_scaling_rotation(pc.scaling_activation(pc._scaling), scaling_modifier, pc._rotation)
        scales_final = rotations_final = None
    want_feat = render_feat and "fine" in stage
    decomposed = None
    if (return_decomposition and dx is not None and means3D_final.is_cuda and not torch.is_grad_enabled()
            and not want_feat and getattr(pipe, "fused_decomposition", True)):
        # evaluation path: full + dynamic-only + static-only renders from ONE preprocess / binning / sort
        max_values = torch.max(torch.abs(dx), dim=1)[0]
        dynamic_mask = max_values > torch.mean(max_values)
        decomposed = rasterizer.forward_decomposed(means3D=means3D_final, opacities=opacity, dynamic_mask=dynamic_mask,
                                                   shs=shs_final, colors_precomp=colors_precomp, scales=scales_final,
                                                   rotations=rotations_final, cov3D_precomp=cov3D_precomp,
                                                   **({"with_alpha": True} if return_alpha else {}))
    pair = want_feat and colors_precomp is not None and means3D_final.is_cuda and getattr(pipe, "fused_pair", True)
    # the bookkeeping rides in the pair node's backward only when that node really is the fused one (forward_pair falls back to
    # two ordinary nodes for P == 0 or debug snapshots); otherwise training_step runs the separate pass (optim.densify_stats)
    fuse_stats = bool(densify_accum is not None and pair and means3D_final.shape[0] > 0 and not rs.debug)
    if decomposed is not None:
        rendered_image, radii, depth, rendered_image2, alpha = (decomposed["render"], decomposed["radii"], decomposed["depth"], None,
                                                                decomposed.get("alpha"))
    else:
        rendered_image, radii, depth, rendered_image2, alpha = _rasterize_view(
            rasterizer, means3D_final, means2D, opacity, scales_final, rotations_final, cov3D_precomp, shs_final, colors_precomp,
            want_feat, feat, pair, return_alpha, densify_accum if fuse_stats else None)
    out = _view_result(rendered_image, screenspace_points, radii, depth, rendered_image2, alpha, want_feat, return_alpha,
                       return_dx and "fine" in stage, dx, dshs, dshs_l1, plane_reg)
    if densify_accum is not None:
        out["densify_stats_fused"] = fuse_stats
    if decomposed is not None:
        vis = out["visibility_filter"]
        out.update({"render_d": decomposed["render_d"], "depth_d": decomposed["depth_d"],
                    "render_s": decomposed["render_s"], "depth_s": decomposed["depth_s"]})
        out.set_lazy("visibility_filter_d", lambda: vis[dynamic_mask])    # boolean indexing = a host sync each: on demand
        out.set_lazy("visibility_filter_s", lambda: vis[~dynamic_mask])
    elif return_decomposition and dx is not None:
        max_values = torch.max(torch.abs(dx), dim=1)[0]
        dynamic_mask = max_values > torch.mean(max_values)
        for tag, m in (("d", dynamic_mask), ("s", ~dynamic_mask)):
            img, rad, dep = rasterizer(means3D=means3D_final[m], means2D=means2D[m],
                                       shs=shs_final[m] if shs_final is not None else None,
                                       colors_precomp=colors_precomp[m] if colors_precomp is not None else None,
                                       opacities=opacity[m],
                                       scales=scales_final[m] if scales_final is not None else None,
                                       rotations=rotations_final[m] if rotations_final is not None else None,
                                       cov3D_precomp=cov3D_precomp[m] if cov3D_precomp is not None else None)
            out.update({f"render_{tag}": img, f"depth_{tag}": dep, f"visibility_filter_{tag}": rad > 0})
    if extra_colors is not None:
        P = means3D_final.shape[0]
        extra = []
        for c in extra_colors:
            if not torch.is_tensor(c) or tuple(c.shape) != (P, 3) or c.device != means3D_final.device:
                raise RuntimeError(f"render: every entry of extra_colors must be a [{P},3] tensor on the Gaussians' device")
            extra.append(rasterizer(means3D=means3D_final, means2D=means2D, shs=None, colors_precomp=c, opacities=opacity,
                                    scales=scales_final, rotations=rotations_final, cov3D_precomp=cov3D_precomp)[0])
        out["extra"] = extra
    if sky_model is not None:
        _sky_compose(out, sky_model, cam)
    return out


# ---- losses (utils/loss_utils.py, scene/regulation.py) -----------------------------------------------------------
def l1_loss(a, b):
    return torch.abs(a - b).mean()


def l2_loss(a, b):
    return ((a - b) ** 2).mean()


def compute_depth_l2(pred, gt, max_depth: float = 80.0):
    pred, gt = pred.squeeze(), gt.squeeze()
    m = (gt > 0.01) & (gt < max_depth)
    return F.mse_loss(torch.clamp(pred[m] / max_depth, 0.0, 1.0), torch.clamp(gt[m] / max_depth, 0.0, 1.0))


_ssim_windows = {}


def ssim(img1, img2, window_size=11):
    ch = img1.size(-3)
    key = (ch, window_size, img1.device, img1.dtype)
    if key not in _ssim_windows:
        g = torch.tensor([math.exp(-(x - window_size // 2) ** 2 / float(2 * 1.5 ** 2)) for x in range(window_size)])
        g = (g / g.sum()).unsqueeze(1)
        _ssim_windows[key] = g.mm(g.t()).float()[None, None].expand(ch, 1, window_size, window_size).contiguous().to(img1)
    w, pad = _ssim_windows[key], window_size // 2
    mu1, mu2 = F.conv2d(img1, w, padding=pad, groups=ch), F.conv2d(img2, w, padding=pad, groups=ch)
    mu1_sq, mu2_sq, mu12 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = F.conv2d(img1 * img1, w, padding=pad, groups=ch) - mu1_sq
    s2 = F.conv2d(img2 * img2, w, padding=pad, groups=ch) - mu2_sq
    s12 = F.conv2d(img1 * img2, w, padding=pad, groups=ch) - mu12
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu12 + c1) * (2 * s12 + c2)) / ((mu1_sq + mu2_sq + c1) * (s1 + s2 + c2))).mean()


def _plane_smoothness(t):
    d1 = t[..., 1:, :] - t[..., :-1, :]
    d2 = d1[..., 1:, :] - d1[..., :-1, :]
    return torch.square(d2).mean()


def psnr(img1, img2):
    mse = ((img1 - img2) ** 2).reshape(img1.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


def evaluate(pc: GaussianParams, cameras, gt_images, pipe: SimpleNamespace, bg: torch.Tensor, masks=None, stage="fine",
             return_decomposition=False, lpips=None, pose=None, sky_model=None) -> Dict:
    """The metric part of the reference's evaluation loop (utils/video_utils.py:169-241, 301-307): every camera is rendered under
    no_grad, frame i's {psnr, ssim, masked_psnr, masked_ssim, masked_pixels} goes into row i of one [N,5] device tensor
    (metrics.image_metrics), and that tensor is read back ONCE after the last frame.  masks: None, or one entry per camera (None
    for a camera without a dynamic mask).  The four scalars are the reference's `non_zero_mean`: the mean over the frames that
    contributed -- for the masked pair the frames with at least one masked pixel -- and -1 when none did.  "per_frame" is the
    [N,5] table on the host.
    lpips: None, or an s3gaussian_amd.lpips.LPIPS model (AlexNet, what utils/video_utils.py reports) or an
    s3gaussian_amd.lpips_vgg.LPIPSVGG model (VGG16, what metrics.py reports), with the caller's weights: frame i's
    {total, tap0..tap4} goes into row i of an [N,6] device tensor that is read back with the metrics table; the result gains "lpips"
    (non_zero_mean of the totals, utils/video_utils.py:210, 305) and "lpips_per_frame" ([N,6] float64 on the host), the same keys
    for either model.  Without a model nothing changes.
    pose: None, or a pose.PoseRefiner with one row per camera: camera i is rendered at pose.corrected(camera, i) (training views at
    their refined poses; no gradient flows here).
    sky_model: None, or a skymodel.SkyModel: every frame is render(sky_model=...)'s composite and the metrics are computed on it
    (`bg` is then not used); refused together with pose=."""
    if sky_model is not None:
        _sky_refusals("evaluate", sky_model, pose)
    n = len(cameras)
    if len(gt_images) != n or (masks is not None and len(masks) != n):
        raise RuntimeError("evaluate: one ground-truth image (and one mask entry) per camera")
    table = torch.empty((n, _metrics.RECORD), dtype=torch.float64, device=pc.get_xyz.device)
    lpips_fn, lpips_table = _lpips_table(lpips, n, pc.get_xyz.device)
    with torch.no_grad():
        for i, cam in enumerate(cameras):
            pkg = render(cam, pc, pipe, bg, stage=stage, return_decomposition=return_decomposition,
                         **({"pose": pose, "cam_index": i} if pose is not None else {}),
                         **({"sky_model": sky_model} if sky_model is not None else {}))
            _metrics.image_metrics(pkg["render"], gt_images[i], None if masks is None else masks[i], out=table[i])
            if lpips is not None:
                lpips_fn(lpips, pkg["render"], gt_images[i], out=lpips_table[i])
    per_frame = table.cpu()
    non_zero_mean = lambda x: float(x.sum() / len(x)) if len(x) > 0 else -1      # video_utils.py:44-46
    contributed = per_frame[:, _metrics.MASKED_PIXELS] > 0
    result = {"psnr": non_zero_mean(per_frame[:, _metrics.PSNR]), "ssim": non_zero_mean(per_frame[:, _metrics.SSIM]),
              "masked_psnr": non_zero_mean(per_frame[contributed, _metrics.MASKED_PSNR]),
              "masked_ssim": non_zero_mean(per_frame[contributed, _metrics.MASKED_SSIM]), "per_frame": per_frame}
    if lpips is not None:
        lpips_per_frame = lpips_table.cpu()
        result.update({"lpips": non_zero_mean(lpips_per_frame[:, _lpips.TOTAL]), "lpips_per_frame": lpips_per_frame})
    return result


def _lpips_table(model, n: int, device):
    """(the per-frame call of the model's kind, the [N,6] device table evaluate() and evaluate_video() fill with it); (None, None)
    without a model.  Both kinds write the same record."""
    if model is None:
        return None, None
    if isinstance(model, _lpips.LPIPS):
        fn = _lpips.lpips
    elif isinstance(model, _lpips_vgg.LPIPSVGG):
        fn = _lpips_vgg.lpips_vgg
    else:
        raise TypeError("evaluate: lpips must be None, an s3gaussian_amd.lpips.LPIPS model or an s3gaussian_amd.lpips_vgg.LPIPSVGG model")
    return fn, torch.empty((n, _lpips.RECORD), dtype=torch.float64, device=device)


def _fused_route(pc: GaussianParams, pipe: SimpleNamespace) -> bool:
    """render() takes the fused deformation route for this model AND the model has a position head (a static model, no_dx=True,
    takes the route too, but produces no dx: nothing to colour a flow with or to split dynamic from static by): GPU tensors, the
    plain-grid network with any head configuration that has a position head (Deformation._fused_any: with or without the scale /
    rotation / opacity, SH and feature heads), SH degree 3, convert_SHs_python and fused_glue on."""
    return _glue_route(pc, pipe, "fine") and not pc._deformation.deformation_net.args.no_dx


def _fused_route_missing(pc: GaussianParams, pipe: SimpleNamespace) -> str:
    """What `_fused_route` asks for, led by the switch that keeps this model off it."""
    net = pc._deformation.deformation_net
    a = net.args
    if a.no_dx and net._fused_any():
        lead = "the model was built with no_dx (a static scene): it has no dx to colour a flow with or to split dynamic from static by"
    else:
        off = [k for k in ("grid_pe", "no_grid", "static_mlp", "empty_voxel") if getattr(a, k, False)]
        lead = (f"the switch {' / '.join(off)} puts the network on the library route" if off else
                "this model or pipe is not on it") + (" (and no_dx is set: a static model has no dx)" if a.no_dx else "")
    return (lead + ".  Needed: GPU tensors, a plain-grid network (defor_depth 1, net_width 64, 128 grid features) with a position head "
            "(not no_dx; the other five heads on or off), SH degree 3, convert_SHs_python and fused_glue on")


@torch.no_grad()
def render_flows(pc: GaussianParams, cameras, pipe: SimpleNamespace, bg: torch.Tensor, num_cams: int = 3, sink=None,
                 with_rgb: bool = False, return_decomposition: bool = False, on_frame=None, return_alpha: bool = False,
                 sky_model=None) -> Dict:
    """The forward and backward scene-flow images of the reference's evaluation loop (utils/video_utils.py:203-209, 252-299): frame t,
    rendered in stage "fine" at its own camera and time, painted with C(dx[t + n] - dx[t]) and C(dx[t] - dx[t - n]) (flow.frame_plan,
    n = num_cams; C = flow.scene_flow_colors).  `cameras` in dataset order: num_cams cameras per timestamp.

    Where the reference keeps dx of every frame, evaluates the colours per image through the host and pays a whole render -- plain
    PyTorch deformation, preprocess, binning, sort -- per image:
      * dx is evaluated once per distinct cam["time"] (net.deform_heads, one timestamp ahead of the frames being rendered); the frame's
        own render() then finds that evaluation in the inference cache.  At most three timestamps' dx are alive (and two cached
        evaluations: the current timestamp's and the next one's);
      * the colours are evaluated once per distinct (time_a, time_b) and serve every camera of both timestamps, as the forward flow of
        the earlier and the backward flow of the later;
      * both images of a frame come from ONE render(..., extra_colors=[ff, bf]): one geometry, two more blend passes.

    -> {"forward_flows": [...], "backward_flows": [...]} (+ "rgbs" with with_rgb=True): one [3,H,W] device tensor per frame.  The
    reference's lists hold `image.permute(1, 2, 0).cpu().numpy()` of the same images ([H,W,3]).
    sink(kind, frame_index, image), kind in ("forward", "backward", "rgb"): every image is handed over as soon as it exists and none
    is kept (the lists come back empty): 150 frames x 2 x 20 MB need not stay resident.
    return_decomposition and return_alpha are passed on to each frame's render(); on_frame(i, pkg) is called with frame i's full render result (its
    "extra" holds the forward flow image first and the backward one last) before the images are delivered: evaluate_video hangs the
    rest of the evaluation on the same render this way.
    sky_model: each frame's render(sky_model=...): "rgbs" (and on_frame's pkg["render"]) are the composite; the flow images stay
    over black and `bg` is not used.
    Needs the fused deformation route (the reference's default head configuration, SH degree 3, on the GPU): there is no second
    implementation behind it."""
    from . import flow as _flow
    forward_plan, backward_plan = _flow.frame_plan(len(cameras), num_cams)
    net = pc._deformation.deformation_net
    xyz = pc.get_xyz
    if not _fused_route(pc, pipe):
        raise RuntimeError("render_flows needs the fused deformation route: " + _fused_route_missing(pc, pipe))
    dev = xyz.device
    times = [float(cam["time"]) for cam in cameras]
    window: Dict[float, torch.Tensor] = {}      # timestamp -> dx
    entries: Dict[float, object] = {}           # timestamp -> the deformation's cached evaluation (dx, dshs) of it
    colors: Dict[tuple, torch.Tensor] = {}      # (time_a, time_b) -> C(dx[time_b] - dx[time_a])
    result = {"forward_flows": [], "backward_flows": []}
    if with_rgb:
        result["rgbs"] = []

    def deliver(kind, key, i, image):
        if sink is not None:
            sink(kind, i, image)
        else:
            result[key].append(image)

    for i, cam in enumerate(cameras):
        pairs = [(times[p.from_frame], times[p.to_frame]) for p in (forward_plan[i], backward_plan[i])]
        needed = {t for pair in pairs for t in pair} | {times[i]}
        for t in [t for t in window if t not in needed]:
            del window[t]
            entries.pop(t, None)
        for key in [key for key in colors if key[0] not in needed or key[1] not in needed]:
            del colors[key]
        for t in sorted(needed - set(window), key=lambda t: t == times[i]):      # the frame's own timestamp last: its entry stays installed
            window[t] = net.deform_heads(xyz, _uniform_time(t, dev), uniform_time=True, reg_weights=None, need_feat=False)[0]
            entries[t] = net.inference_cache_entry()
        net.install_inference_cache(entries.get(times[i]))
        for pair in pairs:
            if pair not in colors:
                colors[pair] = _flow.scene_flow_colors(window[pair[0]], window[pair[1]])
        unique = [colors[pairs[0]]] + ([colors[pairs[1]]] if pairs[1] != pairs[0] else [])
        pkg = render(cam, pc, pipe, bg, stage="fine", return_decomposition=return_decomposition, extra_colors=unique,
                     **({"return_alpha": True} if return_alpha else {}),
                     **({"sky_model": sky_model} if sky_model is not None else {}))
        if on_frame is not None:
            on_frame(i, pkg)
        if with_rgb:
            deliver("rgb", "rgbs", i, pkg["render"])
        deliver("forward", "forward_flows", i, pkg["extra"][0])
        deliver("backward", "backward_flows", i, pkg["extra"][-1])
        if i + 1 == len(cameras) or times[i + 1] != times[i]:
            entries[times[i]] = None             # the timestamp's frames are done: only its dx is still needed, not its dshs
    return result


def dynamic_point_count(dx: torch.Tensor) -> torch.Tensor:
    """The "dynamic point" number of the reference's training log (train.py:445-452): #{i : max|dx_i| > mean_j max|dx_j|}, as a 0-dim
    int32 tensor on dx's device.  Nothing here waits for the device (no boolean index, no .item()): the caller reads the number when
    it logs, which keeps run_training_steps host-asynchronous."""
    from . import split
    return split.motion_classify(dx)[2]


@torch.no_grad()
def save_split_point_clouds(pc: GaussianParams, time: float, dynamic_pcd_path: str, static_pcd_path: str, stage: str = "fine") -> Dict:
    """The export of utils/video_utils.py:243-250 (`save_seperate_pcd`) for one timestamp: the deformation is evaluated once at
    `time` through net.deform_heads -- a frame of that timestamp rendered before or after shares the evaluation through the inference
    cache -- and the model is split by that dx exactly as GaussianParams.save_ply_split splits it.
    A static model (no_dx) is refused: it has no dx to tell moving from static by; so is any stage without a deformation.
    -> {"n_dynamic", "n_static", "thre"}."""
    from . import split
    net = pc._deformation.deformation_net
    if net.args.no_dx:
        raise RuntimeError("save_split_point_clouds: the model was built with no_dx (a static scene): there is no dx to split "
                           "dynamic from static points by")
    if "fine" not in stage:
        raise RuntimeError(f"save_split_point_clouds: stage {stage!r} has no deformation; only the fine stage has a dx")
    xyz = pc.get_xyz
    if not (xyz.is_cuda and net._fused_any()):
        raise RuntimeError("save_split_point_clouds needs GPU tensors and a network on the fused deformation route (plain grid: not "
                           "grid_pe / no_grid / static_mlp / empty_voxel; defor_depth 1, net_width 64, 128 grid features)")
    dx = net.deform_heads(xyz, _uniform_time(float(time), xyz.device), uniform_time=True, reg_weights=None, need_feat=False)[0]
    return split.export_split(pc, dx, dynamic_pcd_path, static_pcd_path)


@torch.no_grad()
def scene_from_lidar(sweeps, l2ws, c2ws, Ks, H: int, W: int, sh_degree: int = 3, hyper: Optional[SimpleNamespace] = None,
                     device="cuda:0", x_range=(-2.0, 80.0), depth_range=(0.01, 80.0), point_offset: int = 3,
                     voxel_size: float = 0.013, num_pts: Optional[int] = None, generator: Optional[torch.Generator] = None) -> Dict:
    """The LiDAR part of the reference's set-up (readWaymoInfo, scene/dataset_readers.py:752-779, 824-977) at ANY image size.

    sweeps: T fp32 [N_t,stride] tables (lidar.read_sweep gives the raw [N,10] rows; host tensors are uploaded once, as they are).
    l2ws [T,4,4], c2ws [T*V,4,4], Ks [T*V,3,3]: float64 host arrays, the cameras timestamp-major as the reference lists them.
    -> {"depth_maps": [T*V,H,W] fp32 (row t*V + v feeds the depth L2 term of camera v at timestamp t as gt_depth[None]),
        "xyz": [M,3] fp32 and "colors": [M,3] float64, what GaussianParams.create_from_points takes,
        "aabb": float64 [2,3] host array (min, max) of the camera frustums, what the deformation field's set_aabb(max, min) takes}
    and, when `hyper` is given, "gaussians": GaussianParams(sh_degree, hyper) created from the three."""
    import numpy as np
    from . import lidar
    dev = torch.device(device)
    c2ws, Ks, l2ws = _np_f64(c2ws), _np_f64(Ks), _np_f64(l2ws)
    T = len(sweeps)
    if T < 1 or l2ws.shape[0] != T or c2ws.shape[0] % T != 0 or Ks.shape[0] != c2ws.shape[0]:
        raise ValueError(f"scene_from_lidar: {T} sweeps, l2ws {l2ws.shape}, c2ws {c2ws.shape}, Ks {Ks.shape}: expected [T,4,4], [T*V,4,4], [T*V,3,3]")
    V = c2ws.shape[0] // T
    aabb = lidar.frustum_aabb(c2ws, Ks, H, W, depth_range)
    tables = [s.to(dev) for s in sweeps]
    cloud = lidar.LidarCloud(aabb, sum(int(s.shape[0]) for s in tables), dev)
    maps = torch.empty((T * V, H, W), dtype=torch.float32, device=dev)
    workspace = torch.empty(V * H * W, dtype=torch.int32, device=dev)
    for t, rows in enumerate(tables):
        w2c = np.stack([np.linalg.inv(c2ws[t * V + v]) for v in range(V)])
        lidar.depth_maps(rows, l2ws[t], w2c, Ks[t * V:(t + 1) * V], H, W, x_range, point_offset, out=maps[t * V:(t + 1) * V],
                         workspace=workspace)
        cloud.add(rows, l2ws[t], x_range, point_offset)
    xyz = cloud.finish(voxel_size, num_pts, generator)
    colors = lidar.init_colors(xyz.shape[0], generator)
    out = {"depth_maps": maps, "xyz": xyz, "colors": colors, "aabb": aabb}
    if hyper is not None:
        pc = GaussianParams(sh_degree, hyper).create_from_points(xyz, colors, dev)
        pc._deformation.deformation_net.set_aabb(aabb[1].tolist(), aabb[0].tolist())
        out["gaussians"] = pc
    return out


def _np_f64(a):
    import numpy as np
    return np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a, dtype=np.float64)


VIDEO_KEYS = ("gt_rgbs", "rgbs", "depths", "dynamic_rgbs", "static_rgbs", "forward_flows", "backward_flows")
SKY_VIDEO_KEYS = ("opacities", "sky_masks", "gt_sky_masks")       # asked for through evaluate_video(sky_keys=...), not through keys=
DEPTH_VIDEO_KEYS = ("depth_colors",)                              # asked for through evaluate_video(depth_keys=...)
_VIDEO_SOURCE = {"rgbs": "render", "depths": "depth", "dynamic_rgbs": "render_d", "static_rgbs": "render_s", "opacities": "alpha"}
_VIDEO_ONE_CHANNEL = ("depths", "opacities")


def evaluate_video(pc: GaussianParams, cameras, gt_images, pipe: SimpleNamespace, bg: torch.Tensor, masks=None, num_cams: int = 3,
                   keys=("gt_rgbs", "rgbs", "depths", "dynamic_rgbs", "static_rgbs"), sink=None, host: bool = False,
                   compute_metrics: bool = True, stage: str = "fine", lpips=None, sky_keys=(), sky_masks=None, depth_keys=(),
                   depth_bounds=(4.0, 120.0), pose=None, sky_model=None) -> Dict:
    """The reference's evaluation loop with its videos' frames (utils/video_utils.py:116-349 render_func, then 439-499
    save_seperate_videos) from ONE render per camera: render(cam, return_decomposition=<a decomposition key is asked for>,
    extra_colors=<the frame's flow colours, if a flow key is asked for>) feeds metrics.image_metrics -- row i of the [N,5] table,
    exactly as evaluate() fills it -- and one frames.compose call with one job per key, which writes camera (i % num_cams)'s tile of
    timestamp (i // num_cams)'s strips; the fp32 images are dropped right after.

    keys: any of VIDEO_KEYS.  A strip is the [H, num_cams * W, C] uint8 array the reference appends to the key's video writer for
    one timestamp -- to8b of the cameras' images side by side; C = 1 for "depths", whose frames are each divided by their own maximum,
    and for "opacities".
    sky_keys: any of SKY_VIDEO_KEYS, delivered like the keys of `keys` and behind them (frames, middle, sink; `keys` itself goes on
    accepting the seven names the reference's render_func fills and refusing every other; both together at most 8 strips).
    "opacities", "sky_masks", "gt_sky_masks" are the keys save_seperate_videos has code for (utils/video_utils.py:461-471) and the
    reference's render_func never fills: the accumulated opacity of each render (render(return_alpha=True)); 1 - opacity, evaluated in
    fp32 from the opacity image and replicated to three channels (`1 - np.stack([frame] * 3, axis=-1)`); and the caller's
    `sky_masks` (one [H,W] / [1,H,W] tensor per camera, required by "gt_sky_masks"), replicated likewise.
    depth_keys: any of DEPTH_VIDEO_KEYS, delivered like the other strips and behind the sky keys.  "depth_colors" is the reference's
    depth_visualizer (utils/video_utils.py:27-33, the call save_seperate_videos carries commented out, :472-479): the render's depth
    through the turbo map with the log curve, weighted by the render's accumulated opacity (render(return_alpha=True)), an
    [H, num_cams * W, 3] strip written by depthvis.depth_colors beside the compose call -- not a compose job, not counted against
    the 8.  depth_bounds = (lo, hi) as depth_colors takes them; a None entry is that frame's own opacity-weighted percentile bound,
    found on the device.
    T = len(cameras) // num_cams timestamps; leftover cameras are rendered and counted in the metrics and appear in no strip.
    When a timestamp's last camera has been composed each of its strips goes to sink(key, timestamp_index, strip), in the order of
    `keys`; without a sink into result["frames"][key] (with one, those lists stay empty).  result["middle"][key] is the strip of
    timestamp T // 2, the reference's return_frame_dict.
    host=True: the strips arrive as numpy arrays, through two pinned slots per key filled with non_blocking copies: timestamp i is
    handed over after the work of timestamp i + 1 has been enqueued (the last one at the end), behind an event that has long fired by
    then, so no frame waits for the device.  A sink receives a view of the pinned slot, valid until it returns (what a video
    writer's append_data needs); the lists and "middle" hold copies.
    -> {"psnr", "ssim", "masked_psnr", "masked_ssim", "per_frame"} as evaluate() (-1 / None with compute_metrics=False),
    "frames", "middle", "num_timestamps".  File names and the encoder stay with the caller.
    lpips: None, or an LPIPS (AlexNet) or LPIPSVGG (VGG16) model: as in evaluate(), the result gains "lpips" and "lpips_per_frame" (it needs
    compute_metrics=True).
    Flow keys run the loop through render_flows (its windowing of dx and colours; stage "fine", at least 2 * num_cams cameras); they
    and the decomposition keys need the fused deformation route, as render_flows does.
    sky_model: None, or a skymodel.SkyModel: every frame is render(sky_model=...); the metrics and the "rgbs" strips are computed on
    the composite (the decomposition and flow strips stay over black; `bg` is not used).  Refused together with pose=."""
    from . import depthvis as _depthvis
    from . import frames as _frames
    if sky_model is not None:
        _sky_refusals("evaluate_video", sky_model, pose)
    sky_kw = {"sky_model": sky_model} if sky_model is not None else {}
    keys, sky_keys, depth_keys = tuple(keys), tuple(sky_keys), tuple(depth_keys)
    unknown = [k for k in keys if k not in VIDEO_KEYS]
    if unknown or not (keys or sky_keys or depth_keys) or len(set(keys)) != len(keys) or len(keys) > _frames.MAX_JOBS:
        raise RuntimeError(f"evaluate_video: keys must be distinct entries of {VIDEO_KEYS} (got {keys}); "
                           f"{SKY_VIDEO_KEYS} are asked for through sky_keys=, {DEPTH_VIDEO_KEYS} through depth_keys=")
    if any(k not in DEPTH_VIDEO_KEYS for k in depth_keys) or len(set(depth_keys)) != len(depth_keys):
        raise RuntimeError(f"evaluate_video: depth_keys must be distinct entries of {DEPTH_VIDEO_KEYS} (got {depth_keys})")
    depth_bounds = tuple(depth_bounds)
    if len(depth_bounds) != 2 or any(b is not None and float(b) != float(b) for b in depth_bounds):
        raise RuntimeError(f"evaluate_video: depth_bounds must be (lo, hi), each a number or None (got {depth_bounds})")
    if any(k not in SKY_VIDEO_KEYS for k in sky_keys) or len(set(sky_keys)) != len(sky_keys) or len(keys) + len(sky_keys) > _frames.MAX_JOBS:
        raise RuntimeError(f"evaluate_video: sky_keys must be distinct entries of {SKY_VIDEO_KEYS} (got {sky_keys}), and keys and "
                           f"sky_keys together at most {_frames.MAX_JOBS}")
    compose_keys = keys + sky_keys                 # the jobs of frames.compose; the depth keys' strips follow them
    keys = compose_keys + depth_keys
    if pose is not None:    # a pose.PoseRefiner with one row per camera: every frame at its refined pose (no gradient flows here)
        with torch.no_grad():
            cameras = [pose.corrected(cam, i) for i, cam in enumerate(cameras)]
    n, N = int(num_cams), len(cameras)
    if n == 5:
        raise RuntimeError("evaluate_video: num_cams = 5 is refused: the reference rescales the two outer views of five with "
                           "resize_five_views (a scipy spline zoom), which is deliberately not rebuilt here")
    if n < 1:
        raise RuntimeError(f"evaluate_video: num_cams = {num_cams}")
    if len(gt_images) != N or (masks is not None and len(masks) != N):
        raise RuntimeError("evaluate_video: one ground-truth image (and one mask entry) per camera")
    if "gt_sky_masks" in keys and (sky_masks is None or len(sky_masks) != N):
        raise RuntimeError('evaluate_video: the sky key "gt_sky_masks" needs sky_masks=, one mask per camera')
    want_alpha = any(k in ("opacities", "sky_masks") for k in keys) or bool(depth_keys)
    want_flow = any(k in ("forward_flows", "backward_flows") for k in keys)
    want_dec = any(k in ("dynamic_rgbs", "static_rgbs") for k in keys)
    if (want_flow or want_dec) and not (_fused_route(pc, pipe) and "fine" in stage):
        raise RuntimeError("evaluate_video: the decomposition and flow keys need the fused deformation route in a fine stage: "
                           + _fused_route_missing(pc, pipe))
    if want_flow and stage != "fine":
        raise RuntimeError('evaluate_video: the flow keys are rendered by render_flows, in stage "fine"')
    dev = pc.get_xyz.device
    T = N // n
    table = torch.empty((N, _metrics.RECORD), dtype=torch.float64, device=dev) if compute_metrics else None
    if lpips is not None and not compute_metrics:
        raise RuntimeError("evaluate_video: lpips needs compute_metrics=True")
    lpips_fn, lpips_table = _lpips_table(lpips, N, dev)
    result = {"frames": {k: [] for k in keys}, "middle": {}, "num_timestamps": T}
    normalize = [k == "depths" for k in compose_keys]
    state = SimpleNamespace(strips=None, size=None, pending=None, ring={})

    def hand_over(t, strips):                  # device strips, or views of the pinned slots
        for k, s in zip(keys, strips):
            if t == T // 2:
                result["middle"][k] = s.copy() if host else s
            if sink is not None:
                sink(k, t, s)
            else:
                result["frames"][k].append(s.copy() if host else s)

    def drain(pending):
        if pending is not None:
            t, event, slots = pending
            event.synchronize()                # recorded one timestamp of work ago
            hand_over(t, [s.numpy() for s in slots])

    def finish_timestamp(t):
        if not host:
            hand_over(t, state.strips)
            return
        slots = []
        for k, s in zip(keys, state.strips):
            ring = state.ring.get(k)
            if ring is None or ring[0].shape != s.shape:
                ring = state.ring[k] = [torch.empty(s.shape, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
            slots.append(ring[t % 2])          # timestamp t - 2 left this slot when t - 1's work was enqueued
            slots[-1].copy_(s, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        previous, state.pending = state.pending, (t, event, slots)
        drain(previous)                        # timestamp t - 1: everything of t is enqueued behind it

    def on_frame(i, pkg):
        H, W = int(pkg["render"].shape[1]), int(pkg["render"].shape[2])
        gt = gt_images[i]
        if not torch.is_tensor(gt) or tuple(gt.shape) != (3, H, W):
            raise RuntimeError(f"evaluate_video: gt_images[{i}] must be a [3,{H},{W}] tensor "
                               f"(got {tuple(gt.shape) if torch.is_tensor(gt) else type(gt).__name__})")
        if compute_metrics:
            _metrics.image_metrics(pkg["render"], gt, None if masks is None else masks[i], out=table[i])
            if lpips is not None:
                lpips_fn(lpips, pkg["render"], gt, out=lpips_table[i])
        t, c = divmod(i, n)
        if t >= T:
            return
        if c == 0:
            state.size = (H, W)
            state.strips = [torch.empty(_frames.strip_shape(H, W, 1 if k in _VIDEO_ONE_CHANNEL else 3, n), dtype=torch.uint8, device=dev)
                            for k in keys]
        elif state.size != (H, W):
            raise RuntimeError(f"evaluate_video: camera {i} renders {H} x {W}, the first camera of its timestamp "
                               f"{state.size[0]} x {state.size[1]}: one strip holds images of one size")
        images = []
        for k in compose_keys:
            if k == "gt_rgbs":
                images.append(gt)
            elif k == "forward_flows":
                images.append(pkg["extra"][0])
            elif k == "backward_flows":
                images.append(pkg["extra"][-1])
            elif k == "sky_masks":           # prepared outside frames.compose: 1 - opacity in fp32, three equal channels
                images.append((1.0 - pkg["alpha"]).expand(3, H, W))
            elif k == "gt_sky_masks":
                m = sky_masks[i]
                if not torch.is_tensor(m) or m.numel() != H * W:
                    raise RuntimeError(f"evaluate_video: sky_masks[{i}] must be a tensor of {H} x {W} elements")
                images.append(m.to(dev).float().reshape(1, H, W).expand(3, H, W))
            else:
                if _VIDEO_SOURCE[k] not in pkg:
                    raise RuntimeError(f'evaluate_video: render() returned no "{_VIDEO_SOURCE[k]}" for key "{k}" on this route')
                images.append(pkg[_VIDEO_SOURCE[k]])
        if compose_keys:
            _frames.compose(images, state.strips[:len(compose_keys)], c, normalize=normalize)
        for s in state.strips[len(compose_keys):]:          # "depth_colors"
            _depthvis.depth_colors(pkg["depth"], pkg["alpha"], depth_bounds[0], depth_bounds[1], out=s, cam=c, num_cams=n)
        if c == n - 1:
            finish_timestamp(t)
            state.strips = None

    with torch.no_grad():
        if want_flow:
            render_flows(pc, cameras, pipe, bg, num_cams=n, sink=lambda kind, i, image: None, return_decomposition=want_dec,
                         on_frame=on_frame, **({"return_alpha": True} if want_alpha else {}), **sky_kw)
        else:
            for i, cam in enumerate(cameras):
                on_frame(i, render(cam, pc, pipe, bg, stage=stage, return_decomposition=want_dec,
                                   **({"return_alpha": True} if want_alpha else {}), **sky_kw))
        drain(state.pending)
    if not compute_metrics:
        result.update({"psnr": -1, "ssim": -1, "masked_psnr": -1, "masked_ssim": -1, "per_frame": None})
        return result
    per_frame = table.cpu()
    non_zero_mean = lambda x: float(x.sum() / len(x)) if len(x) > 0 else -1      # video_utils.py:44-46
    contributed = per_frame[:, _metrics.MASKED_PIXELS] > 0
    result.update({"psnr": non_zero_mean(per_frame[:, _metrics.PSNR]), "ssim": non_zero_mean(per_frame[:, _metrics.SSIM]),
                   "masked_psnr": non_zero_mean(per_frame[contributed, _metrics.MASKED_PSNR]),
                   "masked_ssim": non_zero_mean(per_frame[contributed, _metrics.MASKED_SSIM]), "per_frame": per_frame})
    if lpips is not None:
        lpips_per_frame = lpips_table.cpu()
        result.update({"lpips": non_zero_mean(lpips_per_frame[:, _lpips.TOTAL]), "lpips_per_frame": lpips_per_frame})
    return result


_weight_cache: Dict = {}


class _WeightedTerms(torch.autograd.Function):
    """sum_i w_i * term_i  +  w_dx * mean|dx|   in three launches forward (L1 norm, stack, dot) and three backward (scale, sign,
    multiply) instead of the ~19 five-microsecond launches the same expression costs term by term (train.py:404-425 adds the
    regularisers one `loss = loss + ...` at a time; that section of the iteration is bound by the host's launch rate)."""

    @staticmethod
    def forward(ctx, dx, w_dx, weights, *terms):
        vals = list(terms)
        w = list(weights)
        if dx is not None and dx.numel() == 0:   # no Gaussians: mean|dx| of the reference is NaN; it contributes nothing here
            dx = None
        if dx is not None:
            vals.append(torch.linalg.vector_norm(dx, ord=1))
            w.append(w_dx / dx.numel())
        key = (tuple(w), vals[0].device)
        wt = _weight_cache.get(key)
        if wt is None:     # the weights are constants of the run (the dx weight changes with P): one upload each
            if len(_weight_cache) > 64:
                _weight_cache.clear()
            wt = _weight_cache[key] = torch.tensor(w, dtype=torch.float32, device=vals[0].device)
        ctx.save_for_backward(wt, dx if dx is not None else wt)
        ctx.has_dx, ctx.n = dx is not None, len(terms)
        ctx.term_shapes = [tuple(v.shape) for v in terms]   # a [1]-shaped term must get a [1]-shaped gradient back
        return torch.dot(torch.stack([v.reshape(()).float() for v in vals]), wt)

    @staticmethod
    def backward(ctx, g):
        wt, dx = ctx.saved_tensors
        gw = g * wt
        g_dx = torch.sign(dx) * gw[-1] if ctx.has_dx else None   # (None also for an empty dx: no gradient to give)
        return (g_dx, None, None, *(gi.reshape(sh) for gi, sh in zip(gw[:ctx.n].unbind(0), ctx.term_shapes)))


def _sky_weight(opt, sky_mask) -> float:
    """lambda_sky if the sky term is on (a mask was handed in and the weight is not 0), else 0."""
    return float(getattr(opt, "lambda_sky", 0.0)) if sky_mask is not None else 0.0


def _wanted_regularisers(hyper, opt, stage: str):
    """-> (lambda_dx * mean|dx| wanted, lambda_dshs * mean|dshs| wanted, plane regulariser wanted)   (train.py:404-425)"""
    fine = "fine" in stage
    return (fine and not hyper.no_dx and opt.lambda_dx != 0, fine and not hyper.no_dshs and opt.lambda_dshs != 0,
            stage == "fine" and hyper.time_smoothness_weight != 0)


def _dshs_l1(pkg: Dict):
    return pkg["dshs_l1"] if "dshs_l1" in pkg else torch.mean(torch.abs(pkg["dshs"]))


def _plane_reg(pc: GaussianParams, pkgs, hyper):
    """The plane regulariser a render has already evaluated on its sampler node, else evaluated here."""
    reg = next((p["plane_reg"] for p in pkgs if p.get("plane_reg") is not None), None)
    return reg if reg is not None else pc.compute_regulation(hyper.time_smoothness_weight, hyper.l1_time_planes, hyper.plane_tv_weight)


def _with_regularisers(pc: GaussianParams, loss, pkg: Dict, pkgs, sky_term, lam_sky: float, hyper, opt, stage: str):
    """pixel-term loss + lambda_sky * sky_term (None: off) + the regularisers as ONE weighted node (_WeightedTerms): dx / dshs /
    dshs_l1 from `pkg`, the plane regulariser from whichever of `pkgs` carries it."""
    want_dx, want_dshs, want_reg = _wanted_regularisers(hyper, opt, stage)
    terms, weights = [loss], [1.0]
    if sky_term is not None:
        terms.append(sky_term)
        weights.append(lam_sky)
    if want_dshs:
        terms.append(_dshs_l1(pkg))
        weights.append(float(opt.lambda_dshs))
    if want_reg:
        terms.append(_plane_reg(pc, pkgs, hyper))
        weights.append(1.0)
    if len(terms) == 1 and not want_dx:
        return loss
    return _WeightedTerms.apply(pkg["dx"] if want_dx else None, float(opt.lambda_dx), tuple(weights), *terms)


def training_loss(pc: GaussianParams, pkg: Dict, gt_image, gt_depth, gt_feat, hyper, opt, stage="fine", fused_pixel_terms=True,
                  sky_mask=None):
    """train.py:395-425 for a batch of one view.  The per-pixel terms (L1, depth L2, DSSIM, feature L2) run as one fused
    pass (losses.photometric_loss); fused_pixel_terms=False evaluates them step by step like the reference.
    sky_mask ([H,W] / [1,H,W], 1 = sky) with opt.lambda_sky != 0 adds lambda_sky * sky.sky_opacity_loss(pkg["alpha"], sky_mask)
    (an extension: the package must come from render(return_alpha=True))."""
    lam_sky = _sky_weight(opt, sky_mask)
    if lam_sky != 0.0 and pkg.get("alpha") is None:
        raise RuntimeError('training_loss: the sky term needs pkg["alpha"]: render(..., return_alpha=True)')
    use_feat = stage == "fine" and hyper.feat_head
    if fused_pixel_terms:
        loss = fused_photometric_loss(pkg["render"], gt_image[:3], pkg["depth"] if opt.lambda_depth != 0 else None, gt_depth,
                                      pkg["feat"] if use_feat else None, gt_feat, lambda_dssim=opt.lambda_dssim,
                                      lambda_depth=opt.lambda_depth, lambda_feat=opt.lambda_feat if use_feat else 0.0)
        sky_term = _sky.sky_opacity_loss(pkg["alpha"], sky_mask, 1.0) if lam_sky != 0.0 else None
        return _with_regularisers(pc, loss, pkg, [pkg], sky_term, lam_sky, hyper, opt, stage)
    # the reference's own sequence, one term at a time
    image = pkg["render"].unsqueeze(0)
    gt = gt_image.unsqueeze(0)
    loss = l1_loss(image, gt[:, :3])
    if opt.lambda_depth != 0:
        loss = loss + compute_depth_l2(pkg["depth"].unsqueeze(0), gt_depth.unsqueeze(0)) * opt.lambda_depth
    if opt.lambda_dssim != 0:
        loss = loss + opt.lambda_dssim * (1.0 - fused_ssim(image, gt))
    if use_feat:
        loss = loss + l2_loss(pkg["feat"], gt_feat) * opt.lambda_feat
    want_dx, want_dshs, want_reg = _wanted_regularisers(hyper, opt, stage)
    if want_dx:
        loss = loss + torch.mean(torch.abs(pkg["dx"])) * opt.lambda_dx
    if want_dshs:
        loss = loss + _dshs_l1(pkg) * opt.lambda_dshs
    if want_reg:
        loss = loss + _plane_reg(pc, [pkg], hyper)
    if lam_sky != 0.0:
        loss = loss + _sky.sky_opacity_loss(pkg["alpha"], sky_mask, lam_sky)
    return loss


def _finish_step(pc: GaussianParams, pkgs, grad_hook, optimizer_step) -> None:
    """What follows backward (and the densification statistics) in both steps: the caller's hook on the gradients, the optimizer
    step -- `optimizer_step()` in place of `pc.optimizer.step()` where the caller brings one --, and the gradients cleared."""
    if grad_hook is not None:
        grad_hook(pc, pkgs)
    if optimizer_step is not None:
        optimizer_step()
    else:
        pc.optimizer.step()
    pc.optimizer.zero_grad(set_to_none=True)


def training_step(pc: GaussianParams, cam: Dict, gt_image, gt_depth, gt_feat, hyper, opt, bg, stage="fine",
                  pipe: Optional[SimpleNamespace] = None, grad_hook=None, densify_stats=False, optimizer_step=None, sky_mask=None,
                  pose=None, cam_index=None, sky_model=None):
    """One iteration of train.py for one view: render -> loss -> backward -> Adam step.  `grad_hook(pc, pkg)` runs
    between backward and the optimizer step (used by the data-parallel wrapper for the RCCL all-reduce).
    densify_stats=True also does the bookkeeping of train.py:489-493 (max_radii2D, xyz_gradient_accum, denom) for this
    single-view batch: inside the rasterizer's per-Gaussian backward when the RGB + feature pair runs as ONE two-image node
    (the default fine-stage configuration), else -- coarse stage, pipe.fused_pair=False, debug snapshots, P == 0 -- as one fused
    pass over the viewspace gradient afterwards (optim.densify_stats).  Data-parallel runs reduce the statistics first
    (dp.reduce_densification_stats) and must leave this off.  `optimizer_step()` replaces `pc.optimizer.step()` (data parallel:
    dp.OverlappedGradAllReducer.finish_and_step, which steps the early-reduced groups while the last collectives are in flight).
    sky_mask with opt.lambda_sky != 0 (extension): the render also returns its opacity image and the loss gains
    lambda_sky * sky.sky_opacity_loss; its gradient rides in the same rasterizer backward, fused densify statistics included.
    Without a mask, or with lambda_sky = 0, nothing new is launched.
    pose (extension): a pose.PoseRefiner with cam_index = this camera's row in it: the view is rendered at its refined pose and
    the refiner's optimizer steps and clears beside the model's.  Not under the data-parallel wrapper.  None: nothing new.
    sky_model (extension): a skymodel.SkyModel attached with pc.attach_sky_model: the loss sees render(sky_model=...)'s composite,
    the composite's gradient on the opacity image adds to the sky-mask term's inside the one rasterizer backward, and the model's
    gradients are stepped by pc.optimizer ("sky_model" group).  `bg` is then not used.  Refused with pose=.  None: nothing new."""
    pipe = _default_pipe(pipe)
    if sky_model is not None:
        _sky_refusals("training_step", sky_model, pose)
        _sky_attached("training_step", pc, sky_model)
    if pose is not None:
        from . import dp as _dp
        if _dp.active():
            raise RuntimeError("training_step(pose=...): pose refinement under the data-parallel wrapper (dp) is not served")
    acc = (pc.xyz_gradient_accum, pc.denom, pc.max_radii2D) if densify_stats else None
    want_sky = _sky_weight(opt, sky_mask) != 0.0
    pkg = render(cam, pc, pipe, bg, stage=stage, return_dx=True, render_feat=(stage == "fine" and hyper.feat_head),
                 densify_accum=acc, **({"return_alpha": True} if want_sky else {}),
                 **({"pose": pose, "cam_index": cam_index} if pose is not None else {}),
                 **({"sky_model": sky_model} if sky_model is not None else {}))
    loss = training_loss(pc, pkg, gt_image, gt_depth, gt_feat, hyper, opt, stage, **({"sky_mask": sky_mask} if want_sky else {}))
    loss.backward()
    if densify_stats and not pkg.get("densify_stats_fused", False):
        from .optim import densify_stats as _densify_stats
        vg = pkg["viewspace_points"].grad
        if vg is None:     # no gradient reached the screen-space points (nothing visible): the statistics do not move
            vg = torch.zeros_like(pkg["viewspace_points"])
        _densify_stats(pc.xyz_gradient_accum, pc.denom, pc.max_radii2D, vg, pkg["radii"])
    _finish_step(pc, pkg, grad_hook, optimizer_step)
    if pose is not None:
        pose.step()
    return loss.detach(), pkg


# ---- a batch of views per iteration (train.py:286, 327-437: opt.batch_size) ----------------------------------------------------------
def rig_batches(cameras, num_cams: int = 3):
    """Index lists, one per timestamp: consecutive cameras with one `time`, at most `num_cams` each (a rig delivers its cameras of a
    frame back to back, as evaluate_video's strips assume).  What a caller samples from to feed training_step_views batches that
    share one deformation pass; which batch comes when stays with the caller."""
    n = int(num_cams)
    if n < 1:
        raise RuntimeError(f"rig_batches: num_cams = {num_cams}")
    out = []
    for i, cam in enumerate(cameras):
        t = float(cam["time"])
        if out and len(out[-1]) < n and float(cameras[out[-1][0]]["time"]) == t:
            out[-1].append(i)
        else:
            out.append([i])
    return out


def _pose_views_refusals(where: str, V: int, pose, cam_indices, sky_model) -> None:
    """What render_views / training_step_views refuse about pose= and cam_indices=, by name."""
    if pose is None:
        if cam_indices is not None:
            raise RuntimeError(f"{where}(cam_indices=...) without pose=: the indices say which of a pose.PoseRefiner's cameras the "
                               "views are")
        return
    if sky_model is not None:
        _sky_refusals(where, sky_model, pose)
    from . import dp as _dp
    if _dp.active():
        raise RuntimeError(f"{where}(pose=...): pose refinement under the data-parallel wrapper (dp) is not served")
    if cam_indices is None:
        raise RuntimeError(f"{where}(pose=...): cam_indices says which of the refiner's cameras each view is")
    if len(cam_indices) != V:
        raise RuntimeError(f"{where}(pose=...): {len(cam_indices)} cam_indices for {V} views")


def _render_views(cams, pc, pipe, bg_color, stage, render_feat, return_dx, share_deformation, return_alpha=False, sky_model=None,
                  pose=None, cam_indices=None):
    """-> (result dicts, the skip word of each view's asynchronous forward or None)."""
    from . import raster_C
    V = len(cams)
    _pose_views_refusals("render_views", V, pose, cam_indices, sky_model)
    if sky_model is not None:      # as in render(): a zero background of the call's own, the opacity image, the composite per view
        bg_color = torch.zeros(3, dtype=torch.float32, device=pc.get_xyz.device)
        return_alpha = True
    from .glue import MAX_VIEWS, activations_and_colors_views
    if torch.is_grad_enabled() and any(torch.is_tensor(cam.get(k)) and cam[k].requires_grad
                                       for cam in cams for k in ("viewmatrix", "projmatrix", "campos")):
        raise RuntimeError("render_views: a camera requires a gradient; camera gradients (pose refinement) are served through "
                           "pose= / cam_indices= (a pose.PoseRefiner), or by render() / training_step(), one view per call")
    flags = [bool(render_feat)] * V if isinstance(render_feat, (bool, int)) else [bool(f) for f in render_feat]
    if len(flags) != V:
        raise RuntimeError(f"render_views: render_feat has {len(flags)} entries for {V} views")
    if "coarse" not in stage and "fine" not in stage:
        raise NotImplementedError
    dev = pc.get_xyz.device
    if not _glue_route(pc, pipe, stage) or getattr(pipe, "compute_cov3D_python", False):
        outs, words = [], []
        for v, (cam, f) in enumerate(zip(cams, flags)):     # the library route: nothing to share, the same results contract
            outs.append(render(cam, pc, pipe, bg_color, stage=stage, return_dx=return_dx, render_feat=f,
                               **({"return_alpha": True} if return_alpha else {}),
                               **({"pose": pose, "cam_index": cam_indices[v]} if pose is not None else {}),
                               **({"sky_model": sky_model} if sky_model is not None else {})))
            words.append(raster_C.async_skip_flag(dev) if dev.type == "cuda" else None)
        return outs, words
    if pose is not None:
        # the batch's cameras at their refined poses, one node: each view's rasterizer node and each timestamp's glue pass hand
        # their camera gradients back to it
        cams = pose.corrected_views(cams, cam_indices)
    groups: Dict[float, list] = {}
    for i, cam in enumerate(cams):
        groups.setdefault(float(cam["time"]) if share_deformation else i, []).append(i)
    chunks = [idx[k:k + MAX_VIEWS] for idx in groups.values() for k in range(0, len(idx), MAX_VIEWS)]
    hy = pc._deformation.deformation_net.args
    grad = torch.is_grad_enabled()
    outs, words = [None] * V, [None] * V
    for gi, idx in enumerate(chunks):
        # ONE evaluation of the field for the views of this timestamp; the plane regulariser is a term of the iteration, not of
        # a view: it rides on the first group's sampler node only
        means3D_final, scales, rotations, opacity, dx, dshs, feat, plane_reg = _deform_fused(
            pc, cams[idx[0]]["time"], stage, any(flags[i] for i in idx) or grad,
            gi == 0 and stage == "fine" and grad and hy.time_smoothness_weight != 0)
        want_l1 = dshs is not None and grad
        glue_out = activations_and_colors_views(pc.active_sh_degree, pc._features_dc, pc._features_rest, dshs, pc.get_xyz,
                                                torch.stack([cams[i]["campos"].reshape(3) for i in idx]), scales, rotations, opacity,
                                                with_dshs_l1=want_l1, **({"campos_grad": True} if pose is not None else {}))
        colors, scales_final, rotations_final, opacity_final = glue_out[:4]
        dshs_l1 = glue_out[4] if want_l1 else None
        for k, i in enumerate(idx):
            rasterizer = GaussianRasterizer(raster_settings=_raster_settings(cams[i], pc, pipe, bg_color))
            means2D = torch.empty_like(pc.get_xyz).requires_grad_(True)      # carries the viewspace gradient of THIS view (see render)
            want_feat = flags[i] and "fine" in stage
            # densify_accum is never handed over: a batch's statistics take the norm of the SUMMED viewspace gradient
            image, radii, depth, image2, alpha = _rasterize_view(
                rasterizer, means3D_final, means2D, opacity_final, scales_final, rotations_final, None, None, colors[k], want_feat, feat,
                getattr(pipe, "fused_pair", True), return_alpha)
            words[i] = raster_C.async_skip_flag(dev)
            outs[i] = _view_result(image, means2D, radii, depth, image2, alpha, want_feat, return_alpha, return_dx and "fine" in stage,
                                   dx, dshs, dshs_l1, plane_reg)
            if sky_model is not None:
                _sky_compose(outs[i], sky_model, cams[i])
    return outs, words


def render_views(cams, pc: GaussianParams, pipe: SimpleNamespace, bg_color: torch.Tensor, stage="fine", render_feat=False,
                 return_dx=True, share_deformation=True, return_alpha=False, sky_model=None, pose=None, cam_indices=None):
    """render() for a batch of views -> a list of result dicts with the keys render() returns, in the order of `cams`.
    The deformation field depends on (xyz, t) only, never on the camera.  On the fused route (stage "coarse", or a network on
    Deformation._fused_any with the fused glue: every head subset, no_dx, the geometry heads) the views are grouped by cam["time"]
    and each distinct timestamp gets ONE deform_heads evaluation and ONE glue pass for all its cameras
    (glue.activations_and_colors_views; more than 8 cameras of one timestamp are served in chunks of 8, each chunk with passes of
    its own); only the rasterizer runs per view
    (forward_pair where the view's feature image is wanted, the plain rasterizer otherwise).  The tensors of one timestamp --
    "dx", "dshs", "dshs_l1" -- are shared by its views' dicts; "plane_reg" (the HexPlane regulariser, under autograd in stage
    "fine") appears in the first timestamp's dicts only: it is a term of the iteration, not of a view.
    render_feat: a bool, or one bool per view.  share_deformation=False: one evaluation per view (A/B measurements, equivalence
    tests).  On the library route (grid_pe, no_grid, static_mlp, empty_voxel, pipe.fused_glue=False, convert_SHs_python=False,
    compute_cov3D_python) this is one render() per view: same contract, nothing shared.
    No densify_accum here: a batch's densification statistics take the norm of the summed viewspace gradient
    (optim.densify_stats_views), which a per-view update inside the rasterizer's backward cannot give.
    return_alpha: every dict carries "alpha", as render(return_alpha=True) gives it.
    sky_model: every view as render(sky_model=...) gives it ("render" the composite, "render_fg", "alpha"); bg_color is not used.
    pose (extension): a pose.PoseRefiner, with cam_indices = one row of it per view (no row twice): the batch's cameras are
    corrected once (pose.corrected_views, one launch each way), the grouping by cam["time"] is as without a refiner, each
    timestamp's glue pass also returns its views' camera-centre gradients and each view's rasterizer node its camera gradients as
    in render(pose=): a loss on the results back-propagates to rows cam_indices of pose.delta, per camera the bits that one
    render(pose=, cam_index=) per view accumulates.  On the library route each view's render() takes pose= / cam_index= itself.
    Cameras that the caller made require a gradient stay refused.  Refused by name: pose= with sky_model=, pose= under the
    data-parallel wrapper, cam_indices of another length than cams, cam_indices without pose.  None: nothing new is launched."""
    return _render_views(list(cams), pc, pipe, bg_color, stage, render_feat, return_dx, share_deformation, bool(return_alpha),
                         sky_model, pose, None if cam_indices is None else list(cam_indices))[0]


def _supervised_feat_views(V: int, hyper, stage: str, feat_views: str):
    if feat_views not in ("last", "all"):
        raise RuntimeError(f'feat_views must be "last" (the reference) or "all", got {feat_views!r}')
    use_feat = stage == "fine" and hyper.feat_head
    return [bool(use_feat and (feat_views == "all" or v == V - 1)) for v in range(V)]


def training_loss_views(pc: GaussianParams, pkgs, gt_images, gt_depths, gt_feats, hyper, opt, stage="fine", feat_views="last",
                        sky_masks=None):
    """train.py:389-425 for a batch of V views, the reference's semantics line for line, quirks included:
      - L1 and SSIM are means over all V*3*H*W elements of the concatenated images;
      - the depth term is the mean over the valid pixels of the WHOLE batch (one joint count, not a mean of per-view means);
      - lambda_dx * mean|dx|, lambda_dshs * mean|dshs| and lambda_feat * l2(feat, gt_feat) come from the LAST view's package only
        (the reference reads `render_pkg` after its loop);
      - the plane regulariser is applied once.
    feat_views="all" (an extension for rigs whose every camera has a feature map, NOT the reference's behaviour) supervises every
    view's feature image instead: the mean over V*3*H*W.  One fused node for the per-pixel terms (losses.photometric_loss_views).
    sky_masks (one per view) with opt.lambda_sky != 0 (extension) adds lambda_sky * the sky cross entropy as ONE mean over
    V*H*W: every view is supervised, each with weight 1/V (sky.sky_opacity_loss)."""
    from .losses import photometric_loss_views
    V = len(pkgs)
    lam_sky = _sky_weight(opt, sky_masks)
    if lam_sky != 0.0 and (len(sky_masks) != V or any(p.get("alpha") is None for p in pkgs)):
        raise RuntimeError(f'training_loss_views: the sky term needs {V} sky masks and "alpha" in every package '
                           "(render_views(..., return_alpha=True))")
    if V < 1 or len(gt_images) != V:
        raise RuntimeError(f"training_loss_views: {V} views, {len(gt_images)} ground-truth images")
    sup = _supervised_feat_views(V, hyper, stage, feat_views)
    H, W = pkgs[0]["render"].shape[-2:]
    for v, p in enumerate(pkgs):
        h, w = p["render"].shape[-2:]
        if (h, w) != (H, W):
            raise RuntimeError(f"training_loss_views: view {v} renders {h} x {w}, view 0 {H} x {W}: all views of a batch must "
                               "render one size")
    gt_feats = [None] * V if gt_feats is None else list(gt_feats)
    with_depth = opt.lambda_depth != 0
    loss = photometric_loss_views([p["render"] for p in pkgs], [g[:3] for g in gt_images],
                                  [p["depth"] for p in pkgs] if with_depth else None, list(gt_depths) if with_depth else None,
                                  [p["feat"] if s else None for p, s in zip(pkgs, sup)],
                                  [g if s else None for g, s in zip(gt_feats, sup)], lambda_dssim=opt.lambda_dssim,
                                  lambda_depth=opt.lambda_depth, lambda_feat=opt.lambda_feat if any(sup) else 0.0)
    sky_term = _sky.sky_opacity_loss([p["alpha"] for p in pkgs], list(sky_masks), 1.0) if lam_sky != 0.0 else None
    return _with_regularisers(pc, loss, pkgs[-1], pkgs, sky_term, lam_sky, hyper, opt, stage)


def training_step_views(pc: GaussianParams, cams, gt_images, gt_depths, gt_feats, hyper, opt, bg, stage="fine",
                        pipe: Optional[SimpleNamespace] = None, grad_hook=None, densify_stats=False, optimizer_step=None,
                        feat_views="last", share_deformation=True, sky_masks=None, sky_model=None, pose=None, cam_indices=None):
    """One iteration of train.py for a batch of V views (opt.batch_size = V, train.py:365-437, 489-493, 521-522): V renders -> one
    loss (training_loss_views: the reference's batch semantics) -> one backward -> ONE Adam step.  -> (loss, result dicts).
    Views that share a timestamp (a rig's cameras of one frame) share one deformation pass and one glue pass each way
    (render_views); views whose feature image gets no loss (all but the last under feat_views="last") do not rasterize one.
    densify_stats=True: the bookkeeping of train.py:387-388, 435-437, 489-493 in one pass (optim.densify_stats_views): the norm of
    the SUMMED viewspace gradient, any-visibility, the largest radius.  grad_hook(pc, pkgs) receives the list.
    share_deformation=False evaluates the field once per view (A/B measurements, equivalence tests).
    Under run_training_steps an overflow in any view of the batch leaves model and statistics untouched and the whole batch is
    issued again: the sticky word freezes every later forward of the batch, and the guarded launches read the last one's word.
    sky_masks (one per view) with opt.lambda_sky != 0: see training_loss_views; otherwise nothing new is launched.
    sky_model: as training_step's: every view's loss sees its composite; the model must be attached (pc.attach_sky_model).
    pose (extension): a pose.PoseRefiner with cam_indices = the views' rows in it (render_views): the views are rendered at their
    refined poses, the one backward reaches every view's correction, and the refiner's optimizer steps and clears once, after the
    model's.  Refused with sky_model=, under the data-parallel wrapper, and with cam_indices of another length.  After an
    overflowed asynchronous forward the step does what training_step(pose=) does: the camera gradients are exact zeros and the
    refiner's torch Adam takes its step on them; it is not rewound with the model's optimizer.  None: nothing new."""
    from . import raster_C
    from .optim import densify_stats_views as _densify_stats_views
    pipe = _default_pipe(pipe)
    cams = list(cams)
    V = len(cams)
    if V < 1 or len(gt_images) != V or (gt_depths is not None and len(gt_depths) != V) or (gt_feats is not None and len(gt_feats) != V):
        raise RuntimeError(f"training_step_views: {V} views need {V} ground-truth images, depths and feature maps (or None)")
    H, W = int(cams[0]["image_height"]), int(cams[0]["image_width"])
    for v, cam in enumerate(cams):
        if (int(cam["image_height"]), int(cam["image_width"])) != (H, W):
            raise RuntimeError(f"training_step_views: view {v} renders {int(cam['image_height'])} x {int(cam['image_width'])}, "
                               f"view 0 {H} x {W}: all views of a batch must render one size")
    sup = _supervised_feat_views(V, hyper, stage, feat_views)
    want_sky = _sky_weight(opt, sky_masks) != 0.0
    cam_indices = None if cam_indices is None else list(cam_indices)
    _pose_views_refusals("training_step_views", V, pose, cam_indices, sky_model)
    if sky_model is not None:
        _sky_attached("training_step_views", pc, sky_model)
    pkgs, words = _render_views(cams, pc, pipe, bg, stage, sup, True, share_deformation, want_sky, sky_model, pose, cam_indices)
    loss = training_loss_views(pc, pkgs, gt_images, gt_depths, gt_feats, hyper, opt, stage, feat_views,
                               **({"sky_masks": sky_masks} if want_sky else {}))
    loss.backward()
    words = [w for w in words if w is not None]
    if len(words) > 1 and raster_C.POLICY == "speculative" and not raster_C.REPLAY:
        # nothing else joins the views' verdicts in this mode: one overflowed view drops the batch's step and statistics
        raster_C.async_override_skip_flag(pc.get_xyz.device, torch.cat(words).amax(0, keepdim=True))
    if densify_stats:
        grads = [p["viewspace_points"].grad if p["viewspace_points"].grad is not None else torch.zeros_like(p["viewspace_points"])
                 for p in pkgs]
        if V > 8:      # S3G_DENSIFY_MAX_VIEWS; a larger batch would need its gradients summed first -- not a rig's batch
            raise RuntimeError("training_step_views(densify_stats=True) serves batches of up to 8 views")
        _densify_stats_views(pc.xyz_gradient_accum, pc.denom, pc.max_radii2D, grads, [p["radii"] for p in pkgs])
    _finish_step(pc, pkgs, grad_hook, optimizer_step)
    if pose is not None:
        pose.step()
    return loss.detach(), pkgs


_replay_loop = None      # the _ReplayLoop of the run_training_steps call in progress (surgery_barrier talks to it)


class _ReplayLoop:
    """Bookkeeping of run_training_steps: which iteration issued which forward / how many optimizer launches had gone out when it
    started, the (data-parallel: agreed) iteration to resume from, the rewind itself."""

    def __init__(self, optimizer, device, first):
        from . import raster_C
        self.rc, self.optimizer, self.device, self.first = raster_C, optimizer, device, first
        self.marks: Dict[int, tuple] = {}      # iteration -> (forwards issued, optimizer.step_calls) when it started
        self.rewinds = []

    def mark(self, i):
        self.marks[i] = (self.rc.async_issued(self.device), getattr(self.optimizer, "step_calls", None))
        horizon = i - 4 * self.rc._ASYNC_RING      # the host is never more than one status ring of forwards ahead of the device
        for k in [k for k in self.marks if k < horizon]:
            del self.marks[k]

    def iteration_of(self, seq) -> int:
        cands = [k for k, (s0, _) in self.marks.items() if s0 <= seq]
        # (a forward issued BEFORE this loop started cannot be replayed by it: run_training_steps drains those first, and should one
        #  slip through, the loop resumes from its own first iteration instead of failing on an empty max())
        return max(cands) if cands else (min(self.marks) if self.marks else self.first)

    def pending(self, block: bool) -> Optional[int]:
        """-> the iteration to resume from, or None.  Data parallel: the smallest over all ranks, agreed on the host (dp.agree_min),
        so that every replica rewinds to the same iteration at the same point of its loop -- every rank calls this at the same
        points: after each issue(i), at the tail, inside surgery_barrier()."""
        from . import dp
        seq = self.rc.async_replay_pending(self.device, block=block)
        j = None if seq is None else self.iteration_of(seq)
        return dp.agree_min(j) if dp.active() else j

    def rewind(self, j: int, at: int) -> int:
        calls = self.marks[j][1] if j in self.marks else None
        opt = self.optimizer
        if opt is not None and hasattr(opt, "rewind_to") and calls is not None:
            opt.rewind_to(calls)            # per parameter: only what the dropped launches advanced (optim.Adam journal)
        elif opt is not None and hasattr(opt, "rewind"):
            opt.rewind(at - j + 1)
        self.rc.async_acknowledge(self.device)
        self.rewinds.append((j, at))
        for k in [k for k in self.marks if k >= j]:
            del self.marks[k]
        return j


def surgery_barrier(device=None) -> None:
    """Call inside `issue(i)` BEFORE any host-side mutation of the model -- densify / prune / reset_opacity (new Parameters), an
    SH-degree step, a checkpoint -- when the loop is driven by run_training_steps.  Such a mutation is not covered by the device's
    freeze: applied inside a frozen window it would hit the frozen model and then be applied AGAIN by the replay.  This
    waits until every forward issued so far has reported (the reference's loop waits at `loss.item()` every iteration; this waits
    only where it mutates, every 100th) and, if one of them overflowed, raises raster_C.ReplayNeeded: run_training_steps rewinds and
    issue(i) runs again later, when the mutation sees the model the synchronous loop would have shown it.  Outside such a loop:
    no-op."""
    from . import raster_C
    loop = _replay_loop
    if loop is None or not raster_C.REPLAY:
        return
    j = loop.pending(block=True)
    if j is not None:
        raise raster_C.ReplayNeeded(iteration=j)


def run_training_steps(issue, first: int, last: int, optimizer=None, device=None, log: Optional[list] = None) -> Dict:
    """Drives iterations first..last (inclusive) through the host-asynchronous rasterizer WITHOUT ever dropping one.

    `issue(i)` enqueues iteration i -- learning-rate schedule, view choice (both functions of i), `training_step(...)` -- and returns
    nothing that the loop needs.  The loop never waits for the device.  Should a forward overflow its speculative arena, the device
    freezes the model from that iteration on (sticky word, raster_C.set_async_replay: the overflowed forward and every later one
    render nothing, the backward passes return zeros and skip the densification bookkeeping, the guarded Adam launches change
    nothing); the host finds out a few iterations later from the status ring, takes the optimizer's host-side step counts back,
    thaws the model and RE-ISSUES the iterations from the overflowed one with the capacity the true counts ask for.  The sequence of
    (view, optimizer step) pairs applied to the model is then exactly the one the reference's synchronous loop applies
    (train.py:291-522) -- VERDICT r4 item 8: round 4 dropped the overflowed iteration and went on.

    Contract of `issue(i)`: what it does to the model goes through the device (kernels the sticky word freezes); a
    HOST-side mutation -- densify / prune, opacity reset, oneupSHdegree, popping a view stack that is not a function of i -- must be
    preceded by `surgery_barrier()`, which waits for the outstanding reports and hands control back to this loop if a rewind is due.

    Data parallel (round 6): every replica runs this loop; after each iteration the ranks agree on the HOST (dp.agree_min over a gloo
    side group: no device wait) on the earliest iteration any of them has to resume from, and all rewind there together -- the
    reducers have kept every replica skipping the same steps in the meantime (dp.reduce_skip_flag).
    -> {"issued": total issue() calls, "rewinds": [(from_iteration, noticed_at_iteration), ...]}"""
    global _replay_loop
    from . import raster_C
    raster_C.async_status(device, block=True)      # forwards issued BEFORE this loop report under the policy they were issued with
    prev = raster_C.set_async_replay(True)
    loop = _ReplayLoop(optimizer, device, first)
    outer, _replay_loop = _replay_loop, loop
    issued = 0
    try:
        i = first
        while True:
            while i <= last:
                loop.mark(i)
                try:
                    issue(i)
                except raster_C.ReplayNeeded as rn:      # surgery_barrier() / a synchronous-fallback forward inside issue(i)
                    j = rn.iteration if rn.iteration is not None else loop.iteration_of(rn.seq)
                    i = loop.rewind(j, i)
                    continue
                issued += 1
                if log is not None:
                    log.append(i)
                j = loop.pending(block=False)
                i = loop.rewind(j, i) if j is not None else i + 1
            j = loop.pending(block=True)                 # the tail: every status row has landed
            if j is None:
                break
            i = loop.rewind(j, last)
    finally:
        raster_C.set_async_replay(prev)
        _replay_loop = outer
    return {"issued": issued, "rewinds": loop.rewinds}
