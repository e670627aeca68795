"""Deformation network on the MI355X with the module/parameter names of the reference's scene/deformation.py
(`deform_network` :179-235, `Deformation` :16-178) so checkpoints, `get_mlp_parameters` / `get_grid_parameters`
(name filter "grid") and the Adam groups of scene/gaussian_model.py:170-201 keep working.

The reference's default configuration (arguments/__init__.py:202-236) runs as two fused HIP operators (HexPlane sampler +
MFMA MLP), and so does its static one (arguments/static_nvs.py: no_dx=True -- the same kernels with the position head compiled
out).  Every other switch of scene/deformation.py:16-178 is honoured too -- no_dx / no_ds / no_dr / no_do / no_dshs /
feat_head, grid_pe (sin/cos embedding of the grid feature, :84-86), no_grid (:79-80), static_mlp and empty_voxel (the
per-point mask of :108-114, DenseGrid of scene/grid.py:15-42), apply_rotation (:140-141) -- on the same fused sampler with
the heads as PyTorch-ROCm library GEMMs (GPU only; nothing here runs on the CPU).
With any of no_ds / no_dr / no_do off (scale, rotation, opacity deformation) the plain-grid configuration stays on the fused route:
those heads run as a second fused operator beside the MLP (mlp_geom.geometry_heads, `_fused_geometry_ok`).  So does it with no_dshs on
or feat_head off (`_fused_heads_ok`): every on/off combination of the six heads runs fused; the library GEMMs serve grid_pe, no_grid,
static_mlp and empty_voxel.
Inference (no_grad renders without the feature image) takes ONE kernel, sampler (+) heads with no [P,128] array, for the default heads
(mlp.deform_infer) and for every other head set whose weights fit the CU's LDS beside the sampler's tiles (mlp.deform_infer_heads,
`_infer_heads_ok`: static, no_dshs, 4D-Gaussian-Splatting's default, ...); the sets that do not fit (e.g. all five heads) run the
sampler, the MLP kernel and the geometry-heads kernel one after the other, as training does.
"""
from __future__ import annotations

import torch
import torch.nn as nn

import torch.nn.functional as F

from .hexplane import HexPlaneField
import os

from .mlp import deform_infer, deform_infer_heads, deform_mlp, get_mlp_arithmetic, infer_heads_served
from .mlp_geom import geometry_heads

# S3G_FUSED_INFERENCE=0: inference renders go through the separate kernels (sampler, then MLP, then geometry heads) like training
# does -- both one-kernel routes (deform_infer, deform_infer_heads) are off
FUSED_INFERENCE = os.environ.get("S3G_FUSED_INFERENCE", "1") != "0"
# Arithmetic of the fused inference kernel's GEMM layers: "f32" = exact fp32 fma chains (v_mfma_f32_32x32x2_f32, bit-identical to the
# training kernels), "bf16x3" = the bf16 matrix pipe on exactly split operands (include/s3g_mlp.h::s3g_deform_infer_split)
# (round 6: the default follows the training kernels' default -- the split arithmetic; "f32" = the exact chain)
INFER_ARITHMETIC = os.environ.get("S3G_INFER_ARITHMETIC", "bf16x3")
# S3G_INFER_CACHE=0: every no_grad render evaluates the deformation field afresh (A/B, diagnostics).  Default: the heads' outputs of the
# last no_grad evaluation are kept and handed to the next render of the SAME Gaussians at the SAME timestamp with the SAME parameters
# -- the deformation depends on (xyz, t) only, not on the camera, and the evaluation loops of the reference visit the cameras of one
# timestamp back to back (utils/video_utils.py:116-349 iterates `viewpoint_cams` in dataset order: 3 Waymo cameras per frame)
INFER_CACHE = os.environ.get("S3G_INFER_CACHE", "1") != "0"
infer_cache_hits = 0      # renders served from the cache (tests, bench.py)
heads_evaluations = 0     # grad-enabled evaluations of deform_heads: one per training render, one per TIMESTAMP of a pipeline.render_views batch
_served_sets = {}         # (need_dx, need_dshs, need_ds, need_dr, need_do) -> mlp.infer_heads_served, asked once per set


def poc_fre(input_data, poc_buf):
    """scene/deformation.py:244-250."""
    emb = (input_data.unsqueeze(-1) * poc_buf).flatten(-2)
    return torch.cat([input_data, emb.sin(), emb.cos()], -1)


def batch_quaternion_multiply(q1, q2):
    """utils/graphics_utils.py:154-177 (product, then normalisation)."""
    w = q1[:, 0] * q2[:, 0] - q1[:, 1] * q2[:, 1] - q1[:, 2] * q2[:, 2] - q1[:, 3] * q2[:, 3]
    x = q1[:, 0] * q2[:, 1] + q1[:, 1] * q2[:, 0] + q1[:, 2] * q2[:, 3] - q1[:, 3] * q2[:, 2]
    y = q1[:, 0] * q2[:, 2] - q1[:, 1] * q2[:, 3] + q1[:, 2] * q2[:, 0] + q1[:, 3] * q2[:, 1]
    z = q1[:, 0] * q2[:, 3] + q1[:, 1] * q2[:, 2] - q1[:, 2] * q2[:, 1] + q1[:, 3] * q2[:, 0]
    q3 = torch.stack((w, x, y, z), dim=1)
    return q3 / torch.norm(q3, dim=1, keepdim=True)


class DenseGrid(nn.Module):
    """scene/grid.py:15-54: a [1,C,X,Y,Z] voxel grid sampled trilinearly (the `empty_voxel` mask)."""

    def __init__(self, channels, world_size):
        super().__init__()
        self.channels, self.world_size = channels, world_size
        self.grid = nn.Parameter(torch.ones([1, channels, *world_size]))

    def set_aabb(self, xyz_max, xyz_min):
        self.register_buffer('xyz_min', torch.tensor(xyz_min, dtype=torch.float32, device=self.grid.device))
        self.register_buffer('xyz_max', torch.tensor(xyz_max, dtype=torch.float32, device=self.grid.device))

    def forward(self, xyz):
        shape = xyz.shape[:-1]
        ind_norm = ((xyz.reshape(1, 1, 1, -1, 3) - self.xyz_min) / (self.xyz_max - self.xyz_min)).flip((-1,)) * 2 - 1
        out = F.grid_sample(self.grid, ind_norm, mode='bilinear', align_corners=True)
        return out.reshape(self.channels, -1).T.reshape(*shape, self.channels)


def _head(W, out):
    return nn.Sequential(nn.ReLU(), nn.Linear(W, W), nn.ReLU(), nn.Linear(W, out))


class Deformation(nn.Module):
    def __init__(self, D=8, W=256, input_ch=27, input_ch_time=9, grid_pe=0, skips=(), args=None):
        super().__init__()
        self.D, self.W, self.args, self.grid_pe = D, W, args, grid_pe
        self.input_ch, self.input_ch_time, self.skips = input_ch, input_ch_time, list(skips)
        self.no_grid = args.no_grid
        self.grid = HexPlaneField(args.bounds, args.kplanes_config, args.multires)
        if getattr(args, "empty_voxel", False):
            self.empty_voxel = DenseGrid(channels=1, world_size=[64, 64, 64])
        if getattr(args, "static_mlp", False):
            self.static_mlp = nn.Sequential(nn.ReLU(), nn.Linear(W, W), nn.ReLU(), nn.Linear(W, 1))
        self.ratio = 0
        grid_out_dim = self.grid.feat_dim * 3 if grid_pe != 0 else self.grid.feat_dim     # deformation.py:47-51
        layers = [nn.Linear(4 if self.no_grid else grid_out_dim, W)]
        for _ in range(D - 1):
            layers += [nn.ReLU(), nn.Linear(W, W)]
        self.feature_out = nn.Sequential(*layers)
        self.pos_deform = _head(W, 3)
        self.scales_deform = _head(W, 3)
        self.rotations_deform = _head(W, 4)
        self.opacity_deform = _head(W, 1)
        self.shs_deform = _head(W, 16 * 3)
        if args.feat_head:
            self.dino_head = nn.Sequential(nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, 64), nn.ReLU(), nn.Linear(64, 3))

    @property
    def get_aabb(self):
        return self.grid.get_aabb

    def set_aabb(self, xyz_max, xyz_min):
        self.grid.set_aabb(xyz_max, xyz_min)
        if getattr(self.args, "empty_voxel", False):
            self.empty_voxel.set_aabb(xyz_max, xyz_min)

    @property
    def get_empty_ratio(self):
        return self.ratio

    def query_time(self, rays_pts_emb, scales_emb, rotations_emb, time_feature, time_emb):
        """scene/deformation.py:78-94."""
        if self.no_grid:
            hidden = torch.cat([rays_pts_emb[:, :3], time_emb[:, :1]], -1)
        else:
            hidden = self.grid(rays_pts_emb[:, :3], time_emb[:, :1])
            if self.grid_pe > 1:
                hidden = poc_fre(hidden, self.grid_pe)
        return self.feature_out(hidden)

    def forward_static(self, rays_pts_emb):
        """scene/deformation.py:102-105 (needs static_mlp; like the reference, the field is sampled without a time)."""
        raise NotImplementedError("forward_static samples the 4-D field without a timestamp, which the reference's "
                                  "HexPlaneField cannot do either (scene/hexplane.py:151-164 concatenates timestamps)")

    def forward(self, rays_pts_emb, scales_emb=None, rotations_emb=None, opacity=None, shs_emb=None, time_feature=None,
                time_emb=None):
        if time_emb is None:
            return self.forward_static(rays_pts_emb[:, :3])
        return self.forward_dynamic(rays_pts_emb, scales_emb, rotations_emb, opacity, shs_emb, time_feature, time_emb)

    def _plain_network(self):
        """What every fused MLP kernel is built for: a plain grid (per-point mask 1), D == 1, W == 64, 128 features."""
        a = self.args
        plain = not (self.no_grid or self.grid_pe != 0 or getattr(a, "static_mlp", False) or getattr(a, "empty_voxel", False))
        return bool(plain and self.D == 1 and self.W == 64 and self.grid.feat_dim == 128)

    def _mlp_kernels_fit(self):
        """`_plain_network` with the dshs and feature heads on; no_dx either way."""
        a = self.args
        return bool(self._plain_network() and not a.no_dshs and a.feat_head)

    def _fused_ok(self):
        """The fused route serves the reference's default heads (dx + dshs + feat) and the static configuration (no_dx: dshs + feat)."""
        a = self.args
        return bool(self._mlp_kernels_fit() and a.no_ds and a.no_dr and a.no_do)

    def _fused_geometry_ok(self):
        """The fused route with the geometry heads beside it (mlp_geom.geometry_heads): at least one of the scale / rotation / opacity
        heads is on and everything else `_fused_ok` asks for holds.  Never true together with `_fused_ok`, which keeps its meaning: the
        configurations the MLP kernels serve on their own."""
        a = self.args
        return bool(self._mlp_kernels_fit() and not (a.no_ds and a.no_dr and a.no_do))

    def _fused_heads_ok(self):
        """The fused route WITHOUT the SH head (no_dshs) or without the feature head (feat_head off), the configurations the two older
        predicates refuse: any subset of dx / ds / dr / do beside them, as long as one of the six heads is on (no_dshs + feat_head off +
        the geometry heads on is 4D-Gaussian-Splatting's default).  Never true together with `_fused_ok` or `_fused_geometry_ok`, which
        keep their values."""
        a = self.args
        any_head = not (a.no_dx and a.no_ds and a.no_dr and a.no_do and a.no_dshs) or a.feat_head
        return bool(self._plain_network() and (a.no_dshs or not a.feat_head) and any_head)

    def _fused_any(self):
        """Any of the three: the configuration runs on the fused kernels."""
        return self._fused_ok() or self._fused_geometry_ok() or self._fused_heads_ok()

    def _fused_geometry_on(self):
        """A fused configuration with at least one of the scale / rotation / opacity heads on."""
        a = self.args
        return self._fused_any() and not (a.no_ds and a.no_dr and a.no_do)

    def _geometry_modules(self):
        """(scales_deform, rotations_deform, opacity_deform) with None for a head the configuration switches off."""
        a = self.args
        return (None if a.no_ds else self.scales_deform, None if a.no_dr else self.rotations_deform,
                None if a.no_do else self.opacity_deform)

    def _infer_heads_ok(self):
        """The one-kernel inference route for the head sets deform_infer does not serve (mlp.deform_infer_heads): a fused network whose
        set of dx / ds / dr / do / dshs the kernel holds in LDS.  The kernel is the exact fp32 chain.  Without the SH head that is what
        the separate kernels compute in every arithmetic mode; WITH it they follow mlp.set_mlp_arithmetic, so such a set takes the
        route only in the "f32" mode, where it changes no bit (in "bf16x3" the separate kernels stay: a render must not depend on the
        route)."""
        a = self.args
        if not self._fused_any():
            return False
        if not a.no_dshs and get_mlp_arithmetic() != "f32":
            return False
        heads = (not a.no_dx, not a.no_dshs, not a.no_ds, not a.no_dr, not a.no_do)
        served = _served_sets.get(heads)
        if served is None:
            served = _served_sets[heads] = infer_heads_served(*heads)
        return served

    def deform_heads(self, xyz, time, uniform_time=None, reg_weights=None, need_feat=True, with_geometry=False):
        """(dx [P,3], dshs [P,16,3], feat [P,3]) only -- the part of forward_dynamic that is not a pass-through in the
        reference's default configuration.  Lets a caller that fuses `shs + dshs` downstream (pipeline.render) skip
        materialising the [P,16,3] sum.  dx is None for a no_dx network (static scenes): the position head is never evaluated.
        with_geometry=True: one more entry, (ds [P,3], dr [P,4], do [P,1]) -- the outputs of the scale / rotation / opacity heads of a
        `_fused_geometry_ok` network, None for a head that is off -- or None for a network without them; it sits in front of the
        regulariser's entry.
        dshs is None for a no_dshs network and feat for one without a feature head (`_fused_heads_ok`); with no chain head at all
        only the geometry heads run."""
        global infer_cache_hits, heads_evaluations
        key = None
        # the other one-kernel route: every condition of the first one below, for the head sets mlp.deform_infer_heads serves
        heads_route = bool(FUSED_INFERENCE and not torch.is_grad_enabled() and not need_feat and reg_weights is None and xyz.is_cuda
                           and len(self.grid.resolutions) == 4 and self._infer_heads_ok())
        if INFER_CACHE and not torch.is_grad_enabled() and reg_weights is None and xyz.is_cuda:
            # identity + version of everything the outputs depend on (the rasterizer's geometry cache is keyed the same way,
            # raster_C._geom_key): optimizer steps, load_state_dict and in-place edits bump the version counters; writes through
            # `.data` or raw pointers do not -- call raster_C.invalidate_geometry_cache(), which also drops this entry, after those
            key = (tuple((t.data_ptr(), t._version, tuple(t.shape)) for t in (xyz, time)), bool(uniform_time), bool(need_feat),
                   INFER_ARITHMETIC if not need_feat else "f32", FUSED_INFERENCE, heads_route,
                   tuple((p.data_ptr(), p._version) for p in self.parameters()))
            hit = self.__dict__.get("_infer_cache")
            if hit is not None and hit[0] == key and all(t._version == v for t, v in hit[2]):   # (a consumer edited dx in place: miss)
                infer_cache_hits += 1
                return self._heads_result(hit[1], with_geometry)
        need_dx, need_dshs = not self.args.no_dx, not self.args.no_dshs
        dino_head = getattr(self, "dino_head", None)        # feat_head off: the module does not exist
        geometry = self._fused_geometry_on()
        if (FUSED_INFERENCE and need_dx and need_dshs and not geometry and not torch.is_grad_enabled() and not need_feat and reg_weights is None and xyz.is_cuda
                and len(self.grid.resolutions) == 4):
            # inference render without the feature image: sampler (+) heads in one kernel, no [P,128] round trip
            dx, dshs = deform_infer(self.grid, xyz[:, :3], time[:, :1], self.feature_out, self.pos_deform, self.shs_deform,
                                    dino_head, uniform_time, arithmetic=INFER_ARITHMETIC)
            out = (dx, dshs.reshape([xyz.shape[0], 16, 3]), None)
            if key is not None:
                self._keep_inference(key, out, xyz, time)
            return self._heads_result(out, with_geometry)
        if heads_route:
            # the same for a static / no_dshs / geometry-heads network: sampler (+) the heads present in one kernel, bit for bit what
            # the kernels below compute; the cached evaluation carries ds / dr / do behind the three, as theirs does
            dx, dshs, ds, dr, do = deform_infer_heads(self.grid, xyz[:, :3], time[:, :1], self.feature_out,
                                                      self.pos_deform if need_dx else None, self.shs_deform if need_dshs else None,
                                                      self._geometry_modules() if geometry else (None, None, None), uniform_time)
            out = (dx, None if dshs is None else dshs.reshape([xyz.shape[0], 16, 3]), None)
            if geometry:
                out = out + (ds, dr, do)
            if key is not None:
                self._keep_inference(key, out, xyz, time)
            return self._heads_result(out, with_geometry)
        if torch.is_grad_enabled():   # (neither one-kernel route above is taken under autograd)
            heads_evaluations += 1
        reg = None
        if reg_weights is not None:   # plane regulariser evaluated on the sampler's autograd node (hexplane_sample)
            feats, reg = self.grid(xyz[:, :3], time[:, :1], uniform_time, reg_weights)
        else:
            feats = self.grid(xyz[:, :3], time[:, :1], uniform_time)
        # need_feat=False (honoured only when no backward follows): skip the feature head, `feat` is then None
        # (so do the no_grad renders of a network whose head set neither one-kernel route serves -- e.g. all five heads, whose weights
        #  do not fit the LDS beside the sampler's tiles --, with the geometry heads as a third kernel on the same features)
        dx, dshs, feat = deform_mlp(feats, self.feature_out, self.pos_deform, self.shs_deform, dino_head, need_feat, need_dx, need_dshs)
        out = (dx, None if dshs is None else dshs.reshape([xyz.shape[0], 16, 3]), feat)
        if geometry:             # the cached evaluation carries ds / dr / do behind the three
            out = out + tuple(geometry_heads(feats, self.feature_out, *self._geometry_modules()))
        if key is not None:      # (no_grad, no regulariser: what an evaluation render with the feature image asks for)
            self._keep_inference(key, out, xyz, time)
        out = self._heads_result(out, with_geometry)
        return out + (reg,) if reg_weights is not None else out

    @staticmethod
    def _heads_result(out, with_geometry):
        """What deform_heads hands out of an evaluation `out` = (dx, dshs, feat) or (dx, dshs, feat, ds, dr, do)."""
        if not with_geometry:
            return out if len(out) == 3 else out[:3]
        return out[:3] + (tuple(out[3:]) if len(out) > 3 else None,)

    def _keep_inference(self, key, out, xyz, time) -> None:
        """ONE entry (the last timestamp): dx 14 MB + dshs 230 MB (+ feat 14 MB) at 1.2 M Gaussians.  xyz / time are kept alive so
        that their (pointer, version) identity in the key cannot be recycled by another tensor."""
        from . import raster_C
        self.__dict__["_infer_cache"] = (key, out, [(t, t._version) for t in out if t is not None], (xyz, time))
        raster_C._infer_cache_owners.add(self)

    def drop_inference_cache(self) -> None:
        self.__dict__.pop("_infer_cache", None)

    def inference_cache_entry(self):
        """The cached evaluation (or None), for a caller that evaluates one timestamp ahead of the one it renders
        (pipeline.render_flows) and puts this one back with install_inference_cache before the render that should hit it."""
        return self.__dict__.get("_infer_cache")

    def install_inference_cache(self, entry) -> None:
        """Makes an entry taken from inference_cache_entry() the cached evaluation again.  Its key still names the versions of
        everything the outputs depend on: an entry that has gone stale in the meantime simply misses."""
        if entry is not None:
            from . import raster_C
            self.__dict__["_infer_cache"] = entry
            raster_C._infer_cache_owners.add(self)

    def forward_dynamic(self, rays_pts_emb, scales_emb, rotations_emb, opacity_emb, shs_emb, time_feature, time_emb):
        a = self.args
        if self._fused_any() and rays_pts_emb.is_cuda:
            geometry = self._fused_geometry_on()
            # reference default configuration: HexPlane sampler -> one fused MFMA MLP kernel (include/s3g_mlp.h); a head that is
            # switched off is skipped in the kernels and comes back as None (no chain head at all: no launch)
            feats = self.grid(rays_pts_emb[:, :3], time_emb[:, :1])
            dx, dshs, feat = deform_mlp(feats, self.feature_out, self.pos_deform, self.shs_deform, getattr(self, "dino_head", None),
                                        need_dx=not a.no_dx, need_dshs=not a.no_dshs)
            if dshs is not None:
                dshs = dshs.reshape([shs_emb.shape[0], 16, 3])
            pts = rays_pts_emb[:, :3] if dx is None else rays_pts_emb[:, :3] + dx     # no_dx: scene/deformation.py:119-121
            scales, rotations, opacity = scales_emb[:, :3], rotations_emb[:, :4], opacity_emb[:, :1]
            if geometry:
                # scale / rotation / opacity heads: a second fused node on the same features (include/s3g_mlp_geom.h); the per-point
                # mask of scene/deformation.py:108-114 is 1 in every configuration admitted here
                ds, dr, do = geometry_heads(feats, self.feature_out, *self._geometry_modules())
                scales, rotations, opacity = self.apply_geometry(scales, rotations, opacity, ds, dr, do)
            return (pts, scales, rotations, opacity, shs_emb if dshs is None else shs_emb + dshs, dx, feat, dshs)
        # other switch combinations: fused HexPlane sampler + library GEMMs, scene/deformation.py:106-166 line by line
        hidden = self.query_time(rays_pts_emb, scales_emb, rotations_emb, time_feature, time_emb)
        if getattr(a, "static_mlp", False):
            mask = self.static_mlp(hidden)
        elif getattr(a, "empty_voxel", False):
            mask = self.empty_voxel(rays_pts_emb[:, :3])
        else:
            mask = torch.ones_like(opacity_emb[:, 0]).unsqueeze(-1)
        dx = dshs = feat = None
        pts = rays_pts_emb[:, :3]
        if not a.no_dx:
            dx = self.pos_deform(hidden)
            pts = rays_pts_emb[:, :3] * mask + dx
        scales = scales_emb[:, :3] if a.no_ds else scales_emb[:, :3] * mask + self.scales_deform(hidden)
        if a.no_dr:
            rotations = rotations_emb[:, :4]
        else:
            dr = self.rotations_deform(hidden)
            rotations = batch_quaternion_multiply(rotations_emb, dr) if getattr(a, "apply_rotation", False) else rotations_emb[:, :4] + dr
        opacity = opacity_emb[:, :1] if a.no_do else opacity_emb[:, :1] * mask + self.opacity_deform(hidden)
        shs = shs_emb
        if not a.no_dshs:
            dshs = self.shs_deform(hidden).reshape([shs_emb.shape[0], 16, 3])
            shs = shs_emb * mask.unsqueeze(-1) + dshs
        if a.feat_head:
            feat = self.dino_head(hidden)
        return pts, scales, rotations, opacity, shs, dx, feat, dshs

    def apply_geometry(self, scales, rotations, opacity, ds, dr, do):
        """scene/deformation.py:126-152 with mask = 1: scales + ds, rotations + dr (the normalised quaternion product with
        apply_rotation), opacity + do; a head that is off (None) leaves its input as it is."""
        if ds is not None:
            scales = scales + ds
        if dr is not None:
            rotations = batch_quaternion_multiply(rotations, dr) if getattr(self.args, "apply_rotation", False) else rotations + dr
        if do is not None:
            opacity = opacity + do
        return scales, rotations, opacity

    def get_mlp_parameters(self):
        return [p for n, p in self.named_parameters() if "grid" not in n]

    def get_grid_parameters(self):
        return [p for n, p in self.named_parameters() if "grid" in n]


class deform_network(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.timenet = nn.Sequential(nn.Linear(2 * args.timebase_pe + 1, args.timenet_width), nn.ReLU(),
                                     nn.Linear(args.timenet_width, args.timenet_output))  # unused by the reference too
        self.deformation_net = Deformation(W=args.net_width, D=args.defor_depth, input_ch=3 + 3 * args.posebase_pe * 2,
                                           grid_pe=args.grid_pe, input_ch_time=args.timenet_output, args=args)
        for name, n in (("time_poc", args.timebase_pe), ("pos_poc", args.posebase_pe),
                        ("rotation_scaling_poc", args.scale_rotation_pe), ("opacity_poc", args.opacity_pe)):
            self.register_buffer(name, torch.FloatTensor([2 ** i for i in range(n)]))
        for m in self.modules():  # initialize_weights (deformation.py:237-243): xavier on weights, default biases
            if isinstance(m, nn.Linear):
                nn.init.xavier_uniform_(m.weight, gain=1)

    @property
    def get_aabb(self):
        return self.deformation_net.get_aabb

    @property
    def get_empty_ratio(self):
        return self.deformation_net.get_empty_ratio

    def forward(self, point, scales=None, rotations=None, opacity=None, shs=None, times_sel=None):
        return self.forward_dynamic(point, scales, rotations, opacity, shs, times_sel)

    def forward_dynamic(self, point, scales=None, rotations=None, opacity=None, shs=None, times_sel=None):
        # The reference builds sin/cos embeddings of point/scales/rotations here (poc_fre, deformation.py:218-220) and
        # then reads only their first 3/4 columns (= the raw inputs): the embeddings are dead code and are skipped.
        return self.deformation_net(point, scales, rotations, opacity, shs, None, times_sel)

    def get_mlp_parameters(self):
        return self.deformation_net.get_mlp_parameters() + list(self.timenet.parameters())

    def get_grid_parameters(self):
        return self.deformation_net.get_grid_parameters()
