"""Adaptive density control on the MI355X library (include/s3g_density.h): the reference's `GaussianModel.densify`, `prune` and
`reset_opacity` (scene/gaussian_model.py:350-353, 412-522, 661-678) and the schedule that drives them (train.py:494-516).

One event is classify -> scan -> ONE host read (three counts, 12 bytes, to size the outputs) -> apply; the reference spends ~40
boolean-index / cat launches on it, each boolean index with a hidden `nonzero` synchronisation.  The host side is the reference's
optimizer surgery: fresh nn.Parameters into the single-parameter groups, the state dict re-keyed, `step` untouched, the
multi-parameter `deformation` / `grid` groups left alone.  Output row order (include/s3g_density.h, "ORDER CONTRACT"):
    [kept originals | clones | split children copy 1 | copy 2]
GPU only: CPU tensors are refused (no fallback on the product path)."""
from __future__ import annotations

import ctypes as C
from types import SimpleNamespace
from typing import Dict, Optional

import torch
import torch.nn as nn

from . import _lib

KEEP, CLONE, SPLIT, DROP = 0, 1, 2, 3
BLOCK = 256
MAX_TENSORS = 16

# optimizer group name -> attribute of the model (scene/gaussian_model.py:436-441, 482-487)
PER_GAUSSIAN = (("xyz", "_xyz"), ("f_dc", "_features_dc"), ("f_rest", "_features_rest"), ("opacity", "_opacity"),
                ("scaling", "_scaling"), ("rotation", "_rotation"))


class _Tensor(C.Structure):
    """struct s3g_density_tensor (include/s3g_density.h)."""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("src_exp_avg", C.c_void_p), ("dst_exp_avg", C.c_void_p),
                ("src_exp_avg_sq", C.c_void_p), ("dst_exp_avg_sq", C.c_void_p), ("width", C.c_int), ("children_rewritten", C.c_int)]


class _Plan(C.Structure):
    """struct s3g_density_plan (include/s3g_density.h)."""
    _fields_ = [("P", C.c_int), ("n_clone", C.c_int), ("n_split", C.c_int), ("n_drop", C.c_int), ("cls", C.c_void_p),
                ("block_offsets", C.c_void_p), ("table_src", C.c_void_p), ("table_dst", C.c_void_p), ("xyz", C.c_void_p),
                ("scaling", C.c_void_p), ("rotation", C.c_void_p), ("xyz_dst", C.c_void_p), ("scaling_dst", C.c_void_p),
                ("noise", C.c_void_p), ("noise_rows", C.c_size_t), ("seed", C.c_uint64), ("noise_out", C.c_void_p)]


_L = None


def _lib_bound():
    global _L
    if _L is None:
        L = _lib.lib()
        vp, f, i = C.c_void_p, C.c_float, C.c_int
        L.s3g_density_count_words.restype = C.c_size_t
        L.s3g_density_count_words.argtypes = [i]
        L.s3g_density_classify_densify.restype = i
        L.s3g_density_classify_densify.argtypes = [i, vp, vp, vp, f, f, vp, vp, vp]
        L.s3g_density_classify_prune.restype = i
        L.s3g_density_classify_prune.argtypes = [i, vp, vp, vp, f, f, f, vp, vp, vp]
        L.s3g_density_scan.restype = i
        L.s3g_density_scan.argtypes = [i, vp, vp, vp]
        L.s3g_density_apply.restype = i
        L.s3g_density_apply.argtypes = [C.POINTER(_Plan), i, C.POINTER(_Tensor), vp]
        L.s3g_density_reset_opacity.restype = i
        L.s3g_density_reset_opacity.argtypes = [i, vp, vp, vp, vp, vp]
        _L = L
    return _L


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None or t.numel() == 0 else t.data_ptr()


def _require_gpu(pc, what: str) -> torch.device:
    for _, attr in PER_GAUSSIAN:
        t = getattr(pc, attr)
        if not t.is_cuda:
            raise RuntimeError(f"s3gaussian_amd.density.{what}: the model must live on the GPU (no CPU fallback); {attr} is on {t.device}")
        if t.dtype != torch.float32:
            raise RuntimeError(f"s3gaussian_amd.density.{what}: {attr} must be float32")
    return pc._xyz.device


def _dense(t: torch.Tensor) -> torch.Tensor:
    t = t.detach()
    return t if t.is_contiguous() else t.contiguous()


def _groups(pc) -> Dict[str, dict]:
    """name -> single-parameter optimizer group of a per-Gaussian tensor (multi-parameter groups are skipped like the reference's
    `if len(group["params"]) > 1: continue`)."""
    opt = getattr(pc, "optimizer", None)
    out = {}
    if opt is not None:
        names = dict(PER_GAUSSIAN)
        for g in opt.param_groups:
            if len(g["params"]) == 1 and g.get("name") in names:
                out[g["name"]] = g
    return out


def _classify_and_count(L, dev, P, launch):
    """classify (through `launch(cls, counts, stream)`) + scan + the event's one host read -> (cls, offsets, [clone, split, drop])."""
    words = int(L.s3g_density_count_words(P))
    cls = torch.empty(max(P, 1), dtype=torch.uint8, device=dev)
    counts = torch.empty(words, dtype=torch.int32, device=dev)
    totals = torch.empty(3, dtype=torch.int32, device=dev)
    stream = _lib.stream_ptr()
    _lib.check(launch(cls, counts, stream))
    _lib.check(L.s3g_density_scan(P, counts.data_ptr(), totals.data_ptr(), stream))
    return cls, counts, [int(v) for v in totals.tolist()]


def _apply(pc, L, dev, cls, offsets, n_clone, n_split, n_drop, extra, noise=None, seed=0, noise_out=None):
    """The apply launch + the reference's optimizer surgery.  `extra`: {attribute: tensor} of per-Gaussian float tensors without
    moments that are gathered too (prune: the accumulators)."""
    P = pc._xyz.shape[0]
    P_out = P + n_clone + n_split - n_drop
    groups = _groups(pc)
    opt = getattr(pc, "optimizer", None)
    recs, keep, todo = [], [], []
    new, srcs = {}, {}
    for name, attr in PER_GAUSSIAN:
        g = groups.get(name)
        old = g["params"][0] if g is not None else getattr(pc, attr)
        st = opt.state.get(old, None) if (opt is not None and g is not None) else None
        has_m = bool(st) and "exp_avg" in st and "exp_avg_sq" in st
        src = _dense(old)
        dst = torch.empty((P_out,) + tuple(old.shape[1:]), dtype=torch.float32, device=dev)
        width = int(src.numel() // max(P, 1))
        sm = sv = dm = dv = None
        if has_m:
            sm, sv = _dense(st["exp_avg"]), _dense(st["exp_avg_sq"])
            if sm.shape != old.shape or sv.shape != old.shape or sm.dtype != torch.float32 or sv.dtype != torch.float32:
                raise RuntimeError(f"s3gaussian_amd.density: the Adam moments of {attr} do not match the parameter")
            dm, dv = torch.empty_like(dst), torch.empty_like(dst)
        keep += [sm, sv]                       # (possibly contiguous copies: they must outlive the launch call)
        srcs[name] = src
        recs.append(_Tensor(_ptr(src), _ptr(dst), _ptr(sm), _ptr(dm), _ptr(sv), _ptr(dv), width, 1 if name in ("xyz", "scaling") else 0))
        new[name] = dst
        todo.append((name, attr, g, old, st, has_m, dst, dm, dv))
    extra_new = {}
    for attr, t in extra.items():
        src = _dense(t)
        dst = torch.empty((P_out,) + tuple(t.shape[1:]), dtype=torch.float32, device=dev)
        keep.append(src)
        recs.append(_Tensor(_ptr(src), _ptr(dst), None, None, None, None, int(src.numel() // max(P, 1)), 0))
        extra_new[attr] = dst
    table = getattr(pc, "_deformation_table", None)
    table_src = table_dst = None
    if isinstance(table, torch.Tensor) and table.shape[:1] == (P,):
        table_src = _dense(table)
        table_src = table_src.view(torch.uint8) if table_src.dtype == torch.bool else table_src.to(torch.uint8)
        table_dst = torch.empty(P_out, dtype=torch.uint8, device=dev)
    if P_out > 0 and P > 0:
        plan = _Plan(P, n_clone, n_split, n_drop, cls.data_ptr(), offsets.data_ptr(), _ptr(table_src), _ptr(table_dst),
                     _ptr(srcs["xyz"]), _ptr(srcs["scaling"]), _ptr(srcs["rotation"]), _ptr(new["xyz"]), _ptr(new["scaling"]),
                     _ptr(noise), int(noise.shape[0]) if noise is not None else 0, int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(noise_out))
        assert len(recs) <= MAX_TENSORS
        arr = (_Tensor * len(recs))(*recs)
        _lib.check(L.s3g_density_apply(C.byref(plan), len(recs), arr, _lib.stream_ptr()))
    # ---- host surgery (scene/gaussian_model.py:412-494): fresh Parameters, state re-keyed, `step` untouched ----
    for name, attr, g, old, st, has_m, dst, dm, dv in todo:
        fresh = nn.Parameter(dst.requires_grad_(True))
        if g is not None:
            if st is not None:
                if has_m:
                    st["exp_avg"], st["exp_avg_sq"] = dm, dv
                del opt.state[old]
                if len(st):                    # a parameter with no state yet stays without one
                    opt.state[fresh] = st
            g["params"][0] = fresh
        old.grad = None                        # a pending gradient has the old length: dropped
        setattr(pc, attr, fresh)
    for attr, t in extra_new.items():
        setattr(pc, attr, t)
    if table_dst is not None:
        pc._deformation_table = table_dst.view(torch.bool) if table.dtype == torch.bool else table_dst.to(table.dtype)
    _invalidate(pc)
    return P_out


def _invalidate(pc) -> None:
    """What holds per-Gaussian indices or sizes of the old model: the sampler's cached spatial orders and the rasterizer's geometry
    cache (as GaussianParams.reorder_spatially does)."""
    net = getattr(getattr(pc, "_deformation", None), "deformation_net", None)
    grid = getattr(net, "grid", None)
    if grid is not None and hasattr(grid, "_order_cache"):
        grid._order_cache.clear()
    from . import raster_C
    raster_C.invalidate_geometry_cache()


def _barrier() -> None:
    from . import pipeline
    pipeline.surgery_barrier()


def _classify_densify(pc, L, dev, max_grad, extent, percent_dense):
    P = pc._xyz.shape[0]
    accum, denom = getattr(pc, "xyz_gradient_accum", None), getattr(pc, "denom", None)
    if accum is None or denom is None or accum.numel() != P or denom.numel() != P:
        raise RuntimeError("s3gaussian_amd.density.densify: xyz_gradient_accum / denom missing or of another length (training_setup first)")
    for t in (accum, denom):
        if not (t.is_cuda and t.dtype == torch.float32):
            raise RuntimeError("s3gaussian_amd.density.densify: the accumulators must be float32 tensors on the GPU")
    scaling, a, d = _dense(pc._scaling), _dense(accum), _dense(denom)
    return _classify_and_count(L, dev, P, lambda c, k, s: L.s3g_density_classify_densify(
        P, _ptr(a), _ptr(d), _ptr(scaling), float(max_grad), float(percent_dense * extent), _ptr(c), k.data_ptr(), s))


def _classify_prune(pc, L, dev, min_opacity, extent, max_screen_size):
    P = pc._xyz.shape[0]
    screen = float(max_screen_size) if max_screen_size else 0.0       # `if max_screen_size:` -- None and 0 switch the size tests off
    radii = getattr(pc, "max_radii2D", None)
    if screen > 0.0 and not (isinstance(radii, torch.Tensor) and radii.is_cuda and radii.dtype == torch.float32 and radii.numel() == P):
        raise RuntimeError("s3gaussian_amd.density.prune: max_radii2D must be a float32 GPU tensor with one element per Gaussian")
    o, s = _dense(pc._opacity), _dense(pc._scaling)
    r = _dense(radii) if screen > 0.0 else None
    return _classify_and_count(L, dev, P, lambda c, k, st: L.s3g_density_classify_prune(
        P, _ptr(o), _ptr(s), _ptr(r), float(min_opacity), screen, float(0.1 * extent), _ptr(c), k.data_ptr(), st))


@torch.no_grad()
def classify(pc, mode: str, extent, max_grad=None, percent_dense=None, min_opacity=None, max_screen_size=None):
    """The decisions alone, nothing mutated: mode "densify" (max_grad, percent_dense) or "prune" (min_opacity, max_screen_size).
    -> (class byte per Gaussian: KEEP / CLONE / SPLIT / DROP, {"clone", "split", "drop"})."""
    if mode not in ("densify", "prune"):
        raise ValueError(f"density.classify: mode {mode!r}")
    dev = _require_gpu(pc, "classify")
    L = _lib_bound()
    with _lib.on_device(dev):
        if mode == "densify":
            pd = getattr(pc, "percent_dense", 0.01) if percent_dense is None else percent_dense
            cls, _, tot = _classify_densify(pc, L, dev, max_grad, extent, pd)
        else:
            cls, _, tot = _classify_prune(pc, L, dev, min_opacity, extent, max_screen_size)
    return cls[:pc._xyz.shape[0]], {"clone": tot[0], "split": tot[1], "drop": tot[2]}


@torch.no_grad()
def densify(pc, max_grad, extent, percent_dense=None, noise=None, seed=None, return_noise=False):
    """GaussianModel.densify (scene/gaussian_model.py:673-678): clone the small Gaussians and split the large ones whose mean
    viewspace gradient reaches `max_grad`.  noise: optional [>= 2 * n_split, 3] standard normal deviates (child k of the j-th split
    row uses row k * n_split + j, the reference's `.repeat(N, 1)` tiling); otherwise Philox keyed on (seed, row), `seed=None` drawing
    the seed from torch's default CPU generator (torch.manual_seed makes a run repeatable and data-parallel replicas identical).
    -> {"clone", "split", "P"} (+ "noise": the deviates used, [2 * n_split, 3], with return_noise)."""
    _barrier()
    dev = _require_gpu(pc, "densify")
    L = _lib_bound()
    if percent_dense is None:
        percent_dense = getattr(pc, "percent_dense", 0.01)
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if noise is None else 0
    P = pc._xyz.shape[0]
    with _lib.on_device(dev):
        cls, offsets, (n_clone, n_split, _) = _classify_densify(pc, L, dev, max_grad, extent, percent_dense)
        out = {"clone": n_clone, "split": n_split, "P": P + n_clone + n_split}
        if noise is not None and n_split > 0:
            if not (isinstance(noise, torch.Tensor) and noise.is_cuda and noise.dtype == torch.float32 and noise.dim() == 2
                    and noise.shape[1] == 3 and noise.is_contiguous()):
                raise RuntimeError("s3gaussian_amd.density.densify: noise must be a contiguous float32 [n, 3] tensor on the GPU")
            if noise.shape[0] < 2 * n_split:
                raise RuntimeError(f"s3gaussian_amd.density.densify: noise has {noise.shape[0]} rows, {n_split} split rows need {2 * n_split}")
        noise_out = torch.empty((2 * n_split, 3), dtype=torch.float32, device=dev) if return_noise else None
        if n_clone + n_split > 0:
            _apply(pc, L, dev, cls, offsets, n_clone, n_split, 0, {}, noise=noise if n_split > 0 else None, seed=seed, noise_out=noise_out)
            P_new = pc._xyz.shape[0]
            pc.xyz_gradient_accum = torch.zeros((P_new, 1), device=dev)       # densification_postfix, :491-494
            pc.denom = torch.zeros((P_new, 1), device=dev)
            pc.max_radii2D = torch.zeros(P_new, device=dev)
        else:
            # nothing selected: no new tensors.  The reference still runs densification_postfix with empty extensions, which zeroes
            # the statistics: done in place
            pc.xyz_gradient_accum.zero_()
            pc.denom.zero_()
            if isinstance(getattr(pc, "max_radii2D", None), torch.Tensor):
                pc.max_radii2D.zero_()
    if return_noise:
        out["noise"] = noise_out
    return out


@torch.no_grad()
def prune(pc, min_opacity, extent, max_screen_size):
    """GaussianModel.prune (scene/gaussian_model.py:661-670).  -> {"drop", "P"}."""
    _barrier()
    dev = _require_gpu(pc, "prune")
    L = _lib_bound()
    P = pc._xyz.shape[0]
    with _lib.on_device(dev):
        cls, offsets, (_, _, n_drop) = _classify_prune(pc, L, dev, min_opacity, extent, max_screen_size)
        if n_drop > 0:
            extra = {}
            for attr in ("xyz_gradient_accum", "denom", "max_radii2D"):       # gathered, not zeroed (:442-446)
                t = getattr(pc, attr, None)
                if isinstance(t, torch.Tensor) and t.shape[:1] == (P,) and t.is_cuda and t.dtype == torch.float32:
                    extra[attr] = t
            _apply(pc, L, dev, cls, offsets, 0, 0, n_drop, extra)
    return {"drop": n_drop, "P": P - n_drop}


@torch.no_grad()
def reset_opacity(pc):
    """GaussianModel.reset_opacity (scene/gaussian_model.py:350-353, 397-410): opacity = inverse_sigmoid(min(sigmoid(o), 0.01)) as a
    fresh Parameter, both Adam moments zero, `step` untouched; one launch."""
    _barrier()
    dev = _require_gpu(pc, "reset_opacity")
    L = _lib_bound()
    g = _groups(pc).get("opacity")
    opt = getattr(pc, "optimizer", None)
    old = g["params"][0] if g is not None else pc._opacity
    st = opt.state.get(old, None) if g is not None else None
    has_m = bool(st) and "exp_avg" in st and "exp_avg_sq" in st
    P = old.shape[0]
    src = _dense(old)
    dst = torch.empty_like(src)
    m = v = None
    if has_m:
        for name in ("exp_avg", "exp_avg_sq"):
            if not st[name].is_contiguous():
                st[name] = st[name].contiguous()
        m, v = st["exp_avg"], st["exp_avg_sq"]
    with _lib.on_device(dev):
        _lib.check(L.s3g_density_reset_opacity(P, _ptr(src), _ptr(dst), _ptr(m), _ptr(v), _lib.stream_ptr()))
    if has_m:
        torch.autograd.graph.increment_version([m, v])      # written through raw pointers
    fresh = nn.Parameter(dst.requires_grad_(True))
    if g is not None:
        if st is not None:
            del opt.state[old]
            if len(st):
                opt.state[fresh] = st
        g["params"][0] = fresh
    old.grad = None
    pc._opacity = fresh
    from . import raster_C
    raster_C.invalidate_geometry_cache()
    return fresh


def default_density_opt(**over) -> SimpleNamespace:
    """The OptimizationParams that density control reads (arguments/__init__.py:124-172)."""
    o = dict(percent_dense=0.01, densification_interval=100, opacity_reset_interval=3000, pruning_interval=100, pruning_from_iter=500,
             densify_from_iter=500, densify_until_iter=25_000, densify_grad_threshold_coarse=0.0002,
             densify_grad_threshold_fine_init=0.0002, densify_grad_threshold_after=0.0002, opacity_threshold_coarse=0.005,
             opacity_threshold_fine_init=0.005, opacity_threshold_fine_after=0.005)
    o.update(over)
    return SimpleNamespace(**o)


MAX_POINTS_FOR_DENSIFY = 2_000_000      # train.py:501


def density_control(pc, iteration: int, opt, stage: str, cameras_extent: float) -> Dict:
    """The schedule of train.py:494-516 for one iteration (call it between backward and the optimizer step's successor exactly where
    the reference does: after the iteration's statistics -- training_step(densify_stats=True) -- have been accumulated).  Calls
    `pc.densify / pc.prune / pc.reset_opacity` with the reference's arguments.
    -> {"densify": result or None, "prune": result or None, "reset": bool, "densify_threshold", "opacity_threshold", "size_threshold"}"""
    out = {"densify": None, "prune": None, "reset": False, "densify_threshold": None, "opacity_threshold": None, "size_threshold": None}
    if not iteration < opt.densify_until_iter:
        return out
    if stage == "coarse":
        opacity_threshold = opt.opacity_threshold_coarse
        densify_threshold = opt.densify_grad_threshold_coarse
    else:
        opacity_threshold = opt.opacity_threshold_fine_init - iteration * (
            opt.opacity_threshold_fine_init - opt.opacity_threshold_fine_after) / opt.densify_until_iter
        densify_threshold = opt.densify_grad_threshold_fine_init - iteration * (
            opt.densify_grad_threshold_fine_init - opt.densify_grad_threshold_after) / opt.densify_until_iter
    size_threshold = 20 if iteration > opt.opacity_reset_interval else None
    out.update(densify_threshold=densify_threshold, opacity_threshold=opacity_threshold, size_threshold=size_threshold)
    if (iteration > opt.densify_from_iter and iteration % opt.densification_interval == 0
            and pc.get_xyz.shape[0] < MAX_POINTS_FOR_DENSIFY):
        r = pc.densify(densify_threshold, opacity_threshold, cameras_extent, size_threshold, 5, 5, None, iteration, stage)
        out["densify"] = r if r is not None else True
    if iteration > opt.pruning_from_iter and iteration % opt.pruning_interval == 0:
        r = pc.prune(densify_threshold, opacity_threshold, cameras_extent, size_threshold)
        out["prune"] = r if r is not None else True
    if iteration % opt.opacity_reset_interval == 0:
        pc.reset_opacity()
        out["reset"] = True
    return out
