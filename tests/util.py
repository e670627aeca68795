"""Shared scene builders / comparison helpers for the tests."""
from __future__ import annotations

import contextlib
import math

import numpy as np
import torch

from s3gaussian_amd import synth


@contextlib.contextmanager
def library_route(pc_or_net):
    """with library_route(pc): the model's Deformation module (or the module itself) is off the fused route, on the library-GEMM branch
    of forward_dynamic, whatever family of head switches put it on the fused one.  `_fused_any` is what pipeline.py and
    forward_dynamic ask, and `_fused_geometry_on` / `_infer_heads_ok` ask it too: shadowing that one method on the instance is enough."""
    net = pc_or_net._deformation.deformation_net if hasattr(pc_or_net, "_deformation") else pc_or_net
    assert net._fused_any()
    net._fused_any = lambda: False
    try:
        assert not net._fused_geometry_on() and not net._infer_heads_ok()
        yield net
    finally:
        del net._fused_any          # the instance attribute shadows the method


def tiny_scene(P=300, W=48, H=40, seed=0, scale=0.15, sigma=0.4, spread=2.2, bg=(0.2, 0.5, 0.7), zmin=3.0, zmax=6.0):
    """Small pinhole scene; camera at the origin looking along +z (OpenCV).  Returns CPU float32 tensors."""
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(P, 3, generator=g) * 2 - 1
    xyz[:, 2] = zmin + (zmax - zmin) * torch.rand(P, generator=g)
    xyz[:, :2] *= spread
    scales = torch.exp(math.log(scale) + sigma * torch.randn(P, 3, generator=g))
    q = torch.randn(P, 4, generator=g)
    q = q / q.norm(dim=1, keepdim=True)
    op = torch.sigmoid(1.5 * torch.randn(P, 1, generator=g))
    shs = torch.cat([torch.randn(P, 1, 3, generator=g), 0.3 * torch.randn(P, 15, 3, generator=g)], 1)
    col = torch.rand(P, 3, generator=g)
    fov = math.radians(60)
    cam = synth.make_camera(np.eye(3), np.zeros(3), fov, 2 * math.atan(math.tan(fov / 2) * H / W), W, H)
    return dict(means3D=xyz.contiguous(), scales=scales, rotations=q, opacities=op, shs=shs.contiguous(),
                colors_precomp=col, cam=cam, bg=torch.tensor(bg, dtype=torch.float32))


def cam_kwargs(s):
    cam = s["cam"]
    return dict(bg=s["bg"], viewmatrix=cam["viewmatrix"], projmatrix=cam["projmatrix"], campos=cam["campos"],
                tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], image_height=cam["image_height"],
                image_width=cam["image_width"])


def to_np(d):
    return {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else v) for k, v in d.items()}


def oracle_forward(oracle, s, mode="precomp", sh_degree=3, **over):
    kw = to_np(cam_kwargs(s))
    args = dict(means3D=s["means3D"].numpy(), opacities=s["opacities"].numpy(), scales=s["scales"].numpy(),
                rotations=s["rotations"].numpy())
    if mode == "precomp":
        args.update(colors_precomp=s["colors_precomp"].numpy(), sh_degree=0)
    else:
        args.update(shs=s["shs"].numpy(), sh_degree=sh_degree)
    args.update(over)
    return oracle.forward(**kw, **args)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def settings_from(s, device, sh_degree=0, debug=False):
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    cam = s["cam"]
    return GaussianRasterizationSettings(
        image_height=cam["image_height"], image_width=cam["image_width"], tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"],
        bg=s["bg"].to(device), scale_modifier=1.0, viewmatrix=cam["viewmatrix"].to(device),
        projmatrix=cam["projmatrix"].to(device), sh_degree=sh_degree, campos=cam["campos"].to(device),
        prefiltered=False, debug=debug)


def validate_bench_line(d, default_workload=True, n_gpus=1, round3_accounting=False, full=True, trimmed=False):
    """The driver's bench.py contract (one JSON line) + this repo's additions; used on a LIVE run (tests/test_bench_gpu.py), on
    the committed lines of the rounds and on the driver's own records BENCH_rNN.json (tests/test_abi_cpu.py).  The driver keeps a
    trimmed copy of the line (`parsed`: no `config.paths`, no `roofline.kernels`), so those parts are checked where present;
    trimmed=True (the driver's records) also drops the nested objects of `roofline` (`roofline.hbm`), which a live line must carry.
    full=False: the line of a plain run (no --full), the headline and its own timed loop only -- everything that takes runs or
    loops of its own (roofline, cpu_baseline, sustained, comm, config.paths, render times) must be absent from it.
    Nothing here asserts an ORDER between measured throughputs of fast paths: round 3's validator required patched <= 1.02 x
    fused, and the driver's own box violated it (its first timed loop carried 2 ms of GPU idle the later loops did not)."""
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config") + (("roofline",) if full else ()):
        assert k in d, k
    assert d["metric"] == "train_iters_per_sec" and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert d["n_gpus"] == n_gpus and d["scaling"] == "weak" and d["data"] == "synthetic" and d["dtype"] == "f32"
    assert abs(d["value"] - d["n_gpus"] * 1000.0 / d["ms_per_step"]) < 0.02 * d["value"]
    if d.get("sustained") is not None:     # round 5: >= 300 untended steps after the timed burst
        su = d["sustained"]
        assert su["steps"] >= 100 and su["iters_per_s"] > 0 and su["step_ms_median"] <= su["step_ms_p99"] <= su["step_ms_max"]
        assert d["sustained_iters_per_s"] == su["iters_per_s"] and d["step_ms_p99"] == su["step_ms_p99"] and su["arena_overflows"] == 0
    if "step_ms_median" in d:     # round 4: one hipEvent pair per step + the host's enqueue time
        assert 0 < d["step_ms_min"] <= d["step_ms_median"] <= d["step_ms_max"]
        assert d["host_enqueue_ms_per_step"] > 0 and d["gpu_ms_per_step"] > 0
        assert d["gpu_ms_per_step"] <= 1.05 * d["ms_per_step"] + 0.05    # stream time between step boundaries cannot exceed the wall
    if d.get("longest_host_enqueue_of_one_step_ms") is not None:     # round 5: what a host stall inside the 0.15-s region looks like
        assert d["longest_host_enqueue_of_one_step_ms"] > 0 and d["gc_gen1_passes_in_timed_loop"] >= 0
    c = d["config"]
    if n_gpus == 1:
        assert ("BASELINE cfg3" in c["workload"]) == default_workload, c["workload"]     # the label is derived from the arguments
    else:
        assert (f"over {n_gpus} ranks" in c["workload"]) == default_workload, c["workload"]
    assert str(c["gaussians"]) in c["workload"]
    assert c["path"] == "fused"
    if "paths" in c:
        assert {"fused", "patched", "import_swap", "zero_diff"} <= set(c["paths"]) <= {
            "fused", "patched", "import_swap", "zero_diff", "fused_mlp_bf16x3", "fused_mlp_f32", "heavy_raster"}
        ips = {k: v["iters_per_s"] for k, v in c["paths"].items() if k not in ("fused_mlp_bf16x3", "fused_mlp_f32", "heavy_raster")}
        if "fused_mlp_f32" in c["paths"]:        # round 6: bf16x3 is the default, the exact chain is the leg
            assert c["paths"]["fused_mlp_f32"].get("ms_per_step") and c["mlp_arithmetic"].startswith("bf16x3"), c["paths"]["fused_mlp_f32"]
        if "heavy_raster" in c["paths"]:     # round 6: the same step with ~8 x the (tile, Gaussian) instances
            hr = c["paths"]["heavy_raster"]
            assert hr.get("ms_per_step") and hr["arena_overflows"] == 0 and hr["instances_R_per_view"] > c["instances_R_per_view"], hr
        if "fused_mlp_bf16x3" in c["paths"]:     # the opt-in arithmetic of the MLP kernels: timed, never the headline
            assert c["paths"]["fused_mlp_bf16x3"].get("ms_per_step"), c["paths"]["fused_mlp_bf16x3"]
        # the slow routes are slow by an order of magnitude (plain PyTorch deformation field / 24 grid_samples): that much is structural
        assert ips["zero_diff"] < ips["import_swap"] < min(ips["patched"], ips["fused"]), ips
        # tolerant order between the two fast paths: the fused step never syncs, the patched route keeps train.py's
        # loss.item() -- a fused path slower than 0.85 x the patched one would be a regression of the headline path
        assert ips["fused"] >= 0.85 * ips["patched"], ips
    if "render_ms_per_frame_bf16x3" in c:     # faster only where the deformation kernel matters: no ordering asserted on small scenes
        assert c["render_ms_per_frame_bf16x3"] > 0
    assert c["instances_R_per_view"] > 0 and c["visible_V_per_view"] > 0 and c["mean_tile_list_length"] > 0
    for key in ("psnr_delta_vs_oracle_db", "psnr_mean_delta_vs_oracle_db"):
        if c.get(key) is not None:
            assert abs(c[key]) <= 0.1
    if "raster_async" in c:
        assert c["raster_async"]["overflows"] == []      # a step that overflowed its arena did no work: never inside the timed loop
    if not full:
        assert not {"roofline", "cpu_baseline", "sustained", "comm"} & set(d), sorted(d)
        assert not {"paths", "render_ms_per_frame"} & set(c), sorted(c)
        return
    assert c["render_ms_per_frame"] > 0
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma", "valu") and r["unit"] in ("GB/s", "TFLOP/s", "G wave-instructions/s")
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    if r["bound"] == "valu" and not (trimmed and "hbm" not in r):      # round 6: the roof the dominant kernel sits closest to; the HBM figure travels beside it
        assert abs(r["hbm"]["frac"] - r["hbm"]["achieved"] / r["hbm"]["peak"]) < 1e-3 and r["hbm"]["frac"] <= r["frac"]
    if r["traffic"] is not None:
        # (the driver's record keeps the first 128 characters of every string)
        assert ("NOT collected in this run" in r["traffic_source"] or r["traffic_source"].startswith("profiles/kernel_traffic.json")
                or r["traffic_source"].startswith("collected IN THIS RUN"))
    if "kernels" in r:
        dom = max(r["kernels"], key=lambda k: k["ms_per_step"])
        assert dom["kernel"] == r["kernel"]
        for k in r["kernels"]:
            assert k["algorithmic_bytes_per_launch"] <= k["implementation_bytes_per_launch"] and k["avg_launch_ms"] > 0
            if "valu_frac" in k and k["valu_frac"] is not None:   # every kernel with a SQ_INSTS_VALU count is priced on the VALU roof too
                assert 0 < k["valu_frac"] <= 1.05 and k["frac"] >= k["valu_frac"] - 1e-3 and k["frac"] >= k["hbm_frac"] - 1e-3
            if k["kernel"].startswith("s3g::blend_") and not round3_accounting:   # (round 3's lines carry the two bugs below)
                assert k["bound"] == "valu"                    # VALU / v_exp-bound, never priced as an HBM kernel
                assert abs(k["launches_per_step"] - 1.0) < 1e-6, k   # ONE two-image launch per step (round 3 mixed the render loop in)
    if n_gpus > 1:
        cm = d["comm"]
        assert cm["world_size"] == n_gpus and len(cm["devices"]) == n_gpus and cm["backend"] in ("nccl", "gloo")
        return
    assert "cpu_baseline" in d
    cb = d["cpu_baseline"]
    assert cb["kind"] in ("port", "reference") and cb["cores"] >= 1 and cb["value"] > 0      # "reference": the reference's own modules on the host
    if "what" in cb:          # round 3 on: the top-level baseline is the north_star's point-splat stub, one real full-size iteration
        assert cb["what"] == "point_splat"
        assert "measured, not extrapolated" in cb["sample"] or cb["sample"].startswith("ONE full iteration of the workload itself")
    if "tile_rasterizer_port" in cb:
        tr = cb["tile_rasterizer_port"]
        assert tr["value"] > 0 and len(tr["model"]["sample_P"]) == 3 and len(tr["model"]["fit_residual_rel"]) == 3
