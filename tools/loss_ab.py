#!/usr/bin/env python
"""Image-space loss stage: the tree's fused strip-walking launches against the parent commit's five kernels, in one process.

    python tools/loss_ab.py --build-parent [REV]     (CPU box: compiles REV's csrc/ssim.hip -- default HEAD -- with the Makefile's flags
                                                      and links it with the tree's objects that define none of its entry points into
                                                      s3gaussian_amd/lib/variants/libs3g_loss_parent.so, as tools/mkvariants.py does)
    python tools/loss_ab.py [--reps 30] [--warmup 5] [--out profiles/loss_stage_ab_tool.txt]          (GPU box)

At 1066 x 1600 the tool loads the tree's library (the package's own) and the parent build (ctypes, second library) and runs, on the
seeded inputs of tests/test_loss_stage_gpu.py and on a rendered street-scene view with its targets:

  parent  s3g_ssim_forward + s3g_pixel_losses_forward + s3g_pixel_losses_combine; backward: the torch multiply g * (-w_ssim),
          s3g_ssim_backward, s3g_pixel_losses_backward with accumulate_image = 1           (what losses.photometric_loss ran)
  tree    s3g_photometric_forward + s3g_pixel_losses_combine; backward: s3g_photometric_backward

(a) Exactness.  The three maps, g_image, g_depth and g_feat of the two routes must be torch.equal.  The five totals are compared by
    relative difference; the bar is 4 x the distance of the PARENT's totals from a float64 sum (for [1] to [4] of the same fp32
    per-pixel values, formed with torch; for [0], whose per-pixel values no entry point stores, of the SSIM map evaluated in
    float64 on the GPU, which also counts the per-pixel fp32 rounding).
(b) Timing.  Event medians of forward + backward of the stage, the routes alternated.  There is no speed gate."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
PARENT_SO = os.path.join(ROOT, "s3gaussian_amd", "lib", "variants", "libs3g_loss_parent.so")
H, W = 1066, 1600
MAX_DEPTH = 80.0


def build_parent(rev):
    import glob
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import mkvariants as mk
    os.makedirs(mk.OUT, exist_ok=True)
    src = subprocess.check_output(["git", "-C", ROOT, "show", f"{rev}:s3gaussian_amd/csrc/ssim.hip"]).decode()
    tmp_src, obj = os.path.join(mk.SRC, "_variant_loss_parent.hip"), os.path.join(mk.OUT, "loss_parent.o")
    try:
        open(tmp_src, "w").write(src)
        subprocess.check_call(["/opt/rocm/bin/hipcc", *mk.FLAGS, "-c", tmp_src, "-o", obj])
    finally:
        if os.path.exists(tmp_src):
            os.remove(tmp_src)
    # REV's ssim.hip may hold more than the tree's (it held the pixel-loss and plane-regulariser families before they got files of
    # their own): leave out every tree object that defines an entry point the parent object defines
    exports = lambda o: {l.split()[-1] for l in subprocess.check_output(["nm", "--defined-only", o]).decode().splitlines()
                         if l.split()[-1].startswith("s3g_")}
    parent = exports(obj)
    objs = [o for o in glob.glob(os.path.join(mk.LIB, "*.o")) if not exports(o) & parent] + [obj]
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", PARENT_SO])
    os.remove(obj)
    print(PARENT_SO)


def bind_parent():
    L = C.CDLL(PARENT_SO)
    vp, ci, cf = C.c_void_p, C.c_int, C.c_float
    L.s3g_ssim_forward.argtypes = [ci, ci, ci, vp, vp, vp, vp, vp, vp, vp]
    L.s3g_ssim_backward.argtypes = [ci, ci, ci, vp, vp, vp, vp, vp, vp, vp, vp]
    L.s3g_pixel_losses_forward.argtypes = [ci, ci, vp, vp, vp, vp, vp, vp, cf, vp, vp]
    L.s3g_pixel_losses_combine.argtypes = [ci, ci, vp, vp, cf, cf, cf, cf, vp, vp]
    L.s3g_pixel_losses_backward.argtypes = [ci, ci, vp, vp, vp, vp, vp, vp, cf, vp, vp, cf, cf, cf, vp, ci, vp, vp, vp]
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--build-parent", nargs="?", const="HEAD", default=None, metavar="REV")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_stage_ab_tool.txt"))
    args = ap.parse_args()
    if args.build_parent is not None:
        return build_parent(args.build_parent)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("loss_ab.py measures on the GPU; there is none here (nothing measured)")
    if not os.path.exists(PARENT_SO):
        raise SystemExit(f"{PARENT_SO} is missing: run `python tools/loss_ab.py --build-parent` where hipcc is")
    import bench
    from s3gaussian_amd import _lib, losses
    from s3gaussian_amd.pipeline import default_opt
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    T, P = losses._bind(), bind_parent()
    opt = default_opt()
    w_ssim, w_depth, w_feat = float(opt.lambda_dssim), float(opt.lambda_depth), float(opt.lambda_feat)
    SD = losses.SUM_DOUBLES
    p = lambda t: t.data_ptr()
    g = torch.full((1,), 1.0, device=dev)

    def fresh():
        return dict(sums=torch.zeros(5 * SD + 5, dtype=torch.float64, device=dev), maps=torch.empty((3, 3, H, W), device=dev),
                    loss=torch.empty((), device=dev), g_img=torch.empty((3, H, W), device=dev), g_dep=torch.empty((1, H, W), device=dev),
                    g_ft=torch.empty((3, H, W), device=dev))

    def route(tree, ins, o):
        img, gt, dep, gdep, ft, gft = ins
        st = _lib.stream_ptr()
        sums, maps, totals = o["sums"], o["maps"], o["sums"][5 * SD:]
        sums.zero_()
        if tree:
            _lib.check(T.s3g_photometric_forward(H, W, p(img), p(gt), p(dep), p(gdep), p(ft), p(gft), MAX_DEPTH, p(sums), p(maps[0]),
                                                 p(maps[1]), p(maps[2]), st))
            _lib.check(T.s3g_pixel_losses_combine(H, W, p(sums), p(totals), 1.0, w_depth, w_ssim, w_feat, p(o["loss"]), st))
            _lib.check(T.s3g_photometric_backward(H, W, p(img), p(gt), p(dep), p(gdep), p(ft), p(gft), MAX_DEPTH, p(maps[0]), p(maps[1]),
                                                  p(maps[2]), p(totals), p(g), w_ssim, 1.0, w_depth, w_feat, p(o["g_img"]), p(o["g_dep"]),
                                                  p(o["g_ft"]), st))
        else:
            rc = P.s3g_ssim_forward(3, H, W, p(img), p(gt), p(sums), p(maps[0]), p(maps[1]), p(maps[2]), st)
            rc |= P.s3g_pixel_losses_forward(H, W, p(img), p(gt), p(dep), p(gdep), p(ft), p(gft), MAX_DEPTH, p(sums), st)
            rc |= P.s3g_pixel_losses_combine(H, W, p(sums), p(totals), 1.0, w_depth, w_ssim, w_feat, p(o["loss"]), st)
            gs = g * (-w_ssim)
            rc |= P.s3g_ssim_backward(3, H, W, p(img), p(gt), p(maps[0]), p(maps[1]), p(maps[2]), p(gs), p(o["g_img"]), st)
            rc |= P.s3g_pixel_losses_backward(H, W, p(img), p(gt), p(dep), p(gdep), p(ft), p(gft), MAX_DEPTH, p(totals), p(g), 1.0,
                                              w_depth, w_feat, p(o["g_img"]), 1, p(o["g_dep"]), p(o["g_ft"]), st)
            if rc:
                raise SystemExit("a parent entry point failed")

    def seeded():
        from tests.test_loss_stage_gpu import _inputs
        return tuple(t.to(dev).contiguous() for t in _inputs(H, W, seed=11))

    def rendered():
        from types import SimpleNamespace
        from s3gaussian_amd.pipeline import render
        pc, cams, hyper, _, bg = bench.build_scene(300_000, W, H, 2, dev)
        gt, gdep, gft = bench.make_targets(pc, cams[1], bg, hyper, seed=1001)
        pipe = SimpleNamespace(convert_SHs_python=True, compute_cov3D_python=False, debug=False)
        with torch.no_grad():
            pkg = render(cams[1], pc, pipe, bg, stage="fine", render_feat=True)
        return tuple(t.detach().float().contiguous() for t in (pkg["render"], gt, pkg["depth"], gdep, pkg["feat"], gft))

    def f64_totals(ins):
        img, gt, dep, gdep, ft, gft = ins
        import math
        gk = torch.tensor([math.exp(-(x - 5) ** 2 / (2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32, device=dev)
        gk = (gk / gk.sum()).double()

        def conv(x):
            xp = torch.nn.functional.pad(x, (5, 5, 5, 5))
            h = sum(gk[k] * xp[..., :, k:k + W] for k in range(11))
            return sum(gk[k] * h[..., k:k + H, :] for k in range(11))
        a, b = img.double(), gt.double()
        mu1, mu2 = conv(a), conv(b)
        s1, s2, s12 = conv(a * a) - mu1 * mu1, conv(b * b) - mu2 * mu2, conv(a * b) - mu1 * mu2
        c1, c2 = 0.01 ** 2, 0.03 ** 2
        t0 = (((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))).sum()
        m = (gdep > 0.01) & (gdep < MAX_DEPTH)
        dd = (torch.clamp(dep / MAX_DEPTH, 0, 1) - torch.clamp(gdep / MAX_DEPTH, 0, 1))[m]
        df = ft - gft
        return [t0.item(), (img - gt).abs().double().sum().item(), (dd * dd).double().sum().item(), float(m.sum().item()),
                (df * df).double().sum().item()]

    lines = [f"# tools/loss_ab.py --reps {args.reps} --warmup {args.warmup}: loss stage at {H} x {W}, w_ssim {w_ssim} w_depth {w_depth} w_feat {w_feat};",
             f"# parent build {os.path.relpath(PARENT_SO, ROOT)} against the tree's library, one process.  {torch.cuda.get_device_name(0)}"]
    ok = True
    sets = {"seeded": seeded(), "rendered street-scene view": rendered()}
    for name, ins in sets.items():
        op, ot = fresh(), fresh()
        route(False, ins, op)
        route(True, ins, ot)
        torch.cuda.synchronize()
        eq = {k: torch.equal(op[k], ot[k]) for k in ("maps", "g_img", "g_dep", "g_ft")}
        ok &= all(eq.values())
        tp, tt, t64 = op["sums"][5 * SD:].tolist(), ot["sums"][5 * SD:].tolist(), f64_totals(ins)
        rel = lambda x, y: abs(x - y) / max(abs(y), 1e-300)
        lines.append(f"## exactness, {name}: " + "  ".join(f"{k} equal: {v}" for k, v in eq.items()))
        for q, label in enumerate(("ssim", "l1", "depth sq", "depth count", "feat sq")):
            bar = 4 * rel(tp[q], t64[q])
            d = rel(tt[q], tp[q])
            good = d <= bar
            ok &= good
            lines.append(f"  total[{q}] {label:11s} parent {tp[q]:.15g}  tree {tt[q]:.15g}  rel diff {d:.2e}  bar 4 x |parent - f64| {bar:.2e}  {'ok' if good else 'OVER'}")
        lines.append(f"  loss parent {op['loss'].item():.9g}  tree {ot['loss'].item():.9g}")
    ins = sets["rendered street-scene view"]
    op, ot = fresh(), fresh()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = {False: [], True: []}
    for rep in range(args.warmup + args.reps):
        for tree in (False, True):
            torch.cuda.synchronize()
            ev[0].record()
            route(tree, ins, ot if tree else op)
            ev[1].record()
            torch.cuda.synchronize()
            if rep >= args.warmup:
                times[tree].append(ev[0].elapsed_time(ev[1]) * 1e3)
    mp, mt = statistics.median(times[False]), statistics.median(times[True])
    lines.append(f"## timing, forward + backward of the stage incl. the sums memset, us (events; medians of {args.reps}, routes alternated)")
    lines.append(f"  parent  median {mp:.1f}  min {min(times[False]):.1f}  max {max(times[False]):.1f}   (5 kernels + 1 torch multiply)")
    lines.append(f"  tree    median {mt:.1f}  min {min(times[True]):.1f}  max {max(times[True]):.1f}   (3 kernels)")
    lines.append(f"  tree - parent {mt - mp:+.1f} us ({(mt / mp - 1) * 100:+.1f} %)")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")
    if not ok:
        raise SystemExit("exactness: a per-pixel tensor differs or a total is over its bar")


if __name__ == "__main__":
    main()
