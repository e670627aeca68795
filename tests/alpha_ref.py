"""Shared pieces of the accumulated-opacity / sky-loss tests: the two scenes, a float64 restatement of the loss, the oracle
readings of the opacity gradient, and recorded-once references (computed on first use, shared, never modified)."""
from __future__ import annotations

import functools
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests.util import oracle_forward, tiny_scene

BLACK = (0.0, 0.0, 0.0)
COLOUR = (0.2, 0.5, 0.7)
LO, HI = 1e-6, 1.0 - 1e-6


def scene_a(bg=COLOUR):
    """37 x 29 (3 x 2 tiles, the right column and the bottom row partial: lanes outside the image), 300 Gaussians, none of them
    near the top-left corner: its tile keeps an empty list and its pixels no contributor."""
    W, H = 37, 29
    s = tiny_scene(P=300, W=W, H=H, seed=3, scale=0.07, bg=bg)
    g = torch.Generator().manual_seed(17)
    x, y, z = s["means3D"].unbind(1)
    tx, ty = s["cam"]["tanfovx"], s["cam"]["tanfovy"]
    u, v = x / (z * tx), y / (z * ty)                          # normalised device coordinates, -1 .. 1
    corner = (u < 0.25) & (v < 0.5)                            # would reach the first 16 x 16 tile (with its 3-sigma extent)
    u = torch.where(corner, 0.3 + 0.7 * torch.rand(300, generator=g), u)
    s["means3D"] = torch.stack([u * z * tx, y, z], 1).contiguous()
    return s


def scene_b(bg=COLOUR):
    """64 x 48, 1500 Gaussians piled in the middle of the view, many nearly opaque: tile lists longer than one 32-entry batch of the
    blend backward, pixels that stop early (T < 1e-4) and alphas at the 0.99 cap."""
    s = tiny_scene(P=1500, W=64, H=48, seed=5, scale=0.2, spread=0.8, bg=bg)
    g = torch.Generator().manual_seed(23)
    s["opacities"] = torch.sigmoid(2.0 + 1.5 * torch.randn(1500, 1, generator=g))
    s["opacities"][::7] = 0.999
    return s


SCENES = {"A": scene_a, "B": scene_b}


def unit_black(s):
    """The same geometry with unit colours on a black background: its red channel is the accumulated opacity."""
    u = dict(s)
    u["colors_precomp"] = torch.ones_like(s["colors_precomp"])
    u["bg"] = torch.zeros(3)
    return u


def upstream(H, W, seed=5):
    """(c [3,H,W], d [1,H,W], g_A [1,H,W]) fp32 upstream gradients."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(3, H, W, generator=g), torch.randn(1, H, W, generator=g), torch.randn(1, H, W, generator=g)


@functools.lru_cache(maxsize=None)
def oracle64():
    from oracle.oracle import RasterOracle
    return RasterOracle(np.float64)


@functools.lru_cache(maxsize=None)
def forward64(name: str, bg=COLOUR):
    """Float64 oracle forward of a scene (cached; treat as read-only)."""
    return oracle_forward(oracle64(), SCENES[name](bg))


@functools.lru_cache(maxsize=None)
def forward64_unit(name: str):
    return oracle_forward(oracle64(), unit_black(SCENES[name]()))


def alpha64(name: str) -> np.ndarray:
    """[H,W] float64: 1 - final_T of the float64 oracle (the background plays no part in it)."""
    f = forward64(name)
    return 1.0 - f["state"]["final_T"].reshape(f["_cfg"]["H"], f["_cfg"]["W"])


def alpha_backward64(name: str, g_A: np.ndarray) -> dict:
    """Float64 gradients of sum(g_A * A): the oracle's backward of the unit-colour render on black, seeded with (g_A, 0, 0)."""
    f = forward64_unit(name)
    H, W = f["_cfg"]["H"], f["_cfg"]["W"]
    gc = np.zeros((3, H, W))
    gc[0] = np.asarray(g_A, np.float64).reshape(H, W)
    return oracle64().backward(f, gc, np.zeros((1, H, W)))


def bg_dot_reading64(name: str, g_A: np.ndarray, sign=-1.0, forward=None) -> dict:
    """What the blend backward computes for the opacity term: no colour term at all, and g_A entering through the background term
    as bg_dot = sign * g_A (sign = -1: the reading of the kernel; +1: the wrong one).  On the oracle: zero colours (the colour terms
    vanish), background (sign, 0, 0) and the upstream gradient (g_A, 0, 0) give bg . dL_dpixel = sign * g_A."""
    s = SCENES[name]()
    s["colors_precomp"] = torch.zeros_like(s["colors_precomp"])
    s["bg"] = torch.tensor([sign, 0.0, 0.0])
    f = oracle_forward(oracle64(), s) if forward is None else forward(s)
    H, W = f["_cfg"]["H"], f["_cfg"]["W"]
    gc = np.zeros((3, H, W))
    gc[0] = np.asarray(g_A, np.float64).reshape(H, W)
    return oracle64().backward(f, gc, np.zeros((1, H, W)))


def include_terminating_gaussian(f: dict) -> int:
    """The other wrong reading: 1 - sum(w) with the Gaussian that TERMINATED a pixel's walk counted in.  Rewrites the oracle state of
    forward `f` in place -- final_T *= (1 - alpha_k) and n_contrib = k's list position + 1 for every pixel whose walk stopped at an
    entry k (the first entry behind the last contributor that passes the alpha tests) -- and returns how many pixels that were."""
    st, cfg = f["state"], f["_cfg"]
    H, W = cfg["H"], cfg["W"]
    gx = (W + 15) // 16
    n = 0
    for py in range(H):
        for px in range(W):
            lo, hi = (int(v) for v in st["ranges"][(py // 16) * gx + px // 16])
            pix = py * W + px
            for pos in range(lo + int(st["n_contrib"][pix]), hi):
                gid = int(st["point_list"][pos])
                dx, dy = st["means2D"][gid, 0] - px, st["means2D"][gid, 1] - py
                ca, cb, cc, op = st["conic_opacity"][gid]
                power = -0.5 * (ca * dx * dx + cc * dy * dy) - cb * dx * dy
                if power > 0:
                    continue
                alpha = min(0.99, op * math.exp(power))
                if alpha < 1.0 / 255.0:
                    continue
                # the forward skipped every entry behind the last contributor: this one can only have failed the T test
                assert st["final_T"][pix] * (1 - alpha) < 1e-4
                st["final_T"][pix] *= 1 - alpha
                st["n_contrib"][pix] = pos - lo + 1
                n += 1
                break
    return n


def sky_loss_ref(alpha: torch.Tensor, sky_mask: torch.Tensor, dtype=torch.float64):
    """(loss, d loss / d alpha) of mean(-(1 - s) log(a) - s log(1 - a)), a = clamp(alpha, 1e-6, 1 - 1e-6), restated with
    F.binary_cross_entropy on the clamped image, in `dtype` on the CPU.  alpha / sky_mask: any shape, same number of elements."""
    a = alpha.detach().cpu().to(dtype).reshape(-1).requires_grad_(True)
    s = sky_mask.detach().cpu().to(dtype).reshape(-1)
    loss = F.binary_cross_entropy(torch.clamp(a, LO, HI), 1.0 - s)
    (g,) = torch.autograd.grad(loss, a)
    return loss.detach(), g.reshape(alpha.shape)


def sky_inputs(H, W, seed=0):
    """An opacity image with exact 0 and 1, values inside and outside the clamp on both sides, and a soft mask."""
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(H, W, generator=g)
    flat = a.view(-1)
    # (no value ON a clamp bound: float32(1e-6) < 1e-6, so the float64 restatement would clamp what fp32 arithmetic passes)
    special = torch.tensor([0.0, 1.0, 5e-7, 2e-6, 1.0 - 5e-7, 1.0 - 2e-6, 0.5, 1e-3, 0.999])
    idx = torch.randperm(flat.numel(), generator=g)[: 4 * special.numel()]
    flat[idx] = special.repeat(4)
    s = torch.rand(H, W, generator=g)
    s[torch.rand(H, W, generator=g) < 0.3] = 1.0      # hard sky
    s[torch.rand(H, W, generator=g) < 0.3] = 0.0      # hard ground
    return a.contiguous(), s.contiguous()


# ---- the sky term of a training step, as a float64 / float32 chain beside tests/step_ref.py --------------------------------------
def sky_mask_for(H, W, seed=0):
    """A soft sky mask: sky above a wavy horizon, a bilinear-looking ramp of a few pixels across it."""
    g = torch.Generator().manual_seed(100 + seed)
    y = torch.arange(H, dtype=torch.float32)[:, None]
    horizon = 0.35 * H + 0.08 * H * torch.sin(torch.arange(W, dtype=torch.float32)[None, :] * (6.28 / W) + torch.rand(1, generator=g))
    return torch.clamp((horizon - y) / 3.0 + 0.5, 0.0, 1.0).contiguous()


def sky_step(case, sky_mask, lam, dtype=torch.float64, camera=None, weight_of_view=1.0):
    """The sky term ALONE through the chain of step_ref.reference_step (which has no slot for it; by linearity its gradients add to
    that function's): deformation + activations as there, the oracle's render of unit colours on black (its red channel is the
    accumulated opacity), lam * weight_of_view * binary_cross_entropy(clamp(A), 1 - sky_mask), the oracle's backward seeded with
    (dloss/dA, 0, 0).  -> dict(loss, grads {product parameter name: float64 array or None}, dL_dmeans2D, alpha)."""
    from oracle import hexplane_ref as hr
    from oracle.oracle import RasterOracle
    from tests import step_ref as sr
    dt = dtype
    npdt = np.float32 if dt == torch.float32 else np.float64
    hy, cam, fine = case["hyper"], (case["camera"] if camera is None else camera), case["stage"] == "fine"
    with torch.random.fork_rng():
        net = hr.deform_network(hy)
    net.load_state_dict(case["state"])
    net = net.to(dt)
    L = {k: v.clone().to(dt).requires_grad_(True) for k, v in case["leaves"].items()}
    xyz = L["_xyz"]
    if fine:
        shs0 = torch.cat([L["_features_dc"], L["_features_rest"]], 1)
        time_t = torch.full((sr.P, 1), cam["time"], dtype=dt)
        m3, s, r, o = net(xyz, L["_scaling"], L["_rotation"], L["_opacity"], shs0, time_t)[:4]
    else:
        m3, s, r, o = xyz, L["_scaling"], L["_rotation"], L["_opacity"]
    scales, rots, opac = torch.exp(s), torch.nn.functional.normalize(r), torch.sigmoid(o)
    n = lambda t_: t_.detach().numpy()
    Hh, Ww = int(cam["image_height"]), int(cam["image_width"])
    orc = RasterOracle(npdt)
    fwd = orc.forward(means3D=n(m3), opacities=n(opac), scales=n(scales), rotations=n(rots),
                      colors_precomp=np.ones((sr.P, 3), npdt), sh_degree=0, bg=np.zeros(3, npdt),
                      viewmatrix=cam["viewmatrix"].numpy().astype(npdt), projmatrix=cam["projmatrix"].numpy().astype(npdt),
                      campos=cam["campos"].numpy().astype(npdt), tanfovx=cam["tanfovx"], tanfovy=cam["tanfovy"], image_height=Hh,
                      image_width=Ww, scale_modifier=case.get("scale_modifier", 1.0))
    A = torch.from_numpy(1.0 - fwd["state"]["final_T"].reshape(Hh, Ww)).to(dt).requires_grad_(True)
    loss = lam * weight_of_view * F.binary_cross_entropy(torch.clamp(A, LO, HI), 1.0 - sky_mask.to(dt).reshape(Hh, Ww))
    loss.backward()
    gc = np.zeros((3, Hh, Ww), npdt)
    gc[0] = A.grad.numpy()
    g = orc.backward(fwd, gc, np.zeros((1, Hh, Ww), npdt))
    t = torch.from_numpy
    surrogate = ((m3 * t(g["dL_dmeans3D"])).sum() + (scales * t(g["dL_dscales"])).sum() + (rots * t(g["dL_drotations"])).sum()
                 + (opac * t(g["dL_dopacity"])).sum())
    surrogate.backward()
    grads = {k: (None if v.grad is None else v.grad.double().numpy()) for k, v in L.items()}
    for name, p in net.named_parameters():
        if p.requires_grad:
            grads["_deformation." + name] = None if p.grad is None else p.grad.double().numpy()
    return dict(loss=float(loss.detach()), grads=grads, dL_dmeans2D=g["dL_dmeans2D"].astype(np.float64), alpha=A.detach().double().numpy())


def add_steps(base, *extra):
    """Sum of reference_step-shaped results (loss, grads, dL_dmeans2D); a gradient is None only where every part has none."""
    out = dict(base)
    out["grads"] = dict(base["grads"])
    for e in extra:
        out["loss"] = out["loss"] + e["loss"]
        out["dL_dmeans2D"] = out["dL_dmeans2D"] + e["dL_dmeans2D"]
        for k, v in e["grads"].items():
            if v is not None:
                out["grads"][k] = v if out["grads"].get(k) is None else out["grads"][k] + v
    return out


# ---- the three video keys, restated from utils/video_utils.py:461-489 ------------------------------------------------------------
SKY_FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sky_frames.npz")
VIDEO_KEYS = ("opacities", "sky_masks", "gt_sky_masks")


def video_strips(opacities, gt_sky_masks, num_cams):
    """{key: [T strips]} as save_seperate_videos writes them: `opacities` / `gt_sky_masks` are lists of [H,W] fp32 arrays, one per
    camera.  "opacities": to8b(concatenate(frames, axis=1)), [H, n W]; "sky_masks": frames = 1 - np.stack([o, o, o], axis=-1) (fp32),
    [H, n W, 3]; "gt_sky_masks": frames = np.stack([m, m, m], axis=-1)."""
    from tests import frames_ref as fr
    n = num_cams
    T = len(opacities) // n
    out = {k: [] for k in VIDEO_KEYS}
    for t in range(T):
        o = [np.asarray(x, np.float32) for x in opacities[t * n:(t + 1) * n]]
        out["opacities"].append(fr.to8b(np.concatenate(o, axis=1)))
        out["sky_masks"].append(fr.to8b(np.concatenate([1 - np.stack([x, x, x], axis=-1) for x in o], axis=1)))
        if gt_sky_masks is not None:
            m = [np.asarray(x, np.float32) for x in gt_sky_masks[t * n:(t + 1) * n]]
            out["gt_sky_masks"].append(fr.to8b(np.concatenate([np.stack([x, x, x], axis=-1) for x in m], axis=1)))
    return out
