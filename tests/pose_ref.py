"""float64 restatements for the camera-gradient tests (TEST INFRASTRUCTURE ONLY).

camera_terms_ref: the per-Gaussian terms of include/s3g_camera.h::s3g_camera_backward in numpy float64, from the same
per-Gaussian arrays the kernel reads, every operation in the order the kernel writes it (IEEE double on both sides, no
contraction: a Gaussian's terms are then the same numbers and the two sides differ in the order of the sum over P only).
Returns the 35 sums and, per output, the sum of |term| that the tests' bars are relative to.

pose_map_ref: the pose map in plain torch float64, so that autograd gives its derivative.
"""
from __future__ import annotations

import numpy as np
import torch

SH_C1 = 0.4886025119029199
SH_C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
SH_C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
         1.445305721320277, -0.5900435899266435]

UNUSED = (3, 7, 11, 15, 18, 22, 26, 30)     # view[3,7,11,15], proj[2,6,10,14]: in no product of the forward
BLOCKS = {"view": slice(0, 16), "proj": slice(16, 32), "campos": slice(32, 35)}


def _f64(a, shape):
    return None if a is None else np.asarray(a, np.float32).astype(np.float64).reshape(shape)


def camera_terms_ref(*, P, means3D=None, radii=None, cov3D=None, clamped=None, viewmatrix=None, projmatrix=None, campos=None,
                     tanfovx=None, tanfovy=None, image_height=None, image_width=None, dL_dmeans2D=None, dL_dconic=None,
                     dL_ddepths=None, dL_dcolors=None, shs=None, sh_degree=0, g_dir=None):
    """-> (sums [35] float64, abs_sums [35] float64).  All array arguments are what the kernel reads, as fp32 values: cov3D is the
    forward's (or the precomputed) [P,6], clamped the forward's [P,3] flags; tanfov as the fp32 values of s3g_raster_inputs."""
    term = np.zeros((P, 35), np.float64)
    if P == 0:
        return term.sum(0), np.abs(term).sum(0)
    vis = np.zeros(P, bool) if radii is None else (np.asarray(radii).reshape(P) > 0)
    m = _f64(means3D, (P, 3))
    tv = np.zeros((P, 12))
    tp = np.zeros((P, 12))
    tc = np.zeros((P, 3))
    with np.errstate(all="ignore"):
        if dL_dconic is not None or dL_ddepths is not None:
            dc = np.zeros((P, 4)) if dL_dconic is None else _f64(dL_dconic, (P, 4))
            dcx, dcy, dcz = dc[:, 0], dc[:, 1], dc[:, 3]
            gdep = np.zeros(P) if dL_ddepths is None else _f64(dL_ddepths, (P,))
            conic_live = vis & ((dcx != 0) | (dcy != 0) | (dcz != 0))
            live = vis & (conic_live | (gdep != 0))
            gt = np.zeros((P, 3))
            gt[:, 2] = gdep
            tvc = np.zeros((P, 12))
            if dL_dconic is not None:
                view = _f64(viewmatrix, (16,))
                V = np.array([view[4 * k + i] for k in range(4) for i in range(3)])      # V[3k+i] = view[4k+i]
                tanx, tany = float(np.float32(tanfovx)), float(np.float32(tanfovy))
                fx, fy = float(image_width) / (2.0 * tanx), float(image_height) / (2.0 * tany)
                limx, limy = 1.3 * tanx, 1.3 * tany
                t = [V[i] * m[:, 0] + V[3 + i] * m[:, 1] + V[6 + i] * m[:, 2] + V[9 + i] for i in range(3)]
                tz = t[2]
                txtz, tytz = t[0] / tz, t[1] / tz
                xm = np.where((txtz < -limx) | (txtz > limx), 0.0, 1.0)
                ym = np.where((tytz < -limy) | (tytz > limy), 0.0, 1.0)
                txc = np.minimum(limx, np.maximum(-limx, txtz)) * tz
                tyc = np.minimum(limy, np.maximum(-limy, tytz)) * tz
                J00, J11 = fx / tz, fy / tz
                J02, J12 = -(fx * txc) / (tz * tz), -(fy * tyc) / (tz * tz)
                S = _f64(cov3D, (P, 6))
                Sm = [[S[:, 0], S[:, 1], S[:, 2]], [S[:, 1], S[:, 3], S[:, 4]], [S[:, 2], S[:, 4], S[:, 5]]]
                T0 = [V[3 * k] * J00 + V[3 * k + 2] * J02 for k in range(3)]
                T1 = [V[3 * k + 1] * J11 + V[3 * k + 2] * J12 for k in range(3)]
                U0 = [Sm[k][0] * T0[0] + Sm[k][1] * T0[1] + Sm[k][2] * T0[2] for k in range(3)]
                U1 = [Sm[k][0] * T1[0] + Sm[k][1] * T1[1] + Sm[k][2] * T1[2] for k in range(3)]
                ca = (T0[0] * U0[0] + T0[1] * U0[1] + T0[2] * U0[2]) + 0.3
                cb = T0[0] * U1[0] + T0[1] * U1[1] + T0[2] * U1[2]
                cc = (T1[0] * U1[0] + T1[1] * U1[1] + T1[2] * U1[2]) + 0.3
                denom = ca * cc - cb * cb
                denom2inv = 1.0 / ((denom * denom) + 0.0000001)
                dL_da = denom2inv * (-cc * cc * dcx + 2.0 * cb * cc * dcy + (denom - ca * cc) * dcz)
                dL_dc = denom2inv * (-ca * ca * dcz + 2.0 * ca * cb * dcy + (denom - ca * cc) * dcx)
                dL_db = denom2inv * 2.0 * (cb * cc * dcx - (denom + 2.0 * cb * cb) * dcy + ca * cb * dcz)
                G0 = [2.0 * U0[k] * dL_da + U1[k] * dL_db for k in range(3)]
                G1 = [2.0 * U1[k] * dL_dc + U0[k] * dL_db for k in range(3)]
                for k in range(3):
                    tvc[:, 3 * k] = G0[k] * J00
                    tvc[:, 3 * k + 1] = G1[k] * J11
                    tvc[:, 3 * k + 2] = G0[k] * J02 + G1[k] * J12
                dJ00 = V[0] * G0[0] + V[3] * G0[1] + V[6] * G0[2]
                dJ02 = V[2] * G0[0] + V[5] * G0[1] + V[8] * G0[2]
                dJ11 = V[1] * G1[0] + V[4] * G1[1] + V[7] * G1[2]
                dJ12 = V[2] * G1[0] + V[5] * G1[1] + V[8] * G1[2]
                itz = 1.0 / tz
                tz2 = itz * itz
                tz3 = tz2 * itz
                gtc = np.stack([xm * -fx * tz2 * dJ02, ym * -fy * tz2 * dJ12,
                                (-fx * tz2 * dJ00 - fy * tz2 * dJ11 + (2.0 * fx * txc) * tz3 * dJ02 + (2.0 * fy * tyc) * tz3 * dJ12) + gdep], 1)
                gt = np.where(conic_live[:, None], gtc, gt)
                tvc = np.where(conic_live[:, None], tvc, 0.0)
            for k in range(3):
                for i in range(3):
                    tvc[:, 3 * k + i] = tvc[:, 3 * k + i] + m[:, k] * gt[:, i]
            for i in range(3):
                tvc[:, 9 + i] = tvc[:, 9 + i] + gt[:, i]
            tv = np.where(live[:, None], tvc, 0.0)
        if dL_dmeans2D is not None:
            g2 = _f64(dL_dmeans2D, (P, 3))
            g2x, g2y = g2[:, 0], g2[:, 1]
            live = vis & ((g2x != 0) | (g2y != 0))
            Pm = _f64(projmatrix, (16,))
            hx = Pm[0] * m[:, 0] + Pm[4] * m[:, 1] + Pm[8] * m[:, 2] + Pm[12]
            hy = Pm[1] * m[:, 0] + Pm[5] * m[:, 1] + Pm[9] * m[:, 2] + Pm[13]
            hw = Pm[3] * m[:, 0] + Pm[7] * m[:, 1] + Pm[11] * m[:, 2] + Pm[15]
            pw = 1.0 / (hw + 0.0000001)
            gh = [g2x * pw, g2y * pw, -(hx * g2x + hy * g2y) * pw * pw]
            tpc = np.zeros((P, 12))
            for k in range(3):
                for c in range(3):
                    tpc[:, 3 * k + c] = m[:, k] * gh[c]
            for c in range(3):
                tpc[:, 9 + c] = gh[c]
            tp = np.where(live[:, None], tpc, 0.0)
        if shs is not None and dL_dcolors is not None and sh_degree > 0:
            deg = int(sh_degree)
            sh = np.asarray(shs, np.float32).astype(np.float64).reshape(P, -1, 3)
            cl = np.asarray(clamped).reshape(P, 3) != 0
            dRGB = np.where(cl, 0.0, _f64(dL_dcolors, (P, 3)))
            live = vis & (dRGB != 0).any(1)
            cp = _f64(campos, (3,))
            v = [m[:, 0] - cp[0], m[:, 1] - cp[1], m[:, 2] - cp[2]]
            sum2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
            ln = np.sqrt(sum2)
            x, y, z = v[0] / ln, v[1] / ln, v[2] / ln
            dd = [np.zeros(P), np.zeros(P), np.zeros(P)]
            C1, C2, C3 = SH_C1, SH_C2, SH_C3
            for ch in range(3):
                SH = lambda k: sh[:, k, ch]
                dRdx, dRdy, dRdz = -C1 * SH(3), -C1 * SH(1), C1 * SH(2)
                if deg > 1:
                    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
                    dRdx = dRdx + (C2[0] * y * SH(4) + C2[2] * 2.0 * -x * SH(6) + C2[3] * z * SH(7) + C2[4] * 2.0 * x * SH(8))
                    dRdy = dRdy + (C2[0] * x * SH(4) + C2[1] * z * SH(5) + C2[2] * 2.0 * -y * SH(6) + C2[4] * 2.0 * -y * SH(8))
                    dRdz = dRdz + (C2[1] * y * SH(5) + C2[2] * 2.0 * 2.0 * z * SH(6) + C2[3] * x * SH(7))
                    if deg > 2:
                        dRdx = dRdx + (C3[0] * SH(9) * 3.0 * 2.0 * xy + C3[1] * SH(10) * yz + C3[2] * SH(11) * -2.0 * xy +
                                       C3[3] * SH(12) * -3.0 * 2.0 * xz + C3[4] * SH(13) * (-3.0 * xx + 4.0 * zz - yy) +
                                       C3[5] * SH(14) * 2.0 * xz + C3[6] * SH(15) * 3.0 * (xx - yy))
                        dRdy = dRdy + (C3[0] * SH(9) * 3.0 * (xx - yy) + C3[1] * SH(10) * xz + C3[2] * SH(11) * (-3.0 * yy + 4.0 * zz - xx) +
                                       C3[3] * SH(12) * -3.0 * 2.0 * yz + C3[4] * SH(13) * -2.0 * xy + C3[5] * SH(14) * -2.0 * yz +
                                       C3[6] * SH(15) * -3.0 * 2.0 * xy)
                        dRdz = dRdz + (C3[1] * SH(10) * xy + C3[2] * SH(11) * 4.0 * 2.0 * yz + C3[3] * SH(12) * 3.0 * (2.0 * zz - xx - yy) +
                                       C3[4] * SH(13) * 4.0 * 2.0 * xz + C3[5] * SH(14) * (xx - yy))
                dd[0] = dd[0] + dRdx * dRGB[:, ch]
                dd[1] = dd[1] + dRdy * dRGB[:, ch]
                dd[2] = dd[2] + dRdz * dRGB[:, ch]
            inv = 1.0 / np.sqrt(sum2 * sum2 * sum2)
            tcc = np.stack([-(((sum2 - v[0] * v[0]) * dd[0] - v[1] * v[0] * dd[1] - v[2] * v[0] * dd[2]) * inv),
                            -((-v[0] * v[1] * dd[0] + (sum2 - v[1] * v[1]) * dd[1] - v[2] * v[1] * dd[2]) * inv),
                            -((-v[0] * v[2] * dd[0] - v[1] * v[2] * dd[1] + (sum2 - v[2] * v[2]) * dd[2]) * inv)], 1)
            tc = np.where(live[:, None], tcc, 0.0)
    if g_dir is not None:
        tc = tc - _f64(g_dir, (P, 3))
    for k in range(4):
        for i in range(3):
            term[:, 4 * k + i] = tv[:, 3 * k + i]
            term[:, 16 + 4 * k + (3 if i == 2 else i)] = tp[:, 3 * k + i]
    term[:, 32:35] = tc
    return term.sum(0), np.abs(term).sum(0)


POSE_SERIES_BELOW = 1e-4


def pose_map_ref(delta6: torch.Tensor, view0: torch.Tensor, proj0: torch.Tensor):
    """-> (view' [4,4], proj' [4,4], campos' [3]) float64, unrounded; differentiable in delta6 (float64 [6])."""
    dt = torch.float64
    w, tau = delta6[:3], delta6[3:]
    A0, P0 = view0.detach().to(dt).reshape(4, 4), proj0.detach().to(dt).reshape(4, 4)
    s = (w * w).sum()
    if float(s.detach()) < POSE_SERIES_BELOW:
        A = 1.0 - s / 6.0 + s * s / 120.0 - s * s * s / 5040.0
        B = 0.5 - s / 24.0 + s * s / 720.0 - s * s * s / 40320.0
    else:
        th = torch.sqrt(s)
        A = torch.sin(th) / th
        B = (1.0 - torch.cos(th)) / s
    zero = torch.zeros((), dtype=dt, device=delta6.device)
    Kx = torch.stack([torch.stack([zero, -w[2], w[1]]), torch.stack([w[2], zero, -w[0]]), torch.stack([-w[1], w[0], zero])])
    E = torch.eye(3, dtype=dt, device=delta6.device) + A * Kx + B * (Kx @ Kx)
    D = torch.eye(4, dtype=dt, device=delta6.device)
    D = torch.cat([torch.cat([E, tau.reshape(3, 1)], 1), D[3:]], 0)
    view = A0 @ D.t()
    R, t = A0[:3, :3], A0[3, :3]
    Ainv = torch.eye(4, dtype=dt, device=delta6.device)
    Ainv[:3, :3] = R.t()
    Ainv[3, :3] = -(t @ R.t())
    proj = view @ (Ainv @ P0)
    campos = -(view[3, :3] @ view[:3, :3].t())
    return view, proj, campos
