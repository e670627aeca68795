"""Float64 restatement of the camera-centre gradient of the render glue: dL/dcampos_v = -sum_p t_v[p].

t_v[p] is the direction term of view v that csrc/glue_views.hip::glue_backward_sh_point returns in `gx`: the SH backward through
dir = normalize(xyz - campos) (the derivation of the reference's backward.cu:20-139), with the clamp_min(., 0) of the colours as
a mask on the colour gradient.  Formed here term by term in float64 from the same formulas, so that a comparison against it sees
the fp32 rounding of the kernel and the order of its sum over P, and nothing else.  tests/test_pose_views_cpu.py pins it to
float64 autograd of oracle/torch_ref._sh_color.
"""
from __future__ import annotations

import torch

from tests.pose_ref import pose_map_ref  # noqa: F401  (the pose map's restatement lives beside the camera terms)

SH_C1 = 0.4886025119029199
SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
SH_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
         -0.5900435899266435)


def direction_terms(deg: int, shs: torch.Tensor, xyz: torch.Tensor, campos: torch.Tensor, g_colors: torch.Tensor,
                    live: torch.Tensor) -> torch.Tensor:
    """-> t [P,3] float64.  shs [P,16,3] (f_dc | f_rest, + dshs), xyz [P,3], campos [3], g_colors [P,3]; live [P,3] bool: the
    colour is above the clamp (its gradient passes)."""
    d64 = lambda a: a.detach().double()
    sh, xyz, campos = d64(shs), d64(xyz), d64(campos).reshape(3)
    dRGB = torch.where(live, d64(g_colors), torch.zeros((), dtype=torch.float64))
    o = xyz - campos
    ox, oy, oz = o[:, 0:1], o[:, 1:2], o[:, 2:3]
    sum2 = ox * ox + oy * oy + oz * oz
    ln = sum2.sqrt()
    x, y, z = ox / ln, oy / ln, oz / ln
    zero = torch.zeros_like(sh[:, 0])
    dRdx, dRdy, dRdz = zero.clone(), zero.clone(), zero.clone()
    if deg > 0:
        dRdx, dRdy, dRdz = -SH_C1 * sh[:, 3], -SH_C1 * sh[:, 1], SH_C1 * sh[:, 2]
        if deg > 1:
            xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
            dRdx = dRdx + SH_C2[0] * y * sh[:, 4] + SH_C2[2] * 2.0 * -x * sh[:, 6] + SH_C2[3] * z * sh[:, 7] + SH_C2[4] * 2.0 * x * sh[:, 8]
            dRdy = dRdy + SH_C2[0] * x * sh[:, 4] + SH_C2[1] * z * sh[:, 5] + SH_C2[2] * 2.0 * -y * sh[:, 6] + SH_C2[4] * 2.0 * -y * sh[:, 8]
            dRdz = dRdz + SH_C2[1] * y * sh[:, 5] + SH_C2[2] * 2.0 * 2.0 * z * sh[:, 6] + SH_C2[3] * x * sh[:, 7]
            if deg > 2:
                dRdx = dRdx + (SH_C3[0] * sh[:, 9] * 3.0 * 2.0 * xy + SH_C3[1] * sh[:, 10] * yz + SH_C3[2] * sh[:, 11] * -2.0 * xy
                               + SH_C3[3] * sh[:, 12] * -3.0 * 2.0 * xz + SH_C3[4] * sh[:, 13] * (-3.0 * xx + 4.0 * zz - yy)
                               + SH_C3[5] * sh[:, 14] * 2.0 * xz + SH_C3[6] * sh[:, 15] * 3.0 * (xx - yy))
                dRdy = dRdy + (SH_C3[0] * sh[:, 9] * 3.0 * (xx - yy) + SH_C3[1] * sh[:, 10] * xz
                               + SH_C3[2] * sh[:, 11] * (-3.0 * yy + 4.0 * zz - xx) + SH_C3[3] * sh[:, 12] * -3.0 * 2.0 * yz
                               + SH_C3[4] * sh[:, 13] * -2.0 * xy + SH_C3[5] * sh[:, 14] * -2.0 * yz + SH_C3[6] * sh[:, 15] * -3.0 * 2.0 * xy)
                dRdz = dRdz + (SH_C3[1] * sh[:, 10] * xy + SH_C3[2] * sh[:, 11] * 4.0 * 2.0 * yz
                               + SH_C3[3] * sh[:, 12] * 3.0 * (2.0 * zz - xx - yy) + SH_C3[4] * sh[:, 13] * 4.0 * 2.0 * xz
                               + SH_C3[5] * sh[:, 14] * (xx - yy))
    ddx = (dRdx * dRGB).sum(1, keepdim=True)
    ddy = (dRdy * dRGB).sum(1, keepdim=True)
    ddz = (dRdz * dRGB).sum(1, keepdim=True)
    inv = 1.0 / (sum2 * sum2 * sum2).sqrt()
    gx = ((sum2 - ox * ox) * ddx - oy * ox * ddy - oz * ox * ddz) * inv
    gy = (-ox * oy * ddx + (sum2 - oy * oy) * ddy - oz * oy * ddz) * inv
    gz = (-ox * oz * ddx - oy * oz * ddy + (sum2 - oz * oz) * ddz) * inv
    return torch.cat([gx, gy, gz], 1)


def campos_grad_ref(deg, shs, xyz, campos, g_colors, live):
    """-> (dL/dcampos [3], sum_p |t[p]| [3]) in float64."""
    t = direction_terms(deg, shs, xyz, campos, g_colors, live)
    return -t.sum(0), t.abs().sum(0)


def campos_grad_autograd(deg, shs, xyz, campos, g_colors):
    """The same gradient from float64 autograd of oracle/torch_ref._sh_color -> (dL/dcampos [3], live [P,3])."""
    from oracle import torch_ref
    c = campos.detach().double().reshape(3).clone().requires_grad_(True)
    col = torch_ref._sh_color(deg, shs.detach().double(), xyz.detach().double(), c)
    loss = (col * g_colors.detach().double()).sum()
    if not loss.requires_grad:       # degree 0: the colours do not depend on the direction, and so not on campos
        return torch.zeros(3, dtype=torch.float64), col.detach() > 0
    (g,) = torch.autograd.grad(loss, c)
    return g, col.detach() > 0
