"""Torch restatement of the sky colour model (s3gaussian_amd/skymodel.py), dtype-generic: the float64 run is the tests' reference
(pinned to the reference implementation's own output by tests/golden/skymodel.npz), the float32 run on CPU is the yardstick the
project's 4 x rule measures the kernels against."""
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "skymodel.npz")
NAMES = ("sky_head.layers.0.weight", "sky_head.layers.0.bias", "sky_head.layers.1.weight", "sky_head.layers.1.bias",
         "sky_head.layers.2.weight", "sky_head.layers.2.bias")


def load_golden():
    return np.load(GOLDEN)


def golden_weights(z, dtype=torch.float64):
    """W0, b0, W1, b1, W2, b2 of the fixture."""
    return [torch.from_numpy(z["w." + n]).to(dtype) for n in NAMES]


def golden_camera(z, i):
    H, W = (int(v) for v in z[f"cam{i}.size"])
    return torch.from_numpy(z[f"cam{i}.c2w"]), torch.from_numpy(z[f"cam{i}.intrinsic"]), H, W


def directions(R, fx, fy, cx, cy, H, W, dtype):
    """[H*W,3] unit view directions; R [3,3] camera-to-world rotation."""
    R = torch.as_tensor(R).to(dtype)
    fx, fy, cx, cy = (torch.as_tensor(v).to(dtype) for v in (fx, fy, cx, cy))
    x = torch.arange(W).to(dtype).repeat(H)
    y = torch.arange(H).to(dtype).repeat_interleave(W)
    d_cam = torch.stack([(x - cx + 0.5) / fx, (y - cy + 0.5) / fy, torch.ones_like(x)], dim=-1)
    d = (d_cam[:, None, :] * R[None]).sum(-1)
    return d / (torch.linalg.norm(d, dim=-1, keepdim=True) + 1e-8)


def encode(v):
    scales = torch.tensor([1.0, 2.0, 4.0, 8.0, 16.0], dtype=v.dtype)
    xb = (v[:, None, :] * scales[:, None]).reshape(v.shape[0], 15)           # scale-major
    return torch.cat([v, torch.sin(torch.cat([xb, xb + 0.5 * math.pi], dim=-1))], dim=-1)


def sky_colors(weights, v):
    """[N,3] sigmoid(MLP(encode(v))); weights = W0, b0, W1, b1, W2, b2 (may require grad)."""
    W0, b0, W1, b1, W2, b2 = weights
    e = encode(v)
    h0 = torch.relu(e @ W0.T + b0)
    h1 = torch.relu(torch.cat([h0, e], dim=-1) @ W1.T + b1)
    return torch.sigmoid(h1 @ W2.T + b2)


def sky_image(weights, R, fx, fy, cx, cy, H, W):
    dtype = weights[0].dtype
    return sky_colors(weights, directions(R, fx, fy, cx, cy, H, W, dtype)).T.reshape(3, H, W)


def composite(weights, R, fx, fy, cx, cy, render, alpha):
    """render [3,H,W] + (1 - alpha [H,W]) * sky."""
    H, W = render.shape[-2:]
    return render + (1.0 - alpha.reshape(1, H, W)) * sky_image(weights, R, fx, fy, cx, cy, H, W)


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))
