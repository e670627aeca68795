"""Sky colour model, host side only: EmerNeRF's sky head as the reference declares it (scene/background_model.py:
SkyModel, MLP, get_directions, Background_Model(model_type="mlp"); arguments/__init__.py:160-168 use_bg_model, bg_model_type,
bg_model_lr) and wires to nothing.  The view direction of every pixel is encoded (33 sinusoidal values), goes through a 3-layer MLP
of width 256 with the encoding concatenated again in front of layer 1, and a sigmoid gives the sky colour, which is composited
behind the Gaussians:

    image = render + (1 - A) * sky          render made over a ZERO background, A the accumulated opacity (sky.opacity_image)

This module holds what needs no kernel: the parameter container with the reference's names (so its checkpoints load) and the
mapping from a camera to the intrinsics the direction grid uses.  The arithmetic is restated in tests/skymodel_ref.py and pinned to
the reference's own output by tests/golden/skymodel.npz.  There is no device route yet: nothing here evaluates the model."""
from __future__ import annotations

import torch
from torch import nn

WIDTH = 256
N_ENC = 33
N_PARAMS = WIDTH * N_ENC + WIDTH + WIDTH * (WIDTH + N_ENC) + WIDTH + 3 * WIDTH + 3   # 83 715


class _Encoding(nn.Module):
    """Holds the reference's `scales` buffer (SinusoidalEncoder(n_input_dims=3, min_deg=0, max_deg=4)), so that its state dicts load."""

    def __init__(self):
        super().__init__()
        self.register_buffer("scales", torch.tensor([2.0 ** i for i in range(5)]))


class _Head(nn.Module):
    def __init__(self):
        super().__init__()
        self.layers = nn.ModuleList([nn.Linear(N_ENC, WIDTH), nn.Linear(WIDTH + N_ENC, WIDTH), nn.Linear(WIDTH, 3)])


class SkyModel(nn.Module):
    """The reference's SkyModel(model_cfg={"mlp_width": 256}): parameter and buffer names are the reference's
    (direction_encoding.scales, sky_head.layers.{0,1,2}.{weight,bias}), so load_state_dict takes a reference state; default
    initialisation is nn.Linear's.  The module has no forward of its own."""

    def __init__(self, model_cfg: dict = None, model_type: str = "mlp", encoder: str = "sinusoidal"):
        super().__init__()
        cfg = {"mlp_width": WIDTH} if model_cfg is None else dict(model_cfg)
        if model_type != "mlp":
            raise NotImplementedError(f"model_type={model_type!r}: only the 'mlp' sky model is built (no shell or 'gs' model)")
        if encoder != "sinusoidal":
            raise NotImplementedError(f"encoder={encoder!r}: only the sinusoidal direction encoding (degrees 0..4) is built")
        width = cfg.get("mlp_width", cfg.get("head_mlp_layer_width", WIDTH))
        if width != WIDTH:
            raise NotImplementedError(f"mlp_width={width}: only the reference's mlp_width=256 is supported")
        self.model_cfg = cfg
        self.direction_encoding = _Encoding()
        self.sky_head = _Head()

    def tensors(self):
        """W0, b0, W1, b1, W2, b2."""
        out = []
        for layer in self.sky_head.layers:
            out += [layer.weight, layer.bias]
        return out

    @classmethod
    def from_state_dict(cls, sd) -> "SkyModel":
        """From a reference SkyModel state, or a Background_Model state (keys prefixed `sky_model.`)."""
        sd = {(k[len("sky_model."):] if k.startswith("sky_model.") else k): v for k, v in sd.items()}
        m = cls()
        m.load_state_dict(sd)
        return m


def camera_intrinsics(cam=None, c2w=None, intrinsic=None):
    """-> (R_c2w [3,3], fx, fy, cx, cy).  From a camera dict (viewmatrix = (world->camera)^T, tanfovx, tanfovy, image sizes):
    R_c2w = viewmatrix[:3,:3], fx = W / (2 tanfovx), cx = W / 2 and likewise for y, which are the rasterizer's pixel centres (a point
    along pixel (x, y)'s direction projects onto (x + 0.5, y + 0.5) in pixel units).  Or from the reference's own arguments instead:
    c2w [4,4] (or [3,4] / [3,3]: only the rotation is used; a leading camera axis of 1 is dropped) and intrinsic [3,3]."""
    if c2w is not None or intrinsic is not None:
        if c2w is None or intrinsic is None:
            raise RuntimeError("camera_intrinsics: c2w= and intrinsic= come together")
        if c2w.dim() == 3:
            c2w = c2w[0]
        if intrinsic.dim() == 3:
            intrinsic = intrinsic[0]
        if tuple(c2w.shape) not in ((4, 4), (3, 4), (3, 3)):
            raise RuntimeError(f"c2w must have shape [4,4], [3,4] or [3,3], got {tuple(c2w.shape)}")
        if tuple(intrinsic.shape) != (3, 3):
            raise RuntimeError(f"intrinsic must have shape [3,3], got {tuple(intrinsic.shape)}")
        return c2w[:3, :3], intrinsic[0, 0], intrinsic[1, 1], intrinsic[0, 2], intrinsic[1, 2]
    if cam is None:
        raise RuntimeError("camera_intrinsics: a camera dict, or c2w= and intrinsic=")
    W, H = int(cam["image_width"]), int(cam["image_height"])
    return cam["viewmatrix"][:3, :3], W / (2.0 * cam["tanfovx"]), H / (2.0 * cam["tanfovy"]), W / 2.0, H / 2.0
