"""Sky colour model: EmerNeRF's sky head as the reference declares it (scene/background_model.py: SkyModel, MLP, get_directions,
Background_Model(model_type="mlp"); arguments/__init__.py:160-168 use_bg_model, bg_model_type, bg_model_lr) and wires to nothing.
The view direction of every pixel is encoded (33 sinusoidal values), goes through a 3-layer MLP of width 256 with the encoding
concatenated again in front of layer 1, and a sigmoid gives the sky colour, which is composited behind the Gaussians:

    image = render + (1 - A) * sky          render made over a ZERO background, A the accumulated opacity (sky.opacity_image)

SkyModel is the parameter container with the reference's names (so its checkpoints load); camera_intrinsics maps a camera to the
intrinsics the direction grid uses.  sky_composite / sky_image evaluate the model on the GPU (include/s3g_skymodel.h: one fused
forward kernel, a banded recompute backward), as ONE autograd node; GPU only, no CPU fallback.  Nothing is kept between calls: the
packed weight image and the workspace are tensors made in the call (the node holds the pack for its backward), the camera travels
as host doubles.  The arithmetic is restated in tests/skymodel_ref.py and pinned to the reference's own output by
tests/golden/skymodel.npz."""
from __future__ import annotations

import torch
from torch import nn

from . import _lib

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
    initialisation is nn.Linear's.  The module has no forward of its own: sky_image / sky_composite evaluate it."""

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
    along pixel (x, y)'s direction projects onto (x + 0.5, y + 0.5) in pixel units).  A dict that also carries "viewmatrix_host" (a
    CPU copy of viewmatrix) has the rotation taken from there: the sky model then reads nothing back from the device.  Or from the reference's own arguments instead:
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
    return cam.get("viewmatrix_host", cam["viewmatrix"])[:3, :3], W / (2.0 * cam["tanfovx"]), H / (2.0 * cam["tanfovy"]), W / 2.0, H / 2.0


def _gpu(t, name: str) -> None:
    if not (torch.is_tensor(t) and t.is_cuda):
        where = t.device if torch.is_tensor(t) else type(t).__name__
        raise RuntimeError(f"{name} must live on the GPU (got {where}); the sky model has no CPU fallback")


def _host_camera(cam):
    """A camera dict or (R, fx, fy, cx, cy) -> (_lib.SkyCamera of host doubles, (H, W) of a dict or None).  A rotation that lives
    on the device is read back here, once per call: a blocking copy, so the host waits for the work enqueued so far.  A camera dict
    with "viewmatrix_host" (camera_intrinsics) or a tuple with a CPU rotation avoids it."""
    size = None
    if isinstance(cam, dict):
        size = (int(cam["image_height"]), int(cam["image_width"]))
        cam = camera_intrinsics(cam)
    if not isinstance(cam, (tuple, list)) or len(cam) != 5:
        raise RuntimeError("the sky model's camera is a camera dict or (R_c2w [3,3], fx, fy, cx, cy)")
    R = torch.as_tensor(cam[0]).detach().to("cpu", torch.float64)
    if tuple(R.shape) != (3, 3):
        raise RuntimeError(f"R_c2w must have shape [3,3], got {tuple(R.shape)}")
    rec = _lib.SkyCamera()
    for i, v in enumerate(R.reshape(9).tolist()):
        rec.R[i] = v
    rec.fx, rec.fy, rec.cx, rec.cy = (float(v) for v in cam[1:])
    return rec, size


def plan(n_pixels: int, band_pixels=None) -> "_lib.SkyExtents":
    """s3g_skymodel_plan: tiles, bands, chunks and workspace bytes of an image of n_pixels (host only; nothing is launched)."""
    e = _lib.SkyExtents()
    _lib.check(_lib.lib().s3g_skymodel_plan(int(n_pixels), int(band_pixels or 0), e))
    return e


class _SkyComposite(torch.autograd.Function):
    """image = render + (1 - alpha) * sky(model, camera); render / alpha may be None (zero render, A = 0)."""

    @staticmethod
    def forward(ctx, camera, H, W, band_pixels, render, alpha, *weights):
        L = _lib.lib()
        dev = weights[0].device
        w = [t.detach().float().contiguous() for t in weights]
        r = None if render is None else render.detach().float().contiguous()
        a = None if alpha is None else alpha.detach().float().contiguous()
        pack = torch.empty(int(L.s3g_skymodel_pack_bytes()) // 4, dtype=torch.float32, device=dev)
        out = torch.empty((3, H, W), dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            stream = _lib.stream_ptr()
            _lib.check(L.s3g_sky_pack(*(t.data_ptr() for t in w), pack.data_ptr(), stream))
            _lib.check(L.s3g_sky_forward(H, W, camera, pack.data_ptr(), None if r is None else r.data_ptr(),
                                         None if a is None else a.data_ptr(), out.data_ptr(), stream))
        ctx.save_for_backward(pack, *(() if a is None else (a,)))
        ctx.camera, ctx.size, ctx.band_pixels = camera, (H, W), band_pixels
        ctx.alpha_shape = None if alpha is None else tuple(alpha.shape)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        pack, *rest = ctx.saved_tensors
        a = rest[0] if rest else None
        H, W = ctx.size
        need = ctx.needs_input_grad
        g = g.detach().float().contiguous()
        g_render = g if need[4] else None
        if not any(need[5:]):
            return (None, None, None, None, g_render, None) + (None,) * 6
        L = _lib.lib()
        dev = pack.device
        ext = plan(H * W, ctx.band_pixels)
        work = torch.empty(max(int(ext.workspace_bytes), 1), dtype=torch.uint8, device=dev)
        d_params = torch.empty(N_PARAMS, dtype=torch.float32, device=dev)
        g_alpha = torch.empty((H, W), dtype=torch.float32, device=dev) if (a is not None and need[5]) else None
        with _lib.on_device(dev):
            _lib.check(L.s3g_sky_backward(H, W, ctx.camera, pack.data_ptr(), None if a is None else a.data_ptr(), g.data_ptr(),
                                          int(ctx.band_pixels or 0), d_params.data_ptr(),
                                          None if g_alpha is None else g_alpha.data_ptr(), work.data_ptr(), _lib.stream_ptr()))
        grads, off = [], 0
        for shape in ((WIDTH, N_ENC), (WIDTH,), (WIDTH, WIDTH + N_ENC), (WIDTH,), (3, WIDTH), (3,)):
            n = 1
            for d in shape:
                n *= d
            grads.append(d_params[off:off + n].view(shape))
            off += n
        return (None, None, None, None, g_render, None if g_alpha is None else g_alpha.reshape(ctx.alpha_shape), *grads)


def sky_composite(model: SkyModel, cam, render, alpha, band_pixels=None) -> torch.Tensor:
    """render [3,H,W] + (1 - alpha) * sky, [3,H,W] fp32: the sky colour of every pixel composited behind a render made over a zero
    background.  One autograd node, differentiable w.r.t. the model's six parameters, `render` and `alpha`.
    cam: a camera dict (camera_intrinsics) or (R_c2w, fx, fy, cx, cy); converted to host doubles once.  alpha: [H,W] or [1,H,W], the
    accumulated opacity (out["alpha"] of render(return_alpha=True)).  Either of render / alpha may be None (zero render, A = 0).
    band_pixels: pixels per band of the backward (None: the library's default); it bounds the backward's workspace.
    GPU only.  Nothing is cached: the packed weights and the workspace are made in the call."""
    camera, size = _host_camera(cam)
    for t, name in ((render, "render"), (alpha, "alpha")):
        if t is not None:
            _gpu(t, name)
    weights = model.tensors()
    for t in weights:
        _gpu(t, "the sky model")
    if render is not None:
        if render.dim() != 3 or render.shape[0] != 3:
            raise RuntimeError(f"render must have shape [3,H,W], got {tuple(render.shape)}")
        hw = tuple(render.shape[-2:])
        if size is not None and size != hw:
            raise RuntimeError(f"render is {hw[0]} x {hw[1]}, the camera {size[0]} x {size[1]}")
        size = hw
    if size is None:
        raise RuntimeError("the sky model needs an image size: a camera dict, a render, or H= and W=")
    H, W = size
    if alpha is not None and alpha.numel() != H * W:
        raise RuntimeError(f"alpha {tuple(alpha.shape)} does not match the {H} x {W} image")
    dev = weights[0].device
    for t, name in ((render, "render"), (alpha, "alpha")):
        if t is not None and t.device != dev:
            raise RuntimeError(f"{name} lives on {t.device}, the sky model on {dev}")
    return _SkyComposite.apply(camera, H, W, band_pixels, render, alpha, *weights)


def sky_image(model: SkyModel, cam, H=None, W=None, band_pixels=None) -> torch.Tensor:
    """The sky colour of every pixel, [3,H,W] fp32: sky_composite with neither render nor alpha.  H, W: required with a camera
    tuple, taken from a camera dict otherwise."""
    for t in model.tensors():
        _gpu(t, "the sky model")
    if isinstance(cam, dict):
        if (H is not None and int(H) != int(cam["image_height"])) or (W is not None and int(W) != int(cam["image_width"])):
            raise RuntimeError("sky_image: H / W disagree with the camera dict")
        return sky_composite(model, cam, None, None, band_pixels)
    if H is None or W is None:
        raise RuntimeError("sky_image: a camera tuple needs H= and W=")
    camera, _ = _host_camera(cam)
    return _SkyComposite.apply(camera, int(H), int(W), band_pixels, None, None, *model.tensors())


def attached_group(optimizer, model: SkyModel):
    """The "sky_model" param group of `optimizer` that holds this model's parameters, or None."""
    if optimizer is None:
        return None
    ids = [id(t) for t in model.tensors()]
    for g in optimizer.param_groups:
        if g.get("name") == "sky_model" and [id(p) for p in g["params"]] == ids:
            return g
    return None
