"""Evaluation LPIPS, VGG16 variant, on the MI355X: what the reference's metrics.py reports with `lpips(render, gt, net_type='vgg')`
(metrics.py:74 over lpipsPyTorch/) -- the thirteen 3x3 convolutions of torchvision's VGG16 on the fp32 matrix pipe, the per-pixel
normalisation and the weighted mean per tap, without building a network, loading a file or waiting for the device per frame
(include/s3g_lpips_vgg.h).  The AlexNet variant the evaluation loop uses is s3gaussian_amd.lpips.

The arithmetic does not depend on the weights it is given, and no weights ship with this package: the caller names the two files
every user of the reference already has in the torch hub cache,

    model = LPIPSVGG.from_files("~/.cache/torch/hub/checkpoints/vgg16-397923af.pth",         # torchvision's VGG16
                                "~/.cache/torch/hub/checkpoints/vgg.pth", "cuda:0")           # the LPIPS v0.1 lin layers
    record = lpips_vgg(model, image, gt)                                                     # [6] float64 on the device

Nothing is downloaded and nothing is searched for.  Equality with published LPIPS values rests on those weights."""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _lib

TOTAL, TAP0 = 0, 1          # S3G_LPIPS_* (include/s3g_lpips.h): the record is the AlexNet variant's
RECORD = 6                  # {total, tap0..tap4}
MIN_SIZE = 16

FEATURE_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)     # torchvision's vgg16.features: the thirteen Conv2d modules
CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
            (512, 512), (512, 512), (512, 512))
CONV_SHAPES = tuple((co, ci, 3, 3) for ci, co in CHANNELS)
TAP_CONVS = (1, 3, 6, 9, 12)                # conv1_2, conv2_2, conv3_3, conv4_3, conv5_3: tapped after their ReLU, before the pool
TAP_CHANNELS = tuple(CHANNELS[c][1] for c in TAP_CONVS)

_L = None


def _bind():
    global _L
    if _L is None:
        L = _lib.lib()
        if not hasattr(L, "s3g_lpips_vgg"):
            raise ImportError(f"{_lib.LIB_PATH} has no s3g_lpips_vgg: it was built from an older tree: rebuild")
        vp, i = C.c_void_p, C.c_int
        L.s3g_lpips_vgg_weights_bytes.restype = C.c_size_t
        L.s3g_lpips_vgg_weights_bytes.argtypes = []
        L.s3g_lpips_vgg_pack_weights.restype = i
        L.s3g_lpips_vgg_pack_weights.argtypes = [C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp, vp]
        L.s3g_lpips_vgg_workspace_bytes.restype = C.c_size_t
        L.s3g_lpips_vgg_workspace_bytes.argtypes = [i, i]
        L.s3g_lpips_vgg.restype = i
        L.s3g_lpips_vgg.argtypes = [i, i, vp, vp, vp, vp, vp, vp]
        _L = L
    return _L


def collect_weights(vgg_sd, lin_sd):
    """-> (conv_w, conv_b, lin_w): lists of thirteen, thirteen and five fp32 tensors, shapes checked.
    vgg_sd: torchvision's keys features.{0,2,5,...,28}.{weight,bias}; other keys (the classifier) are ignored.
    lin_sd: lin{i}.model.1.weight (upstream) or {i}.1.weight (as the reference renames them), each [1,C,1,1]."""
    conv_w, conv_b, lin_w = [], [], []
    for f, shape in zip(FEATURE_INDEX, CONV_SHAPES):
        for name in (f"features.{f}.weight", f"features.{f}.bias"):
            if name not in vgg_sd:
                raise KeyError(f"LPIPS: the VGG16 state dict has no '{name}'")
        w, b = vgg_sd[f"features.{f}.weight"], vgg_sd[f"features.{f}.bias"]
        if tuple(w.shape) != shape or tuple(b.shape) != shape[:1]:
            raise RuntimeError(f"LPIPS: features.{f} has weight {tuple(w.shape)} and bias {tuple(b.shape)}, expected {shape} and "
                               f"{shape[:1]}")
        conv_w.append(w.detach().float())
        conv_b.append(b.detach().float())
    for i, c in enumerate(TAP_CHANNELS):
        names = (f"lin{i}.model.1.weight", f"{i}.1.weight")
        found = [n for n in names if n in lin_sd]
        if len(found) != 1:
            raise KeyError(f"LPIPS: the lin state dict must hold exactly one of {names}")
        lw = lin_sd[found[0]]
        if tuple(lw.shape) != (1, c, 1, 1):
            raise RuntimeError(f"LPIPS: {found[0]} has shape {tuple(lw.shape)}, expected {(1, c, 1, 1)}")
        lin_w.append(lw.detach().float().reshape(-1))
    return conv_w, conv_b, lin_w


class LPIPSVGG:
    """The packed weights of the VGG16 LPIPS on one GPU: the conv kernel's B operands, the biases and the lin weights in one blob
    (s3g_lpips_vgg_pack_weights, about 59 MB), and nothing else."""

    net_type = "vgg"

    def __init__(self, packed: torch.Tensor):
        self.packed = packed

    @property
    def device(self):
        return self.packed.device

    @classmethod
    def from_state_dicts(cls, vgg_sd, lin_sd, device):
        conv_w, conv_b, lin_w = collect_weights(vgg_sd, lin_sd)
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"LPIPS: the weights are packed on the GPU (got {dev}); no CPU fallback")
        L = _bind()
        groups = [[t.to(dev).contiguous() for t in g] for g in (conv_w, conv_b, lin_w)]
        arrays = [(C.c_void_p * len(g))(*[t.data_ptr() for t in g]) for g in groups]
        packed = torch.empty(int(L.s3g_lpips_vgg_weights_bytes()), dtype=torch.uint8, device=dev)
        with _lib.on_device(dev):             # the device copies and the pack share the current stream: `groups` may go after it
            _lib.check(L.s3g_lpips_vgg_pack_weights(arrays[0], arrays[1], arrays[2], packed.data_ptr(), _lib.stream_ptr()))
        return cls(packed)

    @classmethod
    def from_files(cls, vgg16_path, lin_path, device):
        load = lambda p: torch.load(os.path.expanduser(os.fspath(p)), weights_only=True, map_location="cpu")
        return cls.from_state_dicts(load(vgg16_path), load(lin_path), device)


def lpips_vgg(model: LPIPSVGG, image: torch.Tensor, gt: torch.Tensor, out=None):
    """{total, tap0..tap4} of one frame pair as a float64 device tensor of 6 entries; total is the reference's
    lpips(image, gt, net_type='vgg').

    image, gt: [3,H,W] on the model's GPU, any strides (a permuted [H,W,3] view is fine), H, W >= 16; used as they are, in [0,1].
    out: a contiguous float64 tensor of 6 entries on the same device -- one row of an [N,6] tensor -- written in place and returned.
    Nothing here waits for the device."""
    if not isinstance(model, LPIPSVGG):
        raise TypeError("lpips_vgg: the first argument is an LPIPSVGG model (LPIPSVGG.from_files / LPIPSVGG.from_state_dicts)")
    if not (torch.is_tensor(image) and image.is_cuda and torch.is_tensor(gt) and gt.is_cuda):
        where = image.device if torch.is_tensor(image) else type(image).__name__
        raise RuntimeError(f"lpips_vgg: images must live on the GPU (got {where}); no CPU fallback")
    if image.dim() != 3 or image.shape[0] != 3 or gt.shape != image.shape:
        raise RuntimeError("lpips_vgg expects image and gt of shape [3,H,W]")
    dev = image.device
    if model.device != dev:
        raise RuntimeError(f"lpips_vgg: the model lives on {model.device}, the images on {dev}")
    L = _bind()
    img, ref = image.detach().float().contiguous(), gt.detach().to(dev).float().contiguous()
    _, H, W = img.shape
    if out is None:
        out = torch.empty(RECORD, dtype=torch.float64, device=dev)
    elif not (out.is_cuda and out.device == dev and out.dtype == torch.float64 and out.numel() == RECORD and out.is_contiguous()):
        raise RuntimeError("lpips_vgg: out must be a contiguous float64 tensor of 6 entries on the images' device")
    work = torch.empty(max(int(L.s3g_lpips_vgg_workspace_bytes(H, W)), 1), dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        _lib.check(L.s3g_lpips_vgg(H, W, img.data_ptr(), ref.data_ptr(), model.packed.data_ptr(), out.data_ptr(), work.data_ptr(),
                                   _lib.stream_ptr()))
    return out
