"""Evaluation LPIPS on the MI355X: what the reference's evaluation loop reports per frame with `lpips(rgb, gt, net_type='alex')`
(utils/video_utils.py:210-241 over lpipsPyTorch/) -- the AlexNet feature stack on the fp32 matrix pipe, the per-pixel normalisation
and the weighted mean per tap, without building a network, loading a file or waiting for the device per frame
(include/s3g_lpips.h).

The arithmetic does not depend on the weights it is given, and no weights ship with this package: the caller names the two files
every user of the reference already has in the torch hub cache,

    model = LPIPS.from_files("~/.cache/torch/hub/checkpoints/alexnet-owt-7be5be79.pth",     # torchvision's AlexNet
                             "~/.cache/torch/hub/checkpoints/alex.pth", "cuda:0")            # the LPIPS v0.1 lin layers
    record = lpips(model, image, gt)                                                        # [6] float64 on the device

Nothing is downloaded and nothing is searched for.  Equality with published LPIPS values rests on those weights."""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple, Tuple

import torch

from . import _lib

TOTAL, TAP0 = 0, 1          # S3G_LPIPS_* (include/s3g_lpips.h)
RECORD = 6                  # {total, tap0..tap4}
MIN_SIZE = 31

FEATURE_INDEX = (0, 3, 6, 8, 10)            # torchvision's alexnet.features: the five Conv2d modules
CONV_SHAPES = ((64, 3, 11, 11), (192, 64, 5, 5), (384, 192, 3, 3), (256, 384, 3, 3), (256, 256, 3, 3))


class Variant(NamedTuple):
    """What tells one feature stack from the other on this side of the C ABI; s3gaussian_amd.lpips_vgg holds the VGG16 one."""
    prefix: str                             # the C symbols are {prefix}, {prefix}_weights_bytes, _pack_weights, _workspace_bytes
    fn: str                                 # the Python function, as messages name it
    model: str                              # the model class, as messages name it
    net: str                                # the network, as messages name it
    feature_index: Tuple[int, ...]          # torchvision's features.{f} of every conv
    conv_shapes: Tuple[Tuple[int, ...], ...]
    tap_convs: Tuple[int, ...]              # the convs tapped after their ReLU, one lin layer each


ALEX = Variant("s3g_lpips", "lpips", "LPIPS", "AlexNet", FEATURE_INDEX, CONV_SHAPES, (0, 1, 2, 3, 4))

_BOUND = {}


def _bind_variant(v: Variant):
    if v.prefix not in _BOUND:
        L = _lib.lib()
        if not hasattr(L, v.prefix):
            raise ImportError(f"{_lib.LIB_PATH} has no {v.prefix}: it was built from an older tree: rebuild")
        vp, i = C.c_void_p, C.c_int
        for name, restype, argtypes in (("_weights_bytes", C.c_size_t, []),
                                        ("_pack_weights", i, [C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp, vp]),
                                        ("_workspace_bytes", C.c_size_t, [i, i]),
                                        ("", i, [i, i, vp, vp, vp, vp, vp, vp])):
            f = getattr(L, v.prefix + name)
            f.restype, f.argtypes = restype, argtypes
        _BOUND[v.prefix] = L
    return _BOUND[v.prefix]


def _collect(v: Variant, net_sd, lin_sd):
    conv_w, conv_b, lin_w = [], [], []
    for f, shape in zip(v.feature_index, v.conv_shapes):
        for name in (f"features.{f}.weight", f"features.{f}.bias"):
            if name not in net_sd:
                raise KeyError(f"LPIPS: the {v.net} state dict has no '{name}'")
        w, b = net_sd[f"features.{f}.weight"], net_sd[f"features.{f}.bias"]
        if tuple(w.shape) != shape or tuple(b.shape) != shape[:1]:
            raise RuntimeError(f"LPIPS: features.{f} has weight {tuple(w.shape)} and bias {tuple(b.shape)}, expected {shape} and "
                               f"{shape[:1]}")
        conv_w.append(w.detach().float())
        conv_b.append(b.detach().float())
    for i, conv in enumerate(v.tap_convs):
        c = v.conv_shapes[conv][0]
        names = (f"lin{i}.model.1.weight", f"{i}.1.weight")
        found = [n for n in names if n in lin_sd]
        if len(found) != 1:
            raise KeyError(f"LPIPS: the lin state dict must hold exactly one of {names}")
        lw = lin_sd[found[0]]
        if tuple(lw.shape) != (1, c, 1, 1):
            raise RuntimeError(f"LPIPS: {found[0]} has shape {tuple(lw.shape)}, expected {(1, c, 1, 1)}")
        lin_w.append(lw.detach().float().reshape(-1))
    return conv_w, conv_b, lin_w


def _pack(v: Variant, net_sd, lin_sd, device) -> torch.Tensor:
    """The state dicts' weights as the variant's blob on `device`."""
    groups = _collect(v, net_sd, lin_sd)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"LPIPS: the weights are packed on the GPU (got {dev}); no CPU fallback")
    L = _bind_variant(v)
    groups = [[t.to(dev).contiguous() for t in g] for g in groups]
    arrays = [(C.c_void_p * len(g))(*[t.data_ptr() for t in g]) for g in groups]
    packed = torch.empty(int(getattr(L, v.prefix + "_weights_bytes")()), dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):             # the device copies and the pack share the current stream: `groups` may go after it
        _lib.check(getattr(L, v.prefix + "_pack_weights")(arrays[0], arrays[1], arrays[2], packed.data_ptr(), _lib.stream_ptr()))
    return packed


def _load(path):
    return torch.load(os.path.expanduser(os.fspath(path)), weights_only=True, map_location="cpu")


def _call(v: Variant, cls, model, image, gt, out):
    if not isinstance(model, cls):
        raise TypeError(f"{v.fn}: the first argument is an {v.model} model ({v.model}.from_files / {v.model}.from_state_dicts)")
    if not (torch.is_tensor(image) and image.is_cuda and torch.is_tensor(gt) and gt.is_cuda):
        where = image.device if torch.is_tensor(image) else type(image).__name__
        raise RuntimeError(f"{v.fn}: images must live on the GPU (got {where}); no CPU fallback")
    if image.dim() != 3 or image.shape[0] != 3 or gt.shape != image.shape:
        raise RuntimeError(f"{v.fn} expects image and gt of shape [3,H,W]")
    dev = image.device
    if model.device != dev:
        raise RuntimeError(f"{v.fn}: the model lives on {model.device}, the images on {dev}")
    L = _bind_variant(v)
    img, ref = image.detach().float().contiguous(), gt.detach().to(dev).float().contiguous()
    _, H, W = img.shape
    if out is None:
        out = torch.empty(RECORD, dtype=torch.float64, device=dev)
    elif not (out.is_cuda and out.device == dev and out.dtype == torch.float64 and out.numel() == RECORD and out.is_contiguous()):
        raise RuntimeError(f"{v.fn}: out must be a contiguous float64 tensor of 6 entries on the images' device")
    work = torch.empty(max(int(getattr(L, v.prefix + "_workspace_bytes")(H, W)), 1), dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        _lib.check(getattr(L, v.prefix)(H, W, img.data_ptr(), ref.data_ptr(), model.packed.data_ptr(), out.data_ptr(), work.data_ptr(),
                                        _lib.stream_ptr()))
    return out


def _bind():
    return _bind_variant(ALEX)


def _check_net_type(net_type):
    if net_type != "alex":
        hint = "; the VGG16 variant is s3gaussian_amd.lpips_vgg (LPIPSVGG, lpips_vgg)" if net_type == "vgg" else ""
        raise NotImplementedError(f"lpips: net_type '{net_type}' is not built here; only 'alex', the variant the evaluation loop "
                                  f"uses{hint}")


def collect_weights(alexnet_sd, lin_sd):
    """-> (conv_w, conv_b, lin_w): three lists of five fp32 CPU-or-wherever tensors, shapes checked.
    alexnet_sd: torchvision's keys features.{0,3,6,8,10}.{weight,bias}; other keys (the classifier) are ignored.
    lin_sd: lin{i}.model.1.weight (upstream) or {i}.1.weight (as the reference renames them), each [1,C,1,1]."""
    return _collect(ALEX, alexnet_sd, lin_sd)


class LPIPS:
    """The packed weights of the AlexNet LPIPS on one GPU: the conv kernel's B operands, the biases and the lin weights in one blob
    (s3g_lpips_pack_weights), and nothing else."""

    def __init__(self, packed: torch.Tensor, net_type: str = "alex"):
        _check_net_type(net_type)
        self.packed = packed
        self.net_type = net_type

    @property
    def device(self):
        return self.packed.device

    @classmethod
    def from_state_dicts(cls, alexnet_sd, lin_sd, device, net_type: str = "alex"):
        _check_net_type(net_type)
        return cls(_pack(ALEX, alexnet_sd, lin_sd, device), net_type)

    @classmethod
    def from_files(cls, alexnet_path, lin_path, device, net_type: str = "alex"):
        _check_net_type(net_type)
        return cls.from_state_dicts(_load(alexnet_path), _load(lin_path), device, net_type)


def lpips(model: LPIPS, image: torch.Tensor, gt: torch.Tensor, out=None, net_type: str = "alex"):
    """{total, tap0..tap4} of one frame pair as a float64 device tensor of 6 entries; total is the reference's lpips(image, gt).

    image, gt: [3,H,W] on the model's GPU, any strides (a permuted [H,W,3] view is fine), H, W >= 31; used as they are, in [0,1].
    out: a contiguous float64 tensor of 6 entries on the same device -- one row of an [N,6] tensor -- written in place and returned.
    Nothing here waits for the device."""
    _check_net_type(net_type)
    return _call(ALEX, LPIPS, model, image, gt, out)
