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

import torch

from . import lpips as _base
from .lpips import RECORD, TAP0, TOTAL          # S3G_LPIPS_* (include/s3g_lpips.h): the record is the AlexNet variant's

MIN_SIZE = 16

FEATURE_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)     # torchvision's vgg16.features: the thirteen Conv2d modules
CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
            (512, 512), (512, 512), (512, 512))
CONV_SHAPES = tuple((co, ci, 3, 3) for ci, co in CHANNELS)
TAP_CONVS = (1, 3, 6, 9, 12)                # conv1_2, conv2_2, conv3_3, conv4_3, conv5_3: tapped after their ReLU, before the pool
TAP_CHANNELS = tuple(CHANNELS[c][1] for c in TAP_CONVS)

VGG = _base.Variant("s3g_lpips_vgg", "lpips_vgg", "LPIPSVGG", "VGG16", FEATURE_INDEX, CONV_SHAPES, TAP_CONVS)


def _bind():
    return _base._bind_variant(VGG)


def collect_weights(vgg_sd, lin_sd):
    """-> (conv_w, conv_b, lin_w): lists of thirteen, thirteen and five fp32 tensors, shapes checked.
    vgg_sd: torchvision's keys features.{0,2,5,...,28}.{weight,bias}; other keys (the classifier) are ignored.
    lin_sd: lin{i}.model.1.weight (upstream) or {i}.1.weight (as the reference renames them), each [1,C,1,1]."""
    return _base._collect(VGG, vgg_sd, lin_sd)


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
        return cls(_base._pack(VGG, vgg_sd, lin_sd, device))

    @classmethod
    def from_files(cls, vgg16_path, lin_path, device):
        return cls.from_state_dicts(_base._load(vgg16_path), _base._load(lin_path), device)


def lpips_vgg(model: LPIPSVGG, image: torch.Tensor, gt: torch.Tensor, out=None):
    """{total, tap0..tap4} of one frame pair as a float64 device tensor of 6 entries; total is the reference's
    lpips(image, gt, net_type='vgg').

    image, gt: [3,H,W] on the model's GPU, any strides (a permuted [H,W,3] view is fine), H, W >= 16; used as they are, in [0,1].
    out: a contiguous float64 tensor of 6 entries on the same device -- one row of an [N,6] tensor -- written in place and returned.
    Nothing here waits for the device."""
    return _base._call(VGG, LPIPSVGG, model, image, gt, out)
