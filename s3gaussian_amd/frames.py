"""Evaluation video frames on the MI355X: the uint8 strips the reference hands to its video writer
(utils/video_utils.py:439-499 save_seperate_videos: `to8b(np.concatenate(frames, axis=1))`, [H, num_cams * W, C], with each "depths"
frame divided by its own maximum first, utils/video_utils.py:196-198) written straight from the [C,H,W] fp32 renders of one camera by
one kernel family (include/s3g_frames.h).  pipeline.evaluate_video puts this behind one render per camera; the encoder stays with
the caller."""
from __future__ import annotations

import ctypes as C
from typing import Sequence, Tuple

import torch

from . import _lib

MAX_JOBS = 8         # S3G_FRAME_MAX_JOBS

calls = 0            # compose calls that reached the library (tests, tools/frames_ab.py)

_bound = False


class _Job(C.Structure):
    """struct s3g_frame_job (include/s3g_frames.h)."""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("dst_row_bytes", C.c_longlong), ("dst_col", C.c_int),
                ("channels", C.c_int), ("normalize", C.c_int), ("reserved", C.c_int)]


def _bind():
    global _bound
    L = _lib.lib()
    if not _bound:
        vp = C.c_void_p
        L.s3g_frame_workspace_bytes.restype = C.c_size_t
        L.s3g_frame_workspace_bytes.argtypes = [C.c_int, C.c_int, C.c_int]
        L.s3g_frame_tiles.restype = C.c_int
        L.s3g_frame_tiles.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(_Job), vp, vp, vp]
        _bound = True
    return L


def strip_shape(H: int, W: int, C: int, num_cams: int) -> Tuple[int, int, int]:
    """Shape of one timestamp's strip: num_cams images [H,W,C] side by side."""
    H, W, C, num_cams = int(H), int(W), int(C), int(num_cams)
    if H < 1 or W < 1 or C not in (1, 3) or num_cams < 1:
        raise ValueError(f"strip_shape: H = {H}, W = {W}, C = {C} (1 or 3), num_cams = {num_cams}")
    return (H, num_cams * W, C)


def _flags(normalize, n):
    if isinstance(normalize, (bool, int)):
        return [bool(normalize)] * n
    flags = [bool(f) for f in normalize]
    if len(flags) != n:
        raise RuntimeError("compose: one normalize flag per image")
    return flags


def compose(images, strip, cam: int, normalize=False, maxima=None):
    """Write camera `cam`'s tile of one or several strips: strip[k][:, cam * W:(cam + 1) * W, :] = to8b(images[k]) in [H,W,C] order,
    the bytes utils/visualization_tools.py::to8b gives for `images[k].permute(1, 2, 0)`; with normalize[k] the image is divided by its
    own maximum first (the reference's depth frames).  Every other byte of the strips is left alone.

    images: one [C,H,W] tensor or a sequence of up to 8, C = 1 or 3, all of one H x W, on the GPU, any strides and float dtype (made
    contiguous fp32 here).  strip: one contiguous uint8 [H, n * W, C] tensor per image on the same device (a single tensor for a single
    image), written in place.  normalize: one flag, or one per image.  maxima: a contiguous fp32 device tensor with one entry per
    image; entry k receives image k's maximum where normalize[k] is set.
    One library call for all images: two launches when some image is normalised, else one.  Nothing here waits for the device.
    Returns `strip`."""
    global calls
    single = torch.is_tensor(images)
    imgs = [images] if single else list(images)
    strips = [strip] if torch.is_tensor(strip) else list(strip)
    if not imgs or not all(torch.is_tensor(t) and t.is_cuda for t in imgs) or not all(torch.is_tensor(s) and s.is_cuda for s in strips):
        bad = next((t for t in imgs + strips if not (torch.is_tensor(t) and t.is_cuda)), None)
        where = bad.device if torch.is_tensor(bad) else type(bad).__name__
        raise RuntimeError(f"compose: images and strips must live on the GPU (got {where}); no CPU fallback")
    if len(imgs) > MAX_JOBS or len(strips) != len(imgs):
        raise RuntimeError(f"compose takes 1..{MAX_JOBS} images and one strip per image (got {len(imgs)} and {len(strips)})")
    flags = _flags(normalize, len(imgs))
    dev = imgs[0].device
    if imgs[0].dim() != 3:
        raise RuntimeError("compose expects images of shape [C,H,W]")
    H, W = int(imgs[0].shape[1]), int(imgs[0].shape[2])
    cam = int(cam)
    jobs = (_Job * len(imgs))()
    keep = []
    for k, (img, s) in enumerate(zip(imgs, strips)):
        if img.dim() != 3 or img.shape[0] not in (1, 3) or tuple(img.shape[1:]) != (H, W) or H < 1 or W < 1:
            raise RuntimeError(f"compose: image {k} has shape {tuple(img.shape)}; expected [1 or 3, {H}, {W}]")
        ch = int(img.shape[0])
        if not (s.device == dev and s.dtype == torch.uint8 and s.dim() == 3 and s.is_contiguous() and s.shape[0] == H
                and s.shape[2] == ch and s.shape[1] % W == 0 and 0 <= cam < s.shape[1] // W):
            raise RuntimeError(f"compose: strip {k} must be a contiguous uint8 [{H}, n * {W}, {ch}] tensor on the images' device "
                               f"with n > cam = {cam}")
        src = img.detach().to(dev).float().contiguous()
        keep.append(src)
        jobs[k].src, jobs[k].dst = src.data_ptr(), s.data_ptr()
        jobs[k].dst_row_bytes, jobs[k].dst_col = int(s.shape[1]) * ch, cam * W
        jobs[k].channels, jobs[k].normalize, jobs[k].reserved = ch, int(flags[k]), 0
    if maxima is not None and not (torch.is_tensor(maxima) and maxima.is_cuda and maxima.device == dev and maxima.dtype == torch.float32
                                   and maxima.numel() == len(imgs) and maxima.is_contiguous()):
        raise RuntimeError("compose: maxima must be a contiguous fp32 tensor with one entry per image on the images' device")
    L = _bind()
    work = None
    if any(flags):
        work = torch.empty(max(int(L.s3g_frame_workspace_bytes(H, W, len(imgs))), 1), dtype=torch.uint8, device=dev)
    with _lib.on_device(dev):
        _lib.check(L.s3g_frame_tiles(H, W, len(imgs), jobs, None if maxima is None else maxima.data_ptr(),
                                     None if work is None else work.data_ptr(), _lib.stream_ptr()))
    calls += 1
    return strip


def to8b(image: torch.Tensor, normalize: bool = False) -> torch.Tensor:
    """[H,W,C] uint8 of one [C,H,W] device image: utils/visualization_tools.py::to8b(image.permute(1, 2, 0)) without the host."""
    if not (torch.is_tensor(image) and image.is_cuda):
        where = image.device if torch.is_tensor(image) else type(image).__name__
        raise RuntimeError(f"to8b: the image must live on the GPU (got {where}); no CPU fallback")
    if image.dim() != 3 or image.shape[0] not in (1, 3):
        raise RuntimeError("to8b expects an image of shape [C,H,W] with C = 1 or 3")
    ch, H, W = image.shape
    out = torch.empty(strip_shape(H, W, ch, 1), dtype=torch.uint8, device=image.device)
    return compose(image, out, 0, normalize=normalize)
