"""Bit-level checksums of the image-space loss stack (s3gaussian_amd.losses) -- one JSON line, so that two trees can be compared bit
for bit across processes (a refactor of that stack must print the same line):  python tools/loss_checksum.py
Only public functions of the module, so the same file runs on an older tree.  Per case: the int32 bit-sum (tools/step_checksum.py's
`bits`) of the value and of every gradient, None where there is none.  Inputs are the seeded batch of
tests/test_photometric_views_gpu.py at 45 x 70: ragged against the SSIM kernels' 64 x 21 strips, three strip workgroups, each adding
into an accumulator slot of its own, so the double sums have one order and the values are reproducible too."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from s3gaussian_amd import losses  # noqa: E402
from tests.test_photometric_views_gpu import V, _batch  # noqa: E402

W_SSIM, W_DEPTH, W_FEAT, SEED_GRAD = 0.2, 0.5, 0.001, 2.5
dev = torch.device("cuda", 0)
IMG, GT, DEP, GDEP, FT, GFT = (t.to(dev) for t in _batch())


def bits(t):
    if t is None:
        return None
    t = t.detach().contiguous()
    t = t.float() if t.dtype in (torch.bool, torch.float64) else t
    return int(t.view(torch.int32).to(torch.int64).sum())


def run(fn, *leaves):
    """fn(*leaves) -> scalar, back-propagated with a seed that is not 1; a leaf is a tensor, None, or a list of those."""
    leaf = lambda t: None if t is None else t.clone().requires_grad_(True)
    ls = [[leaf(t) for t in l] if isinstance(l, list) else leaf(l) for l in leaves]
    v = fn(*ls)
    (SEED_GRAD * v).backward()
    grad = lambda t: None if t is None else bits(t.grad)
    return {"value": bits(v.reshape(1)), "grads": [[grad(t) for t in l] if isinstance(l, list) else grad(l) for l in ls]}


def single(depth=True, feat=True, **weights):
    kw = dict(dict(lambda_dssim=W_SSIM, lambda_depth=W_DEPTH, lambda_feat=W_FEAT), **weights)
    f = lambda i, d, t: losses.photometric_loss(i, GT[0], d, None if d is None else GDEP[0], t, None if t is None else GFT[0], **kw)
    return run(f, IMG[0], DEP[0] if depth else None, FT[0] if feat else None)


def views(order, feat_views, **weights):
    kw = dict(dict(lambda_dssim=W_SSIM, lambda_depth=W_DEPTH, lambda_feat=W_FEAT), **weights)
    f = lambda i, d, t: losses.photometric_loss_views(i, [GT[v] for v in order], d, [GDEP[v] for v in order], t,
                                                      [GFT[v] if v in feat_views else None for v in order], **kw)
    return run(f, [IMG[v] for v in order], [DEP[v] for v in order], [FT[v] if v in feat_views else None for v in order])


def planes():
    g = torch.Generator().manual_seed(7)
    sizes = [(2, 3), (5, 2), (3, 5), (17, 4), (4, 33), (9, 9)]   # (h, w) per plane: rows over one PR_ROWS = 16 block, columns over 256
    return [[torch.randn(1, 32, (lv + 1) * h, (lv + 1) * w, generator=g).to(dev).contiguous(memory_format=torch.channels_last)
             for h, w in sizes] for lv in range(2)]


def regulation():
    weights = (0.01, 0.0001, 0.0002)
    grids = [[p.clone().requires_grad_(True) for p in level] for level in planes()]
    v = losses.plane_regulation(grids, *weights)
    (SEED_GRAD * v).backward()
    flat = [p for level in planes() for p in level]
    out = [torch.empty_like(p) for p in flat]
    vi = losses.plane_regulation_into(flat, weights, out)
    return {"plane_regulation": {"value": bits(v.reshape(1)), "grads": [bits(p.grad) for level in grids for p in level]},
            "plane_regulation_into": {"value": bits(vi.reshape(1)), "grads": [bits(t) for t in out]}}


rig = tuple(range(V))
out = {
    "ssim": run(lambda i: losses.ssim(i[None], GT[0][None]), IMG[0]),
    "photometric_all": single(),
    "photometric_no_depth_pair": single(depth=False),
    "photometric_no_feat_pair": single(feat=False),
    "photometric_zero_depth_weight": single(lambda_depth=0.0),
    "photometric_no_ssim": single(lambda_dssim=0.0),
    "photometric_l1_only": single(lambda_dssim=0.0, lambda_depth=0.0, lambda_feat=0.0),
    # the three calls of s3gaussian_amd.patch, one term each
    "pixel_terms_l1": run(lambda i: losses.pixel_terms(image=i, gt_image=GT[0], w_l1=1.0), IMG[0]),
    "pixel_terms_feat": run(lambda t: losses.pixel_terms(feat=t, gt_feat=GFT[0], w_feat=1.0), FT[0]),
    "pixel_terms_depth": run(lambda d: losses.pixel_terms(depth=d, gt_depth=GDEP[0], w_depth=1.0, max_depth=80.0), DEP[0]),
    "pixel_terms_all": run(lambda i, d, t: losses.pixel_terms(i, GT[0], d, GDEP[0], t, GFT[0], w_l1=1.0, w_depth=W_DEPTH, w_feat=W_FEAT),
                           IMG[0], DEP[0], FT[0]),
    "views_feat_last": views(rig, (V - 1,)),
    "views_feat_all": views(rig, rig),
    "views_feat_none": views(rig, ()),
    "views_no_ssim": views(rig, (V - 1,), lambda_dssim=0.0),
    "views_empty_depth_view_first": views((2, 0, 1), (1,)),      # view 2 of the batch has no valid depth pixel
    "views_one": views((0,), (0,)),
    **regulation(),
}
print(json.dumps(out, sort_keys=True))
