"""Generate tests/golden/lpips_vgg.npz: images and the reference's own VGG LPIPS values for s3gaussian_amd/lpips_vgg.py.

    python tests/golden/make_golden_lpips_vgg.py        # rewrites lpips_vgg.npz next to this file

Runs in the build container only: the recorded values come from the REFERENCE'S OWN lpipsPyTorch package (imported from the reference
tree, never copied).  The pretrained weights exist on no machine this runs on, so `torchvision.models.vgg16` is replaced by a stub
whose `.features` is the 31-module stack of torchvision's VGG16 holding lpips_vgg_ref.synthetic_weights(seed) (the stub also provides
`VGG16_Weights.IMAGENET1K_V1`, which networks.py:92 names), and `torch.hub.load_state_dict_from_url` is patched to return the
synthetic lin weights under the upstream key names (the reference renames them itself, lpipsPyTorch/modules/utils.py:22-28).  Without
the reference tree this script refuses to run.

Per size s{H}x{W} of lpips_vgg_ref.FIXTURE_SIZES: seed (weights), image_seed, weight_sums (float64 sum of every weight tensor), x, y
[3,H,W] fp32, ref_f32 (the reference's lpips(x, y, net_type='vgg') as called by metrics.py), ref_f64 (the same module after .double()
on double inputs), ref_taps_f64 (the five entries of LPIPS.forward's `res`, in double, read with forward hooks on its lin layers).
The script asserts lpips_vgg_ref.check_inputs on every case (and on the GPU test's extra size), and that the float64 restatement
reproduces the reference at 1e-12."""
import importlib
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

REF = os.environ.get("S3G_REFERENCE", "/root/reference")
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import lpips_vgg_ref as lv  # noqa: E402


def vgg16_features(weights):
    """torchvision's VGG16 `features`, restated from its public definition (configuration D), holding the synthetic weights."""
    layers = []
    for l, (ci, co) in enumerate(lv.CHANNELS):
        conv = nn.Conv2d(ci, co, kernel_size=3, padding=1)
        with torch.no_grad():
            conv.weight.copy_(torch.from_numpy(weights["conv_w"][l]))
            conv.bias.copy_(torch.from_numpy(weights["conv_b"][l]))
        layers += [conv, nn.ReLU(inplace=True)]
        if l in lv.TAP_CONVS:
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
    assert len(layers) == 31 and [i for i, m in enumerate(layers) if isinstance(m, nn.Conv2d)] == list(lv.FEATURE_INDEX)
    return nn.Sequential(*layers)


def reference_package(weights):
    if not os.path.isfile(os.path.join(REF, "lpipsPyTorch", "__init__.py")):
        raise SystemExit(f"{REF}/lpipsPyTorch is missing: the fixture records the reference's own values and cannot be written "
                         "without it")
    tv, models = types.ModuleType("torchvision"), types.ModuleType("torchvision.models")
    tv.__path__ = []
    models.VGG16_Weights = types.SimpleNamespace(IMAGENET1K_V1="IMAGENET1K_V1")
    models.vgg16 = lambda *a, **k: types.SimpleNamespace(features=vgg16_features(weights))
    tv.models = models
    sys.modules["torchvision"], sys.modules["torchvision.models"] = tv, models
    torch.hub.load_state_dict_from_url = lambda url, **k: lv.lin_state_dict(weights, upstream=True)
    sys.path.insert(0, REF)
    try:
        return importlib.import_module("lpipsPyTorch")
    finally:
        sys.path.remove(REF)


def main():
    torch.manual_seed(0)
    weights = lv.synthetic_weights(lv.WEIGHT_SEED)
    pkg = reference_package(weights)
    sums = lv.weight_sums(weights)
    out = {}
    for H, W in lv.FIXTURE_SIZES:
        x, y = lv.images(H, W, lv.image_seed(H, W))
        with torch.no_grad():
            ref32 = float(pkg.lpips(torch.from_numpy(x), torch.from_numpy(y), net_type="vgg"))
            crit = pkg.LPIPS("vgg", "0.1").double()
            res, hooks = [], []
            for lin in crit.lin:
                hooks.append(lin.register_forward_hook(lambda m, i, o: res.append(float(o.mean((2, 3), True)))))
            ref64 = float(crit(torch.from_numpy(x).double(), torch.from_numpy(y).double()))
            for h in hooks:
                h.remove()
        taps = np.array(res, np.float64)
        assert taps.shape == (5,) and abs(taps.sum() - ref64) <= 1e-14 * ref64
        mine, min_norm = lv.lpips_vgg_ref(x, y, weights, torch.float64, with_min_norm=True)
        mine = mine.numpy()
        lv.check_inputs(x, y, taps, min_norm)
        rel = np.abs(mine - taps) / taps
        assert rel.max() <= 1e-12 and abs(mine.sum() - ref64) <= 1e-12 * ref64, rel
        t = f"s{H}x{W}_"
        out.update({t + "seed": np.int64(lv.WEIGHT_SEED), t + "image_seed": np.int64(lv.image_seed(H, W)), t + "weight_sums": sums,
                    t + "x": x, t + "y": y, t + "ref_f32": np.float32(ref32), t + "ref_f64": np.float64(ref64),
                    t + "ref_taps_f64": taps})
        print(f"{H}x{W}: lpips fp32 {ref32:.9g} fp64 {ref64:.12g} taps {taps} smallest norm {min_norm:.3g} "
              f"restatement rel err {rel.max():.1e}")
    H, W = lv.EXTRA_SIZE
    x, y = lv.images(H, W, lv.image_seed(H, W))
    taps, min_norm = lv.lpips_vgg_ref(x, y, weights, torch.float64, with_min_norm=True)
    lv.check_inputs(x, y, taps.numpy(), min_norm)
    dst = os.path.join(HERE, "lpips_vgg.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")
    assert os.path.getsize(dst) <= 512 * 1024


if __name__ == "__main__":
    main()
