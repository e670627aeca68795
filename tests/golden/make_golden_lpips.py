"""Generate tests/golden/lpips.npz: images and the reference's own LPIPS values for s3gaussian_amd/lpips.py.

    python tests/golden/make_golden_lpips.py        # rewrites lpips.npz next to this file

Runs in the build container only: the recorded values come from the REFERENCE'S OWN lpipsPyTorch package (imported from the reference
tree, never copied).  The pretrained weights exist on no machine this runs on, so `torchvision.models.alexnet` is replaced by a stub
whose `.features` is the 13-layer stack of torchvision's AlexNet holding lpips_ref.synthetic_weights(seed), and
`torch.hub.load_state_dict_from_url` is patched to return the synthetic lin weights under the upstream key names (the reference
renames them itself, lpipsPyTorch/modules/utils.py:22-28).  Without the reference tree this script refuses to run.

Per size s{H}x{W} of lpips_ref.FIXTURE_SIZES: seed (weights), image_seed, weight_sums (float64 sum of every weight tensor), x, y
[3,H,W] fp32, ref_f32 (the reference's lpips(x, y) as called by utils/video_utils.py), ref_f64 (the same module after .double() on
double inputs), ref_taps_f64 (the five entries of LPIPS.forward's `res`, in double, read with forward hooks on its lin layers).
The script asserts lpips_ref.check_inputs on every case, and that the float64 restatement reproduces the reference at 1e-12."""
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

from tests import lpips_ref as lr  # noqa: E402


def alexnet_features(weights):
    """torchvision's AlexNet `features`, restated from its public definition, holding the synthetic weights."""
    layers = []
    for i, (co, ci, k, stride, pad, pool) in enumerate(lr.LAYERS):
        conv = nn.Conv2d(ci, co, kernel_size=k, stride=stride, padding=pad)
        with torch.no_grad():
            conv.weight.copy_(torch.from_numpy(weights["conv_w"][i]))
            conv.bias.copy_(torch.from_numpy(weights["conv_b"][i]))
        layers += [conv, nn.ReLU(inplace=True)]
        if pool or i == 4:
            layers.append(nn.MaxPool2d(kernel_size=3, stride=2))
    assert len(layers) == 13 and [i for i, m in enumerate(layers) if isinstance(m, nn.Conv2d)] == list(lr.FEATURE_INDEX)
    return nn.Sequential(*layers)


def reference_package(weights):
    if not os.path.isfile(os.path.join(REF, "lpipsPyTorch", "__init__.py")):
        raise SystemExit(f"{REF}/lpipsPyTorch is missing: the fixture records the reference's own values and cannot be written "
                         "without it")
    tv, models = types.ModuleType("torchvision"), types.ModuleType("torchvision.models")
    tv.__path__ = []
    models.alexnet = lambda *a, **k: types.SimpleNamespace(features=alexnet_features(weights))
    tv.models = models
    sys.modules["torchvision"], sys.modules["torchvision.models"] = tv, models
    torch.hub.load_state_dict_from_url = lambda url, **k: lr.lin_state_dict(weights, upstream=True)
    sys.path.insert(0, REF)
    try:
        return importlib.import_module("lpipsPyTorch")
    finally:
        sys.path.remove(REF)


def main():
    torch.manual_seed(0)
    weights = lr.synthetic_weights(lr.WEIGHT_SEED)
    pkg = reference_package(weights)
    sums = lr.weight_sums(weights)
    out = {}
    for H, W in lr.FIXTURE_SIZES:
        x, y = lr.images(H, W, lr.image_seed(H, W))
        with torch.no_grad():
            ref32 = float(pkg.lpips(torch.from_numpy(x), torch.from_numpy(y), net_type="alex"))
            crit = pkg.LPIPS("alex", "0.1").double()
            res, hooks = [], []
            for lin in crit.lin:
                hooks.append(lin.register_forward_hook(lambda m, i, o: res.append(float(o.mean((2, 3), True)))))
            ref64 = float(crit(torch.from_numpy(x).double(), torch.from_numpy(y).double()))
            for h in hooks:
                h.remove()
        taps = np.array(res, np.float64)
        assert taps.shape == (5,) and abs(taps.sum() - ref64) <= 1e-14 * ref64
        mine, min_norm = lr.lpips_ref(x, y, weights, torch.float64, with_min_norm=True)
        mine = mine.numpy()
        lr.check_inputs(x, y, taps, min_norm)
        rel = np.abs(mine - taps) / taps
        assert rel.max() <= 1e-12 and abs(mine.sum() - ref64) <= 1e-12 * ref64, rel
        t = f"s{H}x{W}_"
        out.update({t + "seed": np.int64(lr.WEIGHT_SEED), t + "image_seed": np.int64(lr.image_seed(H, W)), t + "weight_sums": sums,
                    t + "x": x, t + "y": y, t + "ref_f32": np.float32(ref32), t + "ref_f64": np.float64(ref64),
                    t + "ref_taps_f64": taps})
        print(f"{H}x{W}: lpips fp32 {ref32:.9g} fp64 {ref64:.12g} taps {taps} smallest norm {min_norm:.3g} "
              f"restatement rel err {rel.max():.1e}")
    dst = os.path.join(HERE, "lpips.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")
    assert os.path.getsize(dst) < 512 * 1024


if __name__ == "__main__":
    main()
