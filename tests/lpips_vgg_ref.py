"""Helper (not a test): the reference's `lpips(x, y, net_type='vgg')` restated on torch-CPU tensors, plus the synthetic weights and
images the VGG LPIPS tests share.

What is restated (lpipsPyTorch/modules/networks.py:41-63, 88-96; utils.py:6-8; lpips.py:30-36), for x, y of shape [3,H,W] in [0,1]:
  z = (img - mean) / std with mean (-.030, -.088, -.188), std (.458, .448, .450): no rescale to [-1,1], no clamp;
  torchvision's vgg16 `features`: thirteen k3 s1 p1 convolutions, each followed by a ReLU, in blocks of 2, 2, 3, 3, 3 with a
  floor-mode 2x2 stride-2 max pool after each of the first four; tapped after the LAST ReLU of every block, before its pool
  (target_layers [4, 9, 16, 23, 30] counts modules from 1);
  per tap and pixel n = sqrt(sum_c a_c^2), a^ = a / (n + 1e-10);  d_c = (a^x_c - a^y_c)^2;
  tap value = mean over pixels of sum_c w_c d_c;  result = sum of the five tap values.

The real weights (torchvision's vgg16-397923af.pth, 528 MB, and the lin weights vgg.pth) are too large for a fixture and exist on no
machine these tests run on: every test draws weights of the same shapes from a seed."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests.lpips_ref import BAR_FACTOR, EPS, MEAN, STD, image_seed, images   # the same images, constants and factor  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "lpips_vgg.npz")

# (ci, co) of the thirteen convolutions; the blocks end after convs 1, 3, 6, 9, 12 (0-based): tap, then (but for the last) pool
CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
            (512, 512), (512, 512), (512, 512))
TAP_CONVS = (1, 3, 6, 9, 12)
FEATURE_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)        # torchvision's vgg16.features: the Conv2d modules

WEIGHT_SEED = 7
FIXTURE_SIZES = ((16, 16), (17, 23), (40, 52))    # 1x1 deep layers; odd extents at every pool
EXTRA_SIZE = (150, 210)                           # GPU test only: blocks of 150x210, 75x105, 37x52, 18x26, 9x13 pixels per image --
                                                  # each spans several 128-row tiles and ends in a partial one
MIN_TAP, MIN_NORM = 1e-4, 1e-3                    # input conditions under which a relative bar means something


def synthetic_weights(seed=WEIGHT_SEED):
    """{"conv_w": 13 x [co,ci,3,3], "conv_b": 13 x [co], "lin_w": 5 x [C]} fp32 numpy, drawn per conv in network order: weight
    N(0, 2 / (9 ci)), then bias N(0, 0.1^2), then -- after a tapped conv -- that tap's lin weights |N(0, 1)|."""
    rng = np.random.default_rng(seed)
    out = {"conv_w": [], "conv_b": [], "lin_w": []}
    for l, (ci, co) in enumerate(CHANNELS):
        out["conv_w"].append((rng.standard_normal((co, ci, 3, 3)) * np.sqrt(2.0 / (9 * ci))).astype(np.float32))
        out["conv_b"].append((rng.standard_normal(co) * 0.1).astype(np.float32))
        if l in TAP_CONVS:
            out["lin_w"].append(np.abs(rng.standard_normal(co)).astype(np.float32))
    return out


def weight_sums(weights):
    """The float64 sum of every weight tensor, in the order conv_w[0..12], conv_b[0..12], lin_w[0..4]: catches generator drift."""
    return np.array([float(np.sum(t, dtype=np.float64)) for name in ("conv_w", "conv_b", "lin_w") for t in weights[name]])


def vgg_state_dict(weights):
    """The synthetic conv weights under torchvision's key names."""
    sd = {}
    for i, f in enumerate(FEATURE_INDEX):
        sd[f"features.{f}.weight"] = torch.from_numpy(weights["conv_w"][i])
        sd[f"features.{f}.bias"] = torch.from_numpy(weights["conv_b"][i])
    return sd


def lin_state_dict(weights, upstream=True):
    """The synthetic lin weights [1,C,1,1] under the upstream names (lin{i}.model.1.weight) or the reference's renamed ones."""
    name = "lin{}.model.1.weight" if upstream else "{}.1.weight"
    return {name.format(i): torch.from_numpy(weights["lin_w"][i]).reshape(1, -1, 1, 1) for i in range(5)}


def _conv(a, w, b, shifted):
    """F.conv2d, or -- a second summation order -- the nine (kh, kw) taps added in order as nine shifted 1x1 convolutions."""
    if not shifted:
        return F.conv2d(a, w, b, padding=1)
    H, W = a.shape[2:]
    p = F.pad(a, (1, 1, 1, 1))
    out = None
    for kh in range(3):
        for kw in range(3):
            t = F.conv2d(p[:, :, kh:kh + H, kw:kw + W], w[:, :, kh:kh + 1, kw:kw + 1])
            out = t if out is None else out + t
    return out + b[None, :, None, None]


def _features(img, weights, dtype, shifted=False, wrong=None):
    mean = torch.tensor(MEAN, dtype=torch.float32).to(dtype)[:, None, None]      # fp32 constants, as the reference's buffers
    std = torch.tensor(STD, dtype=torch.float32).to(dtype)[:, None, None]
    a = ((img - mean) / std)[None]
    taps = []
    for l in range(13):
        w = torch.from_numpy(weights["conv_w"][l]).to(dtype)
        b = torch.from_numpy(weights["conv_b"][l]).to(dtype)
        a = F.relu(_conv(a, w, b, shifted))
        if l in TAP_CONVS:
            if wrong != "tap_after_pool":
                taps.append(a)
            if l != 12 or wrong == "tap_after_pool":
                a = F.max_pool2d(a, 3, 2) if wrong == "pool3" else F.max_pool2d(a, 2, 2)
            if wrong == "tap_after_pool":
                taps.append(a)
    return taps


def lpips_vgg_ref(x, y, weights, dtype=torch.float64, with_min_norm=False, shifted=False, wrong=None):
    """The five tap values (a [5] tensor of `dtype`; the LPIPS value is their sum).  x, y: [3,H,W] numpy or torch.
    with_min_norm: also the smallest feature norm over all pixels, taps and both images.
    shifted: every conv as nine shifted 1x1 convolutions added in (kh, kw) order -- another summation order of the same sum.
    wrong: None, or one of the misreadings the bar must tell apart: "tap_after_pool" (the taps taken after each block's pool, the
    fifth pool included), "pool3" (the AlexNet variant's 3x3 stride-2 pools; needs H, W >= 31)."""
    x, y = torch.as_tensor(x).to(dtype), torch.as_tensor(y).to(dtype)
    fx, fy = _features(x, weights, dtype, shifted, wrong), _features(y, weights, dtype, shifted, wrong)
    vals, min_norm = [], float("inf")
    for i in range(5):
        nx = torch.sqrt((fx[i] ** 2).sum(1, keepdim=True))
        ny = torch.sqrt((fy[i] ** 2).sum(1, keepdim=True))
        min_norm = min(min_norm, float(nx.min()), float(ny.min()))
        d = (fx[i] / (nx + EPS) - fy[i] / (ny + EPS)) ** 2
        w = torch.from_numpy(weights["lin_w"][i]).to(dtype)[None, :, None, None]
        vals.append((d * w).sum(1).mean())
    vals = torch.stack(vals)
    return (vals, min_norm) if with_min_norm else vals


def check_inputs(x, y, taps64, min_norm):
    """The input conditions the generator and the CPU test both assert."""
    assert float(np.ptp(x)) > 0 and float(np.ptp(y)) > 0, "constant image"
    assert float(taps64.min()) >= MIN_TAP, taps64
    assert min_norm >= MIN_NORM, min_norm


def load_fixture():
    """[{H, W, seed, image_seed, weight_sums, x, y, ref_f32, ref_f64, ref_taps_f64}] in the order of FIXTURE_SIZES."""
    z = np.load(FIXTURE)
    cases = []
    for H, W in FIXTURE_SIZES:
        t = f"s{H}x{W}_"
        cases.append({"H": H, "W": W, "seed": int(z[t + "seed"]), "image_seed": int(z[t + "image_seed"]),
                      "weight_sums": z[t + "weight_sums"], "x": z[t + "x"], "y": z[t + "y"], "ref_f32": float(z[t + "ref_f32"]),
                      "ref_f64": float(z[t + "ref_f64"]), "ref_taps_f64": z[t + "ref_taps_f64"]})
    return cases


def all_cases():
    """The three fixture cases' images and the 150x210 pair, as [(H, W, x, y)]."""
    out = [(c["H"], c["W"], c["x"], c["y"]) for c in load_fixture()]
    H, W = EXTRA_SIZE
    return out + [(H, W) + images(H, W, image_seed(H, W))]


_ERRORS = {}


def float32_route_errors():
    """-> (ref64 [4,5] float64 tap values, rel [2,4,5] relative errors of the two float32 restatements -- F.conv2d, and the nine
    shifted 1x1 convolutions -- against the float64 one, bar).  The bar for the GPU values is BAR_FACTOR x the largest entry of
    `rel`; it never comes from the code under test.  Computed once per process for synthetic_weights(WEIGHT_SEED) and all_cases()."""
    if not _ERRORS:
        weights, cases = synthetic_weights(WEIGHT_SEED), all_cases()
        ref64 = np.stack([lpips_vgg_ref(x, y, weights, torch.float64).numpy() for _, _, x, y in cases])
        rel = np.stack([np.stack([np.abs(lpips_vgg_ref(x, y, weights, torch.float32, shifted=s).numpy().astype(np.float64) - r) / r
                                  for (_, _, x, y), r in zip(cases, ref64)]) for s in (False, True)])
        _ERRORS["v"] = (ref64, rel, BAR_FACTOR * float(rel.max()))
    return _ERRORS["v"]
