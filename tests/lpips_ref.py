"""Helper (not a test): the reference's `lpips(x, y, net_type='alex')` restated on torch-CPU tensors, plus the synthetic weights and
images the LPIPS tests share.

What is restated (lpipsPyTorch/modules/networks.py:41-63, 77-85; utils.py:6-8; lpips.py:30-36), for x, y of shape [3,H,W] in [0,1]:
  z = (img - mean) / std with mean (-.030, -.088, -.188), std (.458, .448, .450): no rescale to [-1,1], no clamp;
  torchvision's AlexNet `features` tapped after each of its five ReLUs (floor-mode 3x3 stride-2 pools after the first two);
  per tap and pixel n = sqrt(sum_c a_c^2), a^ = a / (n + 1e-10);  d_c = (a^x_c - a^y_c)^2;
  tap value = mean over pixels of sum_c w_c d_c;  result = sum of the five tap values.

The real weights (torchvision's alexnet-owt-*.pth, about 10 MB, and the lin weights alex.pth) are too large for a fixture and exist on
no machine these tests run on: every test draws weights of the same shapes from a seed."""
import os

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "lpips.npz")

# (co, ci, k, stride, pad, pool after the ReLU)
LAYERS = ((64, 3, 11, 4, 2, True), (192, 64, 5, 1, 2, True), (384, 192, 3, 1, 1, False), (256, 384, 3, 1, 1, False),
          (256, 256, 3, 1, 1, False))
FEATURE_INDEX = (0, 3, 6, 8, 10)               # torchvision's alexnet.features: the five Conv2d modules
MEAN = (-.030, -.088, -.188)
STD = (.458, .448, .450)
EPS = 1e-10

WEIGHT_SEED = 7
FIXTURE_SIZES = ((31, 31), (35, 47), (67, 93), (64, 96))
EXTRA_SIZE = (150, 530)                        # GPU test only: every layer spans several 128-pixel tiles and ends in a partial one
BAR_FACTOR = 4.0                               # a different K summation order, as in test_step_gradients_gpu.py
MIN_TAP, MIN_NORM = 1e-3, 1e-3                 # input conditions under which a relative bar means something


def image_seed(H, W):
    return 1000 * H + W


def synthetic_weights(seed=WEIGHT_SEED):
    """{"conv_w": 5 x [co,ci,k,k], "conv_b": 5 x [co], "lin_w": 5 x [co]} fp32 numpy, drawn per layer in the order conv weight, bias,
    lin: N(0, 2 / (ci k k)), N(0, 0.1^2), |N(0, 1)|."""
    rng = np.random.default_rng(seed)
    out = {"conv_w": [], "conv_b": [], "lin_w": []}
    for co, ci, k, _, _, _ in LAYERS:
        out["conv_w"].append((rng.standard_normal((co, ci, k, k)) * np.sqrt(2.0 / (ci * k * k))).astype(np.float32))
        out["conv_b"].append((rng.standard_normal(co) * 0.1).astype(np.float32))
        out["lin_w"].append(np.abs(rng.standard_normal(co)).astype(np.float32))
    return out


def weight_sums(weights):
    """The float64 sum of every weight tensor, in the order conv_w[0..4], conv_b[0..4], lin_w[0..4]: catches generator drift."""
    return np.array([float(np.sum(t, dtype=np.float64)) for name in ("conv_w", "conv_b", "lin_w") for t in weights[name]])


def images(H, W, seed):
    """(x, y) fp32 [3,H,W]: y uniform in [0,1), x = clamp(y + 0.1 randn, 0, 1)."""
    rng = np.random.default_rng(seed)
    y = rng.random((3, H, W)).astype(np.float32)
    x = np.clip(y + np.float32(0.1) * rng.standard_normal((3, H, W)).astype(np.float32), np.float32(0), np.float32(1))
    return x.astype(np.float32), y


def alexnet_state_dict(weights):
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


def _features(img, weights, dtype):
    mean = torch.tensor(MEAN, dtype=torch.float32).to(dtype)[:, None, None]      # fp32 constants, as the reference's buffers
    std = torch.tensor(STD, dtype=torch.float32).to(dtype)[:, None, None]
    a = ((img - mean) / std)[None]
    taps = []
    for i, (_, _, _, stride, pad, pool) in enumerate(LAYERS):
        w = torch.from_numpy(weights["conv_w"][i]).to(dtype)
        b = torch.from_numpy(weights["conv_b"][i]).to(dtype)
        a = F.relu(F.conv2d(a, w, b, stride=stride, padding=pad))
        taps.append(a)
        if pool:
            a = F.max_pool2d(a, 3, 2)
    return taps


def lpips_ref(x, y, weights, dtype=torch.float64, with_min_norm=False):
    """The five tap values (a [5] tensor of `dtype`; the LPIPS value is their sum).  x, y: [3,H,W] numpy or torch.
    with_min_norm: also the smallest feature norm over all pixels, taps and both images."""
    x, y = torch.as_tensor(x).to(dtype), torch.as_tensor(y).to(dtype)
    fx, fy = _features(x, weights, dtype), _features(y, weights, dtype)
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
    assert float(taps64.min()) > MIN_TAP, taps64
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
    """The four fixture cases' images and the 150x530 pair, as [(H, W, x, y)]."""
    out = [(c["H"], c["W"], c["x"], c["y"]) for c in load_fixture()]
    H, W = EXTRA_SIZE
    return out + [(H, W) + images(H, W, image_seed(H, W))]


def float32_route_errors(weights=None, cases=None):
    """-> (ref64 [n,5] float64 tap values, rel [n,5] relative error of the float32 restatement against the float64 one, bar).
    The bar for the GPU values is BAR_FACTOR x the largest entry of `rel`; it never comes from the code under test."""
    weights = synthetic_weights(WEIGHT_SEED) if weights is None else weights
    cases = all_cases() if cases is None else cases
    ref64 = np.stack([lpips_ref(x, y, weights, torch.float64).numpy() for _, _, x, y in cases])
    ref32 = np.stack([lpips_ref(x, y, weights, torch.float32).numpy().astype(np.float64) for _, _, x, y in cases])
    rel = np.abs(ref32 - ref64) / ref64
    return ref64, rel, BAR_FACTOR * float(rel.max())
