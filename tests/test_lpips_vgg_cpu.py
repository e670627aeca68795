"""CPU-only: tests/lpips_vgg_ref.py (the restatement the GPU test compares s3gaussian_amd.lpips_vgg with) against the values the
reference's own lpipsPyTorch modules produced for tests/golden/lpips_vgg.npz (tests/golden/make_golden_lpips_vgg.py; synthetic
weights, because the pretrained ones exist on no machine these tests run on), the key-name handling of LPIPSVGG.from_state_dicts up
to the device pack, and the library's size queries.

The float64 comparison at 1e-12 pins the z-score without the [-1,1] rescale, the eps placement outside the square root, the taps
after the last ReLU of every block and before its pool, the floor-mode 2x2 pools and the spatial mean before the sum over the taps."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import lpips_vgg_ref as lv


@pytest.fixture(scope="module")
def data():
    weights = lv.synthetic_weights(lv.WEIGHT_SEED)
    cases = lv.load_fixture()
    ref64, rel, bar = lv.float32_route_errors()
    return weights, cases, ref64, rel, bar


def test_generator_has_not_drifted(data):
    weights, cases, _, _, _ = data
    sums = lv.weight_sums(weights)
    assert sums.shape == (31,)
    for c in cases:
        assert c["seed"] == lv.WEIGHT_SEED and c["image_seed"] == lv.image_seed(c["H"], c["W"])
        assert np.array_equal(c["weight_sums"], sums)
        x, y = lv.images(c["H"], c["W"], c["image_seed"])
        assert np.array_equal(x, c["x"]) and np.array_equal(y, c["y"])
    for w, (ci, co) in zip(weights["conv_w"], lv.CHANNELS):
        assert w.shape == (co, ci, 3, 3) and w.dtype == np.float32
    assert [w.shape[0] for w in weights["lin_w"]] == [64, 128, 256, 512, 512] and all((w >= 0).all() for w in weights["lin_w"])


def test_float64_restatement_equals_the_reference(data):
    weights, cases, ref64, _, _ = data
    for k, c in enumerate(cases):
        rel = np.abs(ref64[k] - c["ref_taps_f64"]) / c["ref_taps_f64"]
        print(f"{c['H']}x{c['W']}: taps {ref64[k]} rel err {rel.max():.2e}")
        assert rel.max() <= 1e-12
        assert abs(ref64[k].sum() - c["ref_f64"]) <= 1e-12 * c["ref_f64"]


def test_input_conditions_hold(data):
    """Every tap value at least 1e-4, the smallest feature norm at least 1e-3, no constant image: a relative bar means something."""
    weights, _, _, _, _ = data
    for H, W, x, y in lv.all_cases():
        taps, min_norm = lv.lpips_vgg_ref(x, y, weights, torch.float64, with_min_norm=True)
        print(f"{H}x{W}: smallest tap {float(taps.min()):.3e}, smallest norm {min_norm:.3g}")
        lv.check_inputs(x, y, taps.numpy(), min_norm)


def test_recorded_fp32_value_is_within_the_bar(data):
    """The bar: 4 x the largest relative error, over the four cases and five taps, of two float32 restatements (F.conv2d; nine shifted
    1x1 convolutions added in (kh, kw) order) against the float64 one."""
    weights, cases, ref64, rel, bar = data
    print(f"float32 routes: F.conv2d {rel[0].min():.1e} .. {rel[0].max():.1e}, shifted 1x1 {rel[1].min():.1e} .. {rel[1].max():.1e}, "
          f"bar {bar:.2e}")
    assert rel.shape == (2, 4, 5) and 0 < bar < 1e-3
    for k, c in enumerate(cases):
        mine32 = float(lv.lpips_vgg_ref(c["x"], c["y"], weights, torch.float32).sum())
        assert abs(mine32 - c["ref_f32"]) <= bar * c["ref_f32"], (mine32, c["ref_f32"])
        assert abs(c["ref_f32"] - c["ref_f64"]) <= bar * c["ref_f64"]


def test_wrong_readings_are_far_outside_the_bar(data):
    """What the bar must tell apart, on the 40 x 52 case: taps taken after the pool, the AlexNet variant's 3x3 pool, and the [-1,1]
    rescale of the upstream LPIPS package in front of the z-score each move some tap by more than a hundred bars."""
    weights, cases, ref64, _, bar = data
    c = cases[2]
    readings = {"tap_after_pool": lv.lpips_vgg_ref(c["x"], c["y"], weights, wrong="tap_after_pool"),
                "pool3": lv.lpips_vgg_ref(c["x"], c["y"], weights, wrong="pool3"),
                "rescale": lv.lpips_vgg_ref(2 * c["x"] - 1, 2 * c["y"] - 1, weights)}
    for name, vals in readings.items():
        moved = (np.abs(vals.numpy() - ref64[2]) / ref64[2]).max()
        print(f"{name}: largest tap move {moved:.2e} = {moved / bar:.0f} bars")
        assert moved > 100 * bar, name


def _state_dicts(weights, upstream):
    return lv.vgg_state_dict(weights), lv.lin_state_dict(weights, upstream=upstream)


def test_state_dict_keys_are_collected_under_both_naming_schemes(data):
    from s3gaussian_amd import lpips_vgg as lp
    weights = data[0]
    for upstream in (True, False):
        vgg, lin = _state_dicts(weights, upstream)
        vgg["classifier.0.weight"] = torch.zeros(4, 4)          # other keys are ignored
        conv_w, conv_b, lin_w = lp.collect_weights(vgg, lin)
        assert len(conv_w) == len(conv_b) == 13 and len(lin_w) == 5
        for i in range(13):
            assert conv_w[i].shape == lp.CONV_SHAPES[i] and conv_w[i].dtype == torch.float32
            assert torch.equal(conv_w[i], torch.from_numpy(weights["conv_w"][i]))
            assert torch.equal(conv_b[i], torch.from_numpy(weights["conv_b"][i]))
        for i in range(5):
            assert lin_w[i].shape == (lp.TAP_CHANNELS[i],) and torch.equal(lin_w[i], torch.from_numpy(weights["lin_w"][i]))


def test_bad_state_dicts_and_cpu_devices_are_refused_before_any_device_call(data):
    from s3gaussian_amd import lpips as alex
    from s3gaussian_amd import lpips_vgg as lp
    weights = data[0]
    vgg, lin = _state_dicts(weights, True)
    missing = dict(vgg)
    del missing["features.17.bias"]
    with pytest.raises(KeyError, match="features.17.bias"):
        lp.collect_weights(missing, lin)
    with pytest.raises(KeyError, match="lin3.model.1.weight"):
        lp.collect_weights(vgg, {k: v for k, v in lin.items() if not k.startswith("lin3")})
    both = dict(lin)
    both["2.1.weight"] = lin["lin2.model.1.weight"]
    with pytest.raises(KeyError, match="exactly one"):
        lp.collect_weights(vgg, both)
    wrong = dict(vgg)
    wrong["features.5.weight"] = torch.zeros(128, 64, 5, 5)
    with pytest.raises(RuntimeError, match="features.5"):
        lp.collect_weights(wrong, lin)
    flat = dict(lin)
    flat["lin0.model.1.weight"] = torch.zeros(64)
    with pytest.raises(RuntimeError, match="lin0.model.1.weight"):
        lp.collect_weights(vgg, flat)
    with pytest.raises(RuntimeError, match="GPU"):
        lp.LPIPSVGG.from_state_dicts(vgg, lin, "cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        lp.lpips_vgg(lp.LPIPSVGG(torch.zeros(1, dtype=torch.uint8)), torch.rand(3, 40, 40), torch.rand(3, 40, 40))
    with pytest.raises(TypeError, match="LPIPSVGG model"):
        lp.lpips_vgg(alex.LPIPS(torch.zeros(1, dtype=torch.uint8)), torch.rand(3, 40, 40), torch.rand(3, 40, 40))
    assert lp.MIN_SIZE == 16 and lp.RECORD == alex.RECORD and lp.TOTAL == alex.TOTAL and lp.TAP0 == alex.TAP0
    with pytest.raises(NotImplementedError, match="lpips_vgg"):          # the AlexNet module still refuses, and says where to go
        alex.LPIPS(torch.zeros(1, dtype=torch.uint8), net_type="vgg")


def test_library_sizes_without_a_gpu():
    """The size queries launch nothing: the blob holds every conv's B operand with K = 9 ci padded to the K step of 32, its bias, and
    after a tapped conv the lin weights; the workspace is 0 below 16 x 16, non-decreasing in H and W, and within
    2 A1 + A1 / 8 + 1 MiB with A1 = 2 * 4 * H * W * 64 bytes, one block-1 activation pair."""
    from s3gaussian_amd import lpips_vgg as lp
    L = lp._bind()
    floats = sum(-(-(9 * ci) // 32) * 32 * co + co for ci, co in lv.CHANNELS) + sum(lv.CHANNELS[c][1] for c in lv.TAP_CONVS)
    assert L.s3g_lpips_vgg_weights_bytes() == 4 * floats
    assert L.s3g_lpips_vgg_workspace_bytes(15, 100) == 0 and L.s3g_lpips_vgg_workspace_bytes(100, 15) == 0
    sizes = [16, 17, 23, 31, 32, 40, 52, 64, 150, 210, 1066, 1600]
    prev_row = None
    for H in sizes:
        row = [L.s3g_lpips_vgg_workspace_bytes(H, W) for W in sizes]
        assert row[0] > 0 and all(a <= b for a, b in zip(row, row[1:]))
        assert prev_row is None or all(a <= b for a, b in zip(prev_row, row))
        for W, got in zip(sizes, row):
            a1 = 2 * 4 * H * W * 64
            assert 2 * a1 <= got <= 2 * a1 + a1 // 8 + (1 << 20), (H, W, got)
        prev_row = row
    a1 = 2 * 4 * 1066 * 1600 * 64
    big = L.s3g_lpips_vgg_workspace_bytes(1066, 1600)
    print(f"1066 x 1600: workspace {big / 1e9:.3f} GB, bound {(2 * a1 + a1 // 8 + (1 << 20)) / 1e9:.3f} GB")
    assert big <= 2 * a1 + a1 // 8 + (1 << 20)
    assert L.s3g_lpips_vgg(15, 64, None, None, None, None, None, None) == 1 and b"smaller than 16 x 16" in L.s3g_last_error()
    assert L.s3g_lpips_vgg(64, 64, None, None, None, None, None, None) == 1 and b"NULL" in L.s3g_last_error()
    # 2 * 4096 * 4096 * 64 = 2^31 activation elements in block 1
    assert L.s3g_lpips_vgg(4096, 4096, None, None, None, None, None, None) == 1
    assert b"more activation elements" in L.s3g_last_error()
    assert L.s3g_lpips_vgg(4095, 4096, None, None, None, None, None, None) == 1 and b"NULL" in L.s3g_last_error()


def test_conv_kernels_keep_their_registers_and_lds():
    """The conv kernel's staged operands live in registers: no scratch, and no LDS beyond the two double-buffered tiles (as an array
    captured by the staging lambdas the B rows once went to scratch for BN = 64 and were promoted to 16 KiB of LDS for BN = 128, which
    leaves one workgroup per CU).  64 KiB at BN = 128: two workgroups per CU; 48 KiB at BN = 64: three."""
    from s3gaussian_amd import _lib
    _lib.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run(["bash", os.path.join(root, "tools", "kernel_resources.sh"),
                          os.path.join(root, "s3gaussian_amd", "lib", "lpips_vgg.o")], capture_output=True, text=True, timeout=300).stdout
    convs = {}
    for line in out.splitlines():
        m = re.match(r"\S*lpips_conv_kernelILi3ELi1ELi1ELi(\d+)ELi(\d+)ELi(\d+)E\S*\s+vgpr\s+(\d+).*?lds\s+(\d+)\s+scratch\s+(\d+)", line)
        if m:
            convs[tuple(int(v) for v in m.groups()[:3])] = tuple(int(v) for v in m.groups()[3:])
    assert set(convs) == {(3, 64, 64), (64, 64, 64), (64, 128, 128), (128, 128, 128), (128, 256, 128), (256, 256, 128),
                          (256, 512, 128), (512, 512, 128)}, out
    for (ci, co, bn), (vgpr, lds, scratch) in convs.items():
        assert scratch == 0 and lds == 2 * 32 * (128 + bn) * 4, (ci, co, bn, vgpr, lds, scratch)
        assert vgpr <= 256 and (bn == 128 or vgpr <= 168), (ci, co, bn, vgpr)      # vgpr counts the accumulators' AGPRs too
    # the AlexNet variant instantiates the same kernel, always at BN = 64
    out = subprocess.run(["bash", os.path.join(root, "tools", "kernel_resources.sh"),
                          os.path.join(root, "s3gaussian_amd", "lib", "lpips.o")], capture_output=True, text=True, timeout=300).stdout
    alex = {}
    for line in out.splitlines():
        m = re.match(r"\S*lpips_conv_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E\S*\s+vgpr\s+(\d+).*?lds\s+(\d+)\s+scratch\s+(\d+)",
                     line)
        if m:
            alex[tuple(int(v) for v in m.groups()[:6])] = tuple(int(v) for v in m.groups()[6:])
    assert set(alex) == {(11, 4, 2, 3, 64, 64), (5, 1, 2, 64, 192, 64), (3, 1, 1, 192, 384, 64), (3, 1, 1, 384, 256, 64),
                         (3, 1, 1, 256, 256, 64)}, out
    for key, (vgpr, lds, scratch) in alex.items():
        assert scratch == 0 and lds == 49152 and vgpr <= 168, (key, vgpr, lds, scratch)
