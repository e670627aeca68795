"""CPU-only checks of the sky colour model: the float64 restatement against the reference's recorded output, the state-dict
names, camera_intrinsics against the rasterizer's projection, and refusals that name their argument."""
import math

import numpy as np
import pytest
import torch

from s3gaussian_amd import skymodel, synth
from tests import skymodel_ref as ref


@pytest.fixture(scope="module")
def golden():
    return ref.load_golden()


@pytest.mark.parametrize("i", [0, 1])
def test_restatement_equals_the_reference_in_float64(golden, i):
    c2w, K, H, W = ref.golden_camera(golden, i)
    w = ref.golden_weights(golden)
    dirs = ref.directions(c2w[:3, :3], K[0, 0], K[1, 1], K[0, 2], K[1, 2], H, W, torch.float64)
    assert np.abs(dirs.reshape(H, W, 3).numpy() - golden[f"cam{i}.dirs64"]).max() < 1e-12
    sky = ref.sky_image(w, c2w[:3, :3], K[0, 0], K[1, 1], K[0, 2], K[1, 2], H, W)
    assert sky.shape == (3, H, W)
    assert np.abs(sky.numpy() - golden[f"cam{i}.sky64"]).max() < 1e-12
    # the float32 restatement is a float32 route like the reference's own: its distance from float64 stays within 4 x the distance
    # the reference's float32 output (recorded in the fixture) has from the reference's float64 output, the project's convention
    w32 = ref.golden_weights(golden, torch.float32)
    sky32 = ref.sky_image(w32, c2w[:3, :3], K[0, 0], K[1, 1], K[0, 2], K[1, 2], H, W)
    assert sky32.dtype == torch.float32
    yardstick = np.abs(golden[f"cam{i}.sky32"].astype(np.float64) - golden[f"cam{i}.sky64"]).max()
    assert 1e-7 < yardstick < 2e-6
    assert np.abs(sky32.numpy().astype(np.float64) - golden[f"cam{i}.sky64"]).max() <= 4 * yardstick


def test_parameter_count_and_composite_of_the_restatement(golden):
    w = ref.golden_weights(golden)
    assert sum(t.numel() for t in w) == 83715 == skymodel.N_PARAMS
    c2w, K, H, W = ref.golden_camera(golden, 0)
    g = torch.Generator().manual_seed(0)
    render, alpha = torch.rand(3, H, W, generator=g, dtype=torch.float64), torch.rand(H, W, generator=g, dtype=torch.float64)
    img = ref.composite(w, c2w[:3, :3], K[0, 0], K[1, 1], K[0, 2], K[1, 2], render, alpha)
    want = render.numpy() + (1 - alpha.numpy())[None] * golden["cam0.sky64"]
    assert np.abs(img.numpy() - want).max() < 1e-12


def test_state_dict_names_are_the_references(golden):
    keys = [str(k) for k in golden["state_keys"]]
    m = skymodel.SkyModel()
    assert list(m.state_dict().keys()) == keys
    sd = {k: torch.from_numpy(golden["w." + k]) for k in keys}
    m.load_state_dict(sd)                                          # strict
    for name, t in zip(ref.NAMES, m.tensors()):
        assert torch.equal(t.detach(), sd[name])
    m2 = skymodel.SkyModel.from_state_dict({"sky_model." + k: v for k, v in sd.items()})      # a Background_Model state
    with pytest.raises(RuntimeError, match="pixel_coord"):                                     # strict: nothing is dropped silently
        skymodel.SkyModel.from_state_dict({**sd, "pixel_coord": torch.zeros(2, 4, 4)})
    for a, b in zip(m.tensors(), m2.tensors()):
        assert torch.equal(a.detach(), b.detach())
    assert torch.equal(m2.direction_encoding.scales, torch.tensor([1.0, 2.0, 4.0, 8.0, 16.0]))


def test_default_initialisation_is_nn_linears():
    torch.manual_seed(5)
    m = skymodel.SkyModel()
    torch.manual_seed(5)
    layers = [torch.nn.Linear(33, 256), torch.nn.Linear(289, 256), torch.nn.Linear(256, 3)]
    for mine, theirs in zip(m.sky_head.layers, layers):
        assert torch.equal(mine.weight, theirs.weight) and torch.equal(mine.bias, theirs.bias)


def test_camera_intrinsics_agrees_with_the_rasterizers_projection():
    """A point placed along pixel (x, y)'s direction projects through the camera's projmatrix onto that pixel's centre
    (the rasterizer's ndc2Pix: ((ndc + 1) * S - 1) / 2, integer coordinates at pixel centres).  numpy only."""
    W, H = 53, 37
    fovx = math.radians(70.0)
    fovy = 2 * math.atan(math.tan(fovx / 2) * H / W * 1.1)
    eye = np.array([1.0, -2.0, 0.5])
    cam = synth.make_camera(synth.look_at(eye, eye + np.array([0.8, 0.5, -0.2])), eye, fovx, fovy, W, H)
    R, fx, fy, cx, cy = skymodel.camera_intrinsics(cam)
    R = R.numpy().astype(np.float64)
    proj = cam["projmatrix"].numpy().astype(np.float64)
    for x, y in [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, H // 2)]:
        d = R @ np.array([(x - cx + 0.5) / fx, (y - cy + 0.5) / fy, 1.0])
        pt = eye + 3.7 * d / np.linalg.norm(d)
        hom = np.append(pt, 1.0) @ proj                               # row-vector convention
        ndc = hom[:2] / hom[3]
        pix = ((ndc + 1.0) * np.array([W, H]) - 1.0) * 0.5
        assert np.abs(pix - np.array([x, y])).max() < 1e-3, (x, y, pix)
        assert hom[3] > 0
    # the reference's own arguments are accepted instead
    c2w, K = torch.eye(4), torch.tensor([[20.0, 0, 12.0], [0, 21.0, 8.0], [0, 0, 1.0]])
    R2, fx2, fy2, cx2, cy2 = skymodel.camera_intrinsics(c2w=c2w[None], intrinsic=K)
    assert torch.equal(R2, torch.eye(3)) and (float(fx2), float(fy2), float(cx2), float(cy2)) == (20.0, 21.0, 12.0, 8.0)


def test_refusals_name_the_offending_argument():
    with pytest.raises(NotImplementedError, match="mlp_width"):
        skymodel.SkyModel({"mlp_width": 128})
    with pytest.raises(NotImplementedError, match="model_type"):
        skymodel.SkyModel(model_type="gs")
    with pytest.raises(NotImplementedError, match="encoder"):
        skymodel.SkyModel(encoder="hash")
    with pytest.raises(RuntimeError, match="intrinsic"):
        skymodel.camera_intrinsics(c2w=torch.eye(4))
    with pytest.raises(RuntimeError, match=r"c2w must have shape \[4,4\], \[3,4\] or \[3,3\]"):
        skymodel.camera_intrinsics(c2w=torch.eye(5), intrinsic=torch.eye(3))
    R34 = skymodel.camera_intrinsics(c2w=torch.eye(4)[:3], intrinsic=torch.eye(3))[0]           # [3,4]: rotation and translation
    assert torch.equal(R34, torch.eye(3))
