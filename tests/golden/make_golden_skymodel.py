"""Generate tests/golden/skymodel.npz by RUNNING THE REFERENCE'S OWN SkyModel and get_directions (scene/background_model.py,
scene/encodings.py) on CPU in the build container, in the style of make_golden.py: /root/reference is only ever imported here.

    python tests/golden/make_golden_skymodel.py

Contents: the six weight tensors of a default-initialised SkyModel scaled by 3 (unscaled, the colours only span 0.46 .. 0.55 and
the sigmoid is nearly linear; scaled they span about 0.1 .. 0.99), the state dict's key list, and for two cameras (one of them
rotated; 16 x 24 and 37 x 53 pixels) c2w, intrinsic, the directions [H,W,3] and the sky colours [3,H,W] = sigmoid(SkyModel(dirs))
as Background_Model.forward forms them, each in float32 and in float64.  The pixel grid is built as Background_Model.__init__:489-492
builds it (that constructor itself asks for a CUDA device)."""
import importlib
import math
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))


def import_reference():
    tk = types.ModuleType("tkinter"); tk.W = "w"; sys.modules["tkinter"] = tk
    ply = types.ModuleType("plyfile"); ply.PlyData = ply.PlyElement = object; sys.modules["plyfile"] = ply
    for name in ("open3d", "cv2"):
        sys.modules.setdefault(name, types.ModuleType(name))
    knn = types.ModuleType("simple_knn"); knn_c = types.ModuleType("simple_knn._C"); knn_c.distCUDA2 = None
    knn._C = knn_c; sys.modules["simple_knn"] = knn; sys.modules["simple_knn._C"] = knn_c
    scene = types.ModuleType("scene"); scene.__path__ = [os.path.join(REF, "scene")]; sys.modules["scene"] = scene
    utils = types.ModuleType("utils"); utils.__path__ = [os.path.join(REF, "utils")]; sys.modules["utils"] = utils
    sys.path.insert(0, REF)
    return importlib.import_module("scene.background_model")


def rotation(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch), math.cos(roll), math.sin(roll)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    Ry = np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
    Rx = np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]])
    return Rz @ Ry @ Rx


def pixel_grid(img_width, img_height):
    # scene/background_model.py:489-492 without the device
    x = torch.arange(0, img_width, dtype=torch.float32)
    y = torch.arange(0, img_height, dtype=torch.float32)
    x, y = x.long(), y.long()
    return torch.stack(torch.meshgrid(x, y, indexing='xy')).float()


def main():
    bm = import_reference()
    torch.manual_seed(20240)
    model = bm.SkyModel({"mlp_width": 256})
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(3.0)
    out = {"state_keys": np.array(list(model.state_dict().keys()))}
    for k, v in model.state_dict().items():
        out["w." + k] = v.numpy().copy()
    model64 = bm.SkyModel({"mlp_width": 256}).double()
    model64.load_state_dict({k: v.double() for k, v in model.state_dict().items()})
    cams = [
        dict(H=16, W=24, R=np.eye(3), t=[0.0, 0.0, 0.0], fx=20.0, fy=21.0, cx=12.0, cy=8.0),
        dict(H=37, W=53, R=rotation(0.7, -0.3, 0.2), t=[1.0, -2.0, 0.5], fx=41.5, fy=39.25, cx=25.75, cy=19.5),
    ]
    for i, c in enumerate(cams):
        c2w = np.eye(4)
        c2w[:3, :3] = c["R"]
        c2w[:3, 3] = c["t"]
        K = np.array([[c["fx"], 0, c["cx"]], [0, c["fy"], c["cy"]], [0, 0, 1.0]])
        grid = pixel_grid(c["W"], c["H"])
        out[f"cam{i}.size"] = np.array([c["H"], c["W"]])
        out[f"cam{i}.c2w"] = c2w
        out[f"cam{i}.intrinsic"] = K
        for dt, m, tag in ((torch.float32, model, "32"), (torch.float64, model64, "64")):
            x, y = grid[0].flatten().to(dt), grid[1].flatten().to(dt)
            with torch.no_grad():
                dirs = bm.get_directions(x, y, torch.from_numpy(c2w).to(dt), torch.from_numpy(K).to(dt)).reshape(c["H"], c["W"], 3)
                sky = torch.sigmoid(m(dirs)).permute(2, 0, 1)
            assert dirs.dtype == dt and sky.dtype == dt
            out[f"cam{i}.dirs{tag}"] = dirs.numpy()
            out[f"cam{i}.sky{tag}"] = sky.numpy()
        print(f"cam{i}: sky range {out[f'cam{i}.sky64'].min():.4f} .. {out[f'cam{i}.sky64'].max():.4f}, "
              f"|f32 - f64| max {np.abs(out[f'cam{i}.sky32'] - out[f'cam{i}.sky64']).max():.3e}")
    path = os.path.join(HERE, "skymodel.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
