"""Generate tests/golden/deform_geometry.npz by RUNNING THE REFERENCE'S OWN scene/deformation.py (CPU) in the build container, the
way make_golden.py does (its import_reference() is reused; the reference is only ever imported here, never copied, and does not
exist where the tests run).

    python tests/golden/make_golden_geometry.py

The full-width network (4 levels x 32 channels = the 128 inputs of feature_out, reduced plane resolution [4, 4, 4, 3] x multires
[1, 2, 4, 8]) with every head on (no_ds = no_dr = no_do = False), evaluated on 100 points twice: rotations + dr, and with
apply_rotation (the normalised quaternion product).  apply_rotation has no parameters, so ONE state dict serves both variants.
Recorded: the state dict, the inputs, the eight outputs of each variant with their loss weights, and dL/dxyz."""
import importlib.util
import os
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
VARIANTS = {"all_heads": dict(), "all_heads_apply_rotation": dict(apply_rotation=True)}
NAMES = ["means3D", "scales", "rotations", "opacity", "shs", "dx", "feat", "dshs"]
AABB = ([2.0, 1.5, 1.0], [-1.0, -1.5, -0.5])


def main():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(HERE, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    m = mg.import_reference()
    fx = {}
    for tag, over in VARIANTS.items():
        hyper = SimpleNamespace(net_width=64, timebase_pe=4, defor_depth=1, posebase_pe=10, scale_rotation_pe=2, opacity_pe=2,
                                timenet_width=64, timenet_output=32, bounds=1.6, plane_tv_weight=0.0001,
                                time_smoothness_weight=0.01, l1_time_planes=0.0001,
                                kplanes_config={"grid_dimensions": 2, "input_coordinate_dim": 4, "output_coordinate_dim": 32,
                                                "resolution": [4, 4, 4, 3]},
                                multires=[1, 2, 4, 8], no_dx=False, no_grid=False, no_ds=False, no_dr=False, no_do=False, no_dshs=False,
                                feat_head=True, empty_voxel=False, grid_pe=0, static_mlp=False, apply_rotation=False)
        for k, v in over.items():
            setattr(hyper, k, v)
        torch.manual_seed(4321)          # the same weights for both variants
        net = m["scene.deformation"].deform_network(hyper)
        g = torch.Generator().manual_seed(11)
        with torch.no_grad():            # planes non-trivial (time planes are all-ones at init), biases non-zero
            for p in net.deformation_net.grid.grids.parameters():
                p.add_(0.2 * torch.randn(p.shape, generator=g))
            for mod in net.deformation_net.modules():
                if isinstance(mod, torch.nn.Linear):
                    mod.bias.add_(0.1 * torch.randn(mod.bias.shape, generator=g))
        net.deformation_net.set_aabb(*AABB)
        P = 100
        xyz = (torch.rand(P, 3, generator=g) * torch.tensor([2.6, 2.6, 1.2]) + torch.tensor([-0.8, -1.3, -0.4])).requires_grad_(True)
        sc, rot, op = torch.randn(P, 3, generator=g), torch.randn(P, 4, generator=g), torch.randn(P, 1, generator=g)
        shs = torch.randn(P, 16, 3, generator=g)
        time = torch.full((P, 1), 0.61)
        outs = net(xyz, sc, rot, op, shs, time)
        assert len(outs) == 8 and all(o is not None for o in outs)
        w = [torch.randn(o.shape, generator=g) for o in outs]
        sum((o * wi).sum() for o, wi in zip(outs, w)).backward()
        sd = {k: v.numpy() for k, v in net.state_dict().items()}
        if not any(k.startswith("sd::") for k in fx):
            fx.update({"sd::" + k: v for k, v in sd.items()})
            fx.update(xyz=xyz.detach().numpy(), scales=sc.numpy(), rotations=rot.numpy(), opacity=op.numpy(), shs=shs.numpy(),
                      time=time.numpy())
        else:                            # one state dict, one set of inputs
            assert all(np.array_equal(fx["sd::" + k], v) for k, v in sd.items()) and np.array_equal(fx["xyz"], xyz.detach().numpy())
        fx[tag + "::grad_xyz"] = xyz.grad.numpy()
        for n, o, wi in zip(NAMES, outs, w):
            fx[f"{tag}::out_{n}"] = o.detach().numpy()
            fx[f"{tag}::w_{n}"] = wi.numpy()
    path = os.path.join(HERE, "deform_geometry.npz")
    np.savez_compressed(path, **fx)
    print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
