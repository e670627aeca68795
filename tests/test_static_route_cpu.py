"""Static scenes (no_dx=True) on the fused deformation route, the part that needs no GPU: which switch combinations the route
admits, and the flow / decomposition guards refusing a model without a position head before anything is launched."""
from types import SimpleNamespace

import pytest
import torch

SMALL = dict(grid_dimensions=2, input_coordinate_dim=4, output_coordinate_dim=32, resolution=[8, 8, 8, 5])


def _net(**over):
    from s3gaussian_amd.deformation import deform_network
    from s3gaussian_amd.pipeline import default_hyper
    return deform_network(default_hyper(kplanes_config=SMALL, **over)).deformation_net


def test_fused_route_admits_the_static_configuration():
    assert _net()._fused_ok()
    assert _net(no_dx=True)._fused_ok()


@pytest.mark.parametrize("over", [dict(no_dshs=True), dict(feat_head=False), dict(grid_pe=2), dict(no_ds=False), dict(static_mlp=True)])
def test_fused_route_still_refuses_the_other_switches(over):
    assert not _net(no_dx=True, **over)._fused_ok()
    assert not _net(**over)._fused_ok()


def _stub(net):
    """A model as the guards see it: they read where the Gaussians live, the network's switches and the SH degree."""
    return SimpleNamespace(get_xyz=SimpleNamespace(is_cuda=True, device=torch.device("cpu")), max_sh_degree=3,
                           _deformation=SimpleNamespace(deformation_net=net))


def test_flow_and_decomposition_guards_refuse_a_static_model_without_touching_a_device():
    from s3gaussian_amd import pipeline
    pipe = SimpleNamespace(convert_SHs_python=True)
    assert pipeline._fused_route(_stub(_net()), pipe)                 # the stub passes with a position head ...
    static = _stub(_net(no_dx=True))
    assert not pipeline._fused_route(static, pipe)                    # ... and only the missing head turns it away
    cams = [{"time": float(i // 3)} for i in range(6)]
    with pytest.raises(RuntimeError, match="no_dx"):
        pipeline.render_flows(static, cams, pipe, None, num_cams=3)
    for key in ("forward_flows", "backward_flows", "dynamic_rgbs", "static_rgbs"):
        with pytest.raises(RuntimeError, match="no_dx"):
            pipeline.evaluate_video(static, cams, [None] * 6, pipe, None, num_cams=3, keys=("rgbs", key))
