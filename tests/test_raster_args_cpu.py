"""The two argument checks of the reference's GaussianRasterizer.forward, on every public entry point of the rasterizer module that
takes the same optional tensors: the reference's own exception texts ("excatly" included), raised before any library call."""
import pytest
import torch

COLOURS = "excatly one of either SHs or precomputed colors"
COVARIANCE = "exactly one of either scale/rotation pair or precomputed 3D covariance"
P = 4


def _rasterizer():
    import diff_gaussian_rasterization as d
    return d.GaussianRasterizer(d.GaussianRasterizationSettings(
        image_height=16, image_width=16, tanfovx=1.0, tanfovy=1.0, bg=torch.zeros(3), scale_modifier=1.0, viewmatrix=torch.eye(4),
        projmatrix=torch.eye(4), sh_degree=0, campos=torch.zeros(3), prefiltered=False, debug=False))


def _call(name, **kw):
    r = _rasterizer()
    x, op = torch.zeros(P, 3), torch.zeros(P, 1)
    if name == "forward_decomposed":
        return r.forward_decomposed(means3D=x, opacities=op, dynamic_mask=torch.zeros(P, dtype=torch.bool), **kw)
    if name == "forward_pair":
        return r.forward_pair(means3D=x, means2D=x, opacities=op, colors_a=x, colors_b=x, **kw)
    return getattr(r, name)(means3D=x, means2D=x, opacities=op, **kw)


@pytest.fixture
def no_library_call(monkeypatch):
    from s3gaussian_amd import raster_C

    def reached(*a, **k):
        pytest.fail("the argument check must come before the library call")

    monkeypatch.setattr(raster_C, "rasterize_gaussians", reached)


SR = dict(scales=torch.zeros(P, 3), rotations=torch.zeros(P, 4))


@pytest.mark.parametrize("name", ["forward", "forward_alpha", "forward_decomposed"])
@pytest.mark.parametrize("colours", ["both", "neither"])
def test_colour_sources_are_checked_first(no_library_call, name, colours):
    kw = dict(shs=torch.zeros(P, 1, 3), colors_precomp=torch.zeros(P, 3)) if colours == "both" else {}
    with pytest.raises(Exception, match=COLOURS):
        _call(name, **kw, **SR)


@pytest.mark.parametrize("name", ["forward", "forward_alpha", "forward_decomposed", "forward_pair"])
@pytest.mark.parametrize("geometry", ["scales_only", "pair_and_covariance", "nothing"])
def test_covariance_sources_are_checked(no_library_call, name, geometry):
    kw = {"scales_only": dict(scales=SR["scales"]), "pair_and_covariance": dict(cov3D_precomp=torch.zeros(P, 6), **SR),
          "nothing": {}}[geometry]
    if name != "forward_pair":          # forward_pair takes two sets of precomputed colours and nothing else
        kw["colors_precomp"] = torch.zeros(P, 3)
    with pytest.raises(Exception, match=COVARIANCE):
        _call(name, **kw)
