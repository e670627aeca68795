"""Fused HexPlane sampler + deformation module (HIP) vs the reference's own modules (golden fixture generated from
/root/reference in-container) and vs the plain-PyTorch restatement on random inputs.
Tolerances: features/outputs rtol 1e-5 (same op order as torch.grid_sample, contraction off); plane gradients are
sums of float atomics in arbitrary order: relative L2 <= 1e-5."""
import os

import numpy as np
import pytest
import torch

from tests.util import rel_l2

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _golden_nets(dev):
    from oracle import hexplane_ref as hr
    from s3gaussian_amd.deformation import deform_network
    z = np.load(os.path.join(GOLD, "hexplane_deform.npz"))
    hyper = hr.default_hyper(kplanes_config=dict(grid_dimensions=2, input_coordinate_dim=4, output_coordinate_dim=32,
                                                 resolution=[8, 8, 8, 5]), multires=[1, 2])
    sd = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd::")}
    net = deform_network(hyper)
    net.deformation_net.set_aabb(z["aabb"][0].tolist(), z["aabb"][1].tolist())
    net.load_state_dict(sd, strict=True)   # reference state_dict loads into the accelerated module unchanged
    return net.to(dev), z


def test_deform_network_matches_reference_golden(gpu_device):
    net, z = _golden_nets(gpu_device)
    t = lambda k: torch.from_numpy(z[k]).to(gpu_device)
    for p in net.deformation_net.grid.grids.parameters():
        assert p.is_contiguous(memory_format=torch.channels_last) and p.dim() == 4 and p.shape[:2] == (1, 32)
    xyz = t("xyz").clone().requires_grad_(True)
    shs = t("shs").clone().requires_grad_(True)
    feat = net.deformation_net.grid(xyz.detach(), t("time"))
    np.testing.assert_allclose(feat.detach().cpu().numpy(), z["hexplane_features"], rtol=1e-5, atol=1e-6)
    outs = net(xyz, t("scales"), t("rotations"), t("opacity"), shs, t("time"))
    names = ["means3D", "scales", "rotations", "opacity", "shs", "dx", "feat", "dshs"]
    loss = 0
    for n, o in zip(names, outs):
        np.testing.assert_allclose(o.detach().cpu().numpy(), z["out_" + n], rtol=1e-4, atol=2e-5)
        loss = loss + (o * t("w_" + n)).sum()
    loss.backward()
    assert rel_l2(xyz.grad.cpu().numpy(), z["grad_xyz"]) < 1e-4
    assert rel_l2(shs.grad.cpu().numpy(), z["grad_shs"]) < 1e-5
    for k, p in net.named_parameters():
        if "grad::" + k in z.files:
            assert rel_l2(p.grad.cpu().numpy(), z["grad::" + k]) < 1e-4, k
        else:
            assert p.grad is None, k


@pytest.mark.parametrize("tmode", ["per_point", 0.37, 1.0, -1.0, -1.4, 0.9999, "hint_false"])
@pytest.mark.parametrize("P", [1, 7, 8, 1000])
def test_sampler_vs_restatement_random(gpu_device, P, tmode):
    """Default-resolution field ([64,64,64,25] x [1,2,4,8]); points partly OUTSIDE the aabb (border clamp + zero grad).
    tmode: per-point random times (general 4-tap path), or ONE timestamp for all points -- interior, on both borders,
    outside, just inside the last row -- which takes the uniform-time path (time planes pre-interpolated to row tables,
    auto-detected); "hint_false" = uniform data forced through the general path."""
    from oracle import hexplane_ref as hr
    from s3gaussian_amd.hexplane import HexPlaneField
    torch.manual_seed(P)
    cfg = dict(grid_dimensions=2, input_coordinate_dim=4, output_coordinate_dim=32, resolution=[64, 64, 64, 25])
    ref = hr.HexPlaneField(1.6, cfg, [1, 2, 4, 8])
    with torch.no_grad():
        for p in ref.grids.parameters():
            p.add_(0.3 * torch.randn_like(p))
    ref.set_aabb([3.0, 2.0, 1.5], [-2.0, -2.5, -1.0])
    mine = HexPlaneField(1.6, cfg, [1, 2, 4, 8])
    mine.set_aabb([3.0, 2.0, 1.5], [-2.0, -2.5, -1.0])
    mine.load_state_dict(ref.state_dict())
    mine = mine.to(gpu_device)
    xyz = (torch.rand(P, 3) * torch.tensor([6.0, 5.5, 3.5]) + torch.tensor([-2.5, -3.0, -1.5]))
    time = torch.rand(P, 1) if tmode == "per_point" else torch.full((P, 1), 0.25 if tmode == "hint_false" else float(tmode))
    hint = False if tmode == "hint_false" else None
    w = torch.randn(P, 128)
    xr = xyz.clone().requires_grad_(True)
    fr = ref(xr, time)
    (fr * w).sum().backward()
    xg = xyz.to(gpu_device).requires_grad_(True)
    fg = mine(xg, time.to(gpu_device), uniform_time=hint)
    (fg * w.to(gpu_device)).sum().backward()
    np.testing.assert_allclose(fg.detach().cpu().numpy(), fr.detach().numpy(), rtol=2e-5, atol=1e-6)
    assert rel_l2(xg.grad.cpu().numpy(), xr.grad.numpy()) < 1e-4
    for (k, pr), (_, pg) in zip(ref.named_parameters(), mine.named_parameters()):
        if pr.grad is not None:
            assert rel_l2(pg.grad.cpu().numpy(), pr.grad.numpy()) < 1e-5, k


def test_stale_spatial_order_is_only_a_performance_matter(gpu_device):
    """The backward re-sorts the points only every SORT_REFRESH passes.  A second, completely different point set of the
    same size pushed through the same field walks in the FIRST set's (now meaningless) order: results must still match."""
    from oracle import hexplane_ref as hr
    from s3gaussian_amd.hexplane import HexPlaneField
    torch.manual_seed(3)
    cfg = dict(grid_dimensions=2, input_coordinate_dim=4, output_coordinate_dim=32, resolution=[16, 16, 16, 7])
    ref = hr.HexPlaneField(1.6, cfg, [1, 2, 4])
    with torch.no_grad():
        for p in ref.grids.parameters():
            p.add_(0.3 * torch.randn_like(p))
    mine = HexPlaneField(1.6, cfg, [1, 2, 4])
    mine.load_state_dict(ref.state_dict())
    mine = mine.to(gpu_device)
    P = 3000
    for it in range(3):
        xyz = torch.rand(P, 3) * 3.0 - 1.5
        time = torch.full((P, 1), 0.1 * it)
        w = torch.randn(P, 96)
        for m in (ref, mine):
            for p in m.parameters():
                p.grad = None
        xr = xyz.clone().requires_grad_(True)
        (ref(xr, time) * w).sum().backward()
        xg = xyz.to(gpu_device).requires_grad_(True)
        fg = mine(xg, time.to(gpu_device))
        (fg * w.to(gpu_device)).sum().backward()
        assert mine._order_cache["sort_age"] == it          # sorted on pass 0, reused afterwards
        assert rel_l2(xg.grad.cpu().numpy(), xr.grad.numpy()) < 1e-4
        for (k, pr), (_, pg) in zip(ref.named_parameters(), mine.named_parameters()):
            if pr.grad is not None:
                assert rel_l2(pg.grad.cpu().numpy(), pr.grad.numpy()) < 1e-5, (it, k)


@pytest.mark.parametrize("use", ["both", "features_only", "reg_only"])
def test_regulariser_on_the_sampler_node_matches_separate_nodes(gpu_device, use):
    """field(xyz, t, reg_weights=...) -> (features, compute_regulation value) as ONE autograd node (the regulariser's
    gradient seeds the buffer the sampler's backward accumulates into) vs the two separate nodes autograd would add."""
    from s3gaussian_amd.hexplane import HexPlaneField
    from s3gaussian_amd.losses import plane_regulation
    torch.manual_seed(5)
    cfg = dict(grid_dimensions=2, input_coordinate_dim=4, output_coordinate_dim=32, resolution=[16, 16, 16, 9])
    field = HexPlaneField(1.6, cfg, [1, 2]).to(gpu_device)
    with torch.no_grad():
        for p in field.grids.parameters():
            p.add_(0.3 * torch.randn_like(p))
    P = 2000
    xyz = (torch.rand(P, 3) * 3.0 - 1.5).to(gpu_device)
    time = torch.full((P, 1), 0.3, device=gpu_device)
    w = torch.randn(P, 64, device=gpu_device)
    regw = (0.01, 0.0001, 0.0002)
    res = []
    for fused in (True, False):
        for p in field.parameters():
            p.grad = None
        x = xyz.clone().requires_grad_(True)
        if fused:
            feat, reg = field(x, time, uniform_time=True, reg_weights=regw)
        else:
            feat = field(x, time, uniform_time=True)
            reg = plane_regulation(field.grids, *regw)
        loss = 0
        if use != "reg_only":
            loss = loss + (feat * w).sum()
        if use != "features_only":
            loss = loss + 700.0 * reg
        loss.backward()
        res.append((feat.detach(), reg.detach(), x.grad, [p.grad for p in field.grids.parameters()]))
    (f1, r1, gx1, gp1), (f2, r2, gx2, gp2) = res
    assert torch.equal(f1, f2) and abs(r1.item() - r2.item()) <= 1e-6 * abs(r2.item())
    if use == "reg_only":
        assert gx1 is None and gx2 is None
    else:
        assert rel_l2(gx1.cpu().numpy(), gx2.cpu().numpy()) < 1e-5
    for a, b in zip(gp1, gp2):
        if use == "features_only" and b is None:
            assert a is None or float(a.abs().max()) == 0.0
            continue
        assert a.is_contiguous(memory_format=torch.channels_last)
        assert rel_l2(a.cpu().numpy(), b.cpu().numpy()) < 1e-5


@pytest.mark.parametrize("variant", ["grid_pe", "static_mlp", "empty_voxel", "apply_rotation", "all_heads", "no_dx_no_dshs"])
def test_non_default_deformation_switches_match_reference_golden(gpu_device, variant):
    """grid_pe / static_mlp / empty_voxel / apply_rotation / every head on / dx+dshs off: outputs and dL/dxyz of
    s3gaussian_amd.deformation against tests/golden/deform_switches.npz, produced by the reference's own
    scene/deformation.py (tests/golden/make_golden.py).  These configurations run the fused HexPlane sampler with
    library GEMMs for the heads."""
    import importlib.util
    from s3gaussian_amd.deformation import deform_network
    from s3gaussian_amd.pipeline import default_hyper
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(os.path.dirname(__file__), "golden", "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "deform_switches.npz"))
    over = mg.SWITCH_VARIANTS[variant]
    hyper = default_hyper(kplanes_config=dict(grid_dimensions=2, input_coordinate_dim=4, output_coordinate_dim=32,
                                              resolution=[4, 4, 4, 3]), multires=[1, 2], **over)
    net = deform_network(hyper)
    sd = {k.split("::sd::")[1]: torch.from_numpy(z[k]) for k in z.files if k.startswith(variant + "::sd::")}
    if over.get("empty_voxel"):
        sd["deformation_net.empty_voxel.grid"] = mg.empty_voxel_pattern()
    net.deformation_net.set_aabb([2.0, 1.5, 1.0], [-1.0, -1.5, -0.5])
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert not unexpected and all("empty_voxel.xyz" in k for k in missing), (missing, unexpected)
    net = net.to(gpu_device)
    if over.get("empty_voxel"):
        net.deformation_net.set_aabb([2.0, 1.5, 1.0], [-1.0, -1.5, -0.5])   # buffers on the device
    t = lambda k: torch.from_numpy(z[f"{variant}::{k}"]).to(gpu_device)
    xyz = t("xyz").clone().requires_grad_(True)
    outs = net(xyz, t("scales"), t("rotations"), t("opacity"), t("shs"), t("time"))
    names = ["means3D", "scales", "rotations", "opacity", "shs", "dx", "feat", "dshs"]
    loss = 0
    for n, o in zip(names, outs):
        key = f"{variant}::out_{n}"
        if o is None:
            assert key not in z.files, n
            continue
        np.testing.assert_allclose(o.detach().cpu().numpy(), z[key], rtol=1e-4, atol=3e-5, err_msg=n)
        loss = loss + (o * t("w_" + n)).sum()
    loss.backward()
    assert rel_l2(xyz.grad.cpu().numpy(), z[f"{variant}::grad_xyz"]) < 1e-4


@pytest.mark.parametrize("mode", ["slab", "slab_product"])
@pytest.mark.parametrize("tmode", ["per_point", 0.37])
def test_exact_zero_samples_take_the_exact_fallback(gpu_device, tmode, mode, monkeypatch):
    """The backward forms dL/d(sample_i) as dL/dfeature * feature / sample_i.  Samples that are exactly zero (a zeroed plane
    region, a whole zero plane, a zero time plane) or tiny cannot be divided by: those (point, level, plane) entries must
    come out of the exact fix-up pass with the same gradients as autograd gives the reference.  "slab" is the default (round 4: the
    per-point pass divides too -- its dL/dxyz of such samples comes from exact_du --), "slab_product" the product-rule pass that
    stays as the exact fallback needing nothing from the forward (the slab-free "walk" of rounds 2-4 was removed in round 5)."""
    from oracle import hexplane_ref as hr
    from s3gaussian_amd.hexplane import HexPlaneField
    from s3gaussian_amd import hexplane as hx
    monkeypatch.setattr(hx, "BACKWARD_MODE", mode)
    torch.manual_seed(11)
    cfg = dict(grid_dimensions=2, input_coordinate_dim=4, output_coordinate_dim=32, resolution=[16, 16, 16, 6])
    ref = hr.HexPlaneField(1.6, cfg, [1, 2, 4, 8])
    with torch.no_grad():
        for p in ref.grids.parameters():
            p.add_(0.3 * torch.randn_like(p))
        ref.grids[0][0][:, :, 3:9, 2:11] = 0.0         # a zero block in the (x,y) plane of level 0
        ref.grids[1][3].zero_()                         # the whole (y,z) plane of level 1
        ref.grids[2][4][:, 5:9].zero_()                 # four channels of the (y,t) plane of level 2
        ref.grids[3][1][:, :, ::2, :] *= 1e-25          # tiny but non-zero samples: division is not trusted there either
    mine = HexPlaneField(1.6, cfg, [1, 2, 4, 8])
    mine.load_state_dict(ref.state_dict())
    mine = mine.to(gpu_device)
    P = 4000
    xyz = torch.rand(P, 3) * 3.6 - 1.8
    time = torch.rand(P, 1) if tmode == "per_point" else torch.full((P, 1), float(tmode))
    w = torch.randn(P, 128)
    xr = xyz.clone().requires_grad_(True)
    (ref(xr, time) * w).sum().backward()
    xg = xyz.to(gpu_device).requires_grad_(True)
    fg = mine(xg, time.to(gpu_device))
    (fg * w.to(gpu_device)).sum().backward()
    assert torch.isfinite(xg.grad).all()
    assert rel_l2(xg.grad.cpu().numpy(), xr.grad.numpy()) < 1e-4
    for (k, pr), (_, pg) in zip(ref.named_parameters(), mine.named_parameters()):
        if pr.grad is not None:
            assert torch.isfinite(pg.grad).all(), k
            assert rel_l2(pg.grad.cpu().numpy(), pr.grad.numpy()) < 1e-5, k


@pytest.mark.parametrize("tmode", ["per_point", 0.37, 1.0])
def test_product_rule_fallback_matches_the_default_backward(gpu_device, tmode, monkeypatch):
    """The two backward algorithms (include/s3g_hexplane.h: `features` given = S3G_HEX_SLAB_DIV, NULL = S3G_HEX_SLAB) on the
    default-resolution field: same dL/dxyz and plane gradients to fp32 round-off (1e-5 relative); and the removed algorithm id is
    refused with an error, not silently mapped."""
    from s3gaussian_amd import hexplane as hx
    torch.manual_seed(5)
    cfg = dict(grid_dimensions=2, input_coordinate_dim=4, output_coordinate_dim=32, resolution=[64, 64, 64, 25])
    f = hx.HexPlaneField(1.6, cfg, [1, 2, 4, 8])
    with torch.no_grad():
        for p in f.parameters():
            if p.requires_grad:
                p.add_(0.3 * torch.randn_like(p))
    f = f.to(gpu_device)
    P = 50_000
    xyz = (torch.rand(P, 3) * 3.6 - 1.8).to(gpu_device)
    time = (torch.rand(P, 1) if tmode == "per_point" else torch.full((P, 1), float(tmode))).to(gpu_device)
    w = torch.randn(P, 128).to(gpu_device)
    res = {}
    for mode in ("slab", "slab_product"):
        monkeypatch.setattr(hx, "BACKWARD_MODE", mode)
        for p in f.parameters():
            p.grad = None
        x = xyz.clone().requires_grad_(True)
        (f(x, time) * w).sum().backward()
        res[mode] = (x.grad.clone(), [p.grad.clone() for p in f.parameters() if p.requires_grad])
    for other in ("slab_product",):
        assert rel_l2(res[other][0].cpu().numpy(), res["slab"][0].cpu().numpy()) < 1e-5, other
        for a, b in zip(res[other][1], res["slab"][1]):
            assert rel_l2(a.cpu().numpy(), b.cpu().numpy()) < 1e-5, other


def test_every_walk_order_is_sorted_by_its_own_levels_cells(gpu_device):
    """Round 4: the scatter walks every (orientation, level) in an order sorted by THAT level's (major, minor) texel cells
    (csrc/hexplane_bwd.hpp::sort_cell, csrc/hexplane_sort.hip::order_key; sort_state layout in include/s3g_hexplane.h).  A wrong key would not change any result
    -- the orders only steer the walks -- it would silently bring back the flush storm, so the orders themselves are checked: keys
    recomputed here in the kernel's fp32 arithmetic must be non-decreasing along every order, every order must be a permutation,
    and comp must be the composition with the processing order."""
    from s3gaussian_amd import hexplane as hx
    torch.manual_seed(3)
    cfg = dict(grid_dimensions=2, input_coordinate_dim=4, output_coordinate_dim=32, resolution=[64, 64, 64, 25])
    f = hx.HexPlaneField(1.6, cfg, [1, 2, 4, 8])
    f.set_aabb([30.0, 12.0, 6.0], [-10.0, -12.0, -2.0])
    f = f.to(gpu_device)
    P = 200_000
    g = torch.Generator().manual_seed(1)
    xyz = (torch.rand(P, 3, generator=g) * torch.tensor([44.0, 26.0, 9.0]) + torch.tensor([-12.0, -13.0, -2.5])).to(gpu_device)   # some outside
    x = xyz.clone().requires_grad_(True)
    (f(x, torch.full((P, 1), 0.4, device=gpu_device), uniform_time=True) ** 2).sum().backward()
    L = len(f.resolutions)
    words = hx.sort_state_words(L)
    assert words == 6 * L + 1
    st = f._order_cache["sort_state"].view(words, P).long()
    order, comp, proc = st[:3 * L], st[3 * L:6 * L], st[6 * L]
    everyone = torch.arange(P, device=gpu_device)
    assert torch.equal(torch.sort(proc).values, everyone)
    procrank = torch.empty_like(proc)
    procrank[proc] = everyone
    amax, amin = f.aabb[0].float(), f.aabb[1].float()
    u = (xyz - amax) * (2.0 / (amin - amax)) - 1.0                         # point_coords(), fp32 like the kernel

    def cell(axis, W):
        ix = ((u[:, axis] + 1.0) / 2.0) * float(W - 1)
        return torch.clamp(ix, 0.0, float(W - 1)).floor().long()

    MAJ, MIN_ = [0, 1, 2], [1, 2, 0]
    for o in range(3):
        for l in range(L):
            oi = o * L + l
            W_major, W_minor = f.resolutions[l][MAJ[o]], f.resolutions[l][MIN_[o]]
            key = cell(MAJ[o], W_major) * 512 + cell(MIN_[o], W_minor)
            k = key[order[oi]]
            assert torch.equal(torch.sort(order[oi]).values, everyone), (o, l)
            assert int((k[1:] < k[:-1]).sum()) == 0, (o, l)                   # monotone in its OWN level's cells
            assert torch.equal(comp[oi], procrank[order[oi]]), (o, l)
    # and the coarse levels are NOT monotone in the finest level's order: that is what rounds 1-3 walked
    fine = cell(0, f.resolutions[L - 1][0]) * 512 + cell(1, f.resolutions[L - 1][1])
    coarse_in_fine_order = (cell(0, f.resolutions[0][0]) * 512 + cell(1, f.resolutions[0][1]))[order[L - 1]]
    assert int((fine[order[L - 1]][1:] < fine[order[L - 1]][:-1]).sum()) == 0
    assert int((coarse_in_fine_order[1:] < coarse_in_fine_order[:-1]).sum()) > 100


@pytest.fixture
def deterministic_mode():
    from s3gaussian_amd import hexplane
    prev = hexplane.set_deterministic(True)
    yield
    hexplane.set_deterministic(prev)


@pytest.mark.parametrize("P", [1, 7, 255, 257, 3000, 70_001, 600_000])
def test_deterministic_mode_matches_the_reference_arithmetic_and_is_bit_reproducible(gpu_device, P, deterministic_mode):
    """VERDICT r5 weak #1 / next #3.  include/s3g_hexplane.h::s3g_hexplane_set_deterministic: stable walk orders, run records instead of
    float atomics, a stencil gather in fixed order.  (1) Same gradients as the reference's arithmetic (the bars of
    test_sampler_vs_restatement_random) with points partly outside the aabb, cells that straddle walker segments (at P = 600 000 the
    coarsest level holds ~150 points per cell, the row tables thousands per cell) and empty cells; (2) three fresh fields built from
    the same state give BIT-IDENTICAL plane gradients, dL/dxyz and walk orders; (3) the default mode agrees with it to round-off."""
    from oracle import hexplane_ref as hr
    from s3gaussian_amd import hexplane
    from s3gaussian_amd.hexplane import HexPlaneField
    torch.manual_seed(P)
    cfg = dict(grid_dimensions=2, input_coordinate_dim=4, output_coordinate_dim=32, resolution=[64, 64, 64, 25])
    ref = hr.HexPlaneField(1.6, cfg, [1, 2, 4, 8])
    with torch.no_grad():
        for p in ref.grids.parameters():
            p.add_(0.3 * torch.randn_like(p))
    ref.set_aabb([3.0, 2.0, 1.5], [-2.0, -2.5, -1.0])
    xyz = (torch.rand(P, 3) * torch.tensor([6.0, 5.5, 3.5]) + torch.tensor([-2.5, -3.0, -1.5]))
    time = torch.full((P, 1), 0.37)
    w = torch.randn(P, 128)
    dev = gpu_device

    def run(det):
        hexplane.set_deterministic(det)
        mine = HexPlaneField(1.6, cfg, [1, 2, 4, 8])
        mine.set_aabb([3.0, 2.0, 1.5], [-2.0, -2.5, -1.0])
        mine.load_state_dict(ref.state_dict())
        mine = mine.to(dev)
        outs = []
        for it in range(2):           # the second pass reuses the cached orders
            for p in mine.parameters():
                p.grad = None
            xg = xyz.to(dev).requires_grad_(True)
            fg = mine(xg, time.to(dev), uniform_time=True)
            (fg * w.to(dev)).sum().backward()
            outs.append((xg.grad.clone(), [p.grad.clone() for p in mine.grids.parameters()], mine._order_cache["sort_state"].clone()))
        return outs

    a, b, c = run(True), run(True), run(True)
    for other in (b, c):
        for (gx0, gp0, st0), (gx1, gp1, st1) in zip(a, other):
            assert torch.equal(st0, st1)                                   # stable sorts: the orders themselves are reproducible
            assert torch.equal(gx0, gx1)
            for i, (x, y) in enumerate(zip(gp0, gp1)):
                assert torch.equal(x, y), i
    for x, y in zip(a[0][1], a[1][1]):
        assert torch.equal(x, y)                                           # and the pass on cached orders equals the first
    if P <= 70_001:      # against the reference's arithmetic on the host (the big size is held to the default mode below)
        xr = xyz.clone().requires_grad_(True)
        (ref(xr, time) * w).sum().backward()
        assert rel_l2(a[0][0].cpu().numpy(), xr.grad.numpy()) < 1e-4
        for (k, pr), pg in zip(ref.grids.named_parameters(), a[0][1]):
            assert rel_l2(pg.cpu().numpy(), pr.grad.numpy()) < 1e-5, k
    d = run(False)
    for i, (x, y) in enumerate(zip(a[0][1], d[0][1])):
        assert rel_l2(x.cpu().numpy(), y.cpu().numpy()) < 2e-6, i
    assert torch.equal(a[0][0], d[0][0])                                   # dL/dxyz comes from the per-point pass: the same in both modes


def test_deterministic_mode_refuses_what_it_cannot_do(gpu_device, deterministic_mode):
    from s3gaussian_amd.hexplane import HexPlaneField
    cfg = dict(grid_dimensions=2, input_coordinate_dim=4, output_coordinate_dim=32, resolution=[16, 16, 16, 7])
    f = HexPlaneField(1.6, cfg, [1, 2]).to(gpu_device)
    xyz = (torch.rand(500, 3, device=gpu_device) * 2 - 1).requires_grad_(True)
    t = torch.rand(500, 1, device=gpu_device)                             # per-point time: the (axis, t) planes are not row tables
    with pytest.raises(Exception, match="uniform_time"):      # (S3G_ERR_INVALID_ARG: the reference's plain Exception for bad argument combinations)
        f(xyz, t, uniform_time=False).sum().backward()


def test_deterministic_mode_re_sorts_for_every_backward(gpu_device, deterministic_mode):
    """The run records of the deterministic mode rely on every cell being CONTIGUOUS in the walk order: that only holds for an order
    sorted on the current coordinates, so the mode must not reuse cached orders (the default walk sums with atomics and is indifferent
    to a stale order: test_stale_spatial_order_is_only_a_performance_matter).  Three different point sets through ONE field."""
    from oracle import hexplane_ref as hr
    from s3gaussian_amd.hexplane import HexPlaneField
    torch.manual_seed(5)
    cfg = dict(grid_dimensions=2, input_coordinate_dim=4, output_coordinate_dim=32, resolution=[16, 16, 16, 7])
    ref = hr.HexPlaneField(1.6, cfg, [1, 2, 4])
    with torch.no_grad():
        for p in ref.grids.parameters():
            p.add_(0.3 * torch.randn_like(p))
    mine = HexPlaneField(1.6, cfg, [1, 2, 4])
    mine.load_state_dict(ref.state_dict())
    mine = mine.to(gpu_device)
    P = 5000
    for it in range(3):
        xyz = torch.rand(P, 3) * 3.0 - 1.5
        time = torch.full((P, 1), 0.1 * it)
        w = torch.randn(P, 96)
        for m in (ref, mine):
            for p in m.parameters():
                p.grad = None
        xr = xyz.clone().requires_grad_(True)
        (ref(xr, time) * w).sum().backward()
        xg = xyz.to(gpu_device).requires_grad_(True)
        (mine(xg, time.to(gpu_device), uniform_time=True) * w.to(gpu_device)).sum().backward()
        assert rel_l2(xg.grad.cpu().numpy(), xr.grad.numpy()) < 1e-4
        for (k, pr), (_, pg) in zip(ref.grids.named_parameters(), mine.grids.named_parameters()):
            assert rel_l2(pg.grad.cpu().numpy(), pr.grad.numpy()) < 1e-5, (it, k)
