"""Stacked views (ScorpGs3dInputs.num_views) and the scoring render (scorp_gs2d_render_score) of the 2DGS path, and the
surfel rotation sweep built on them."""
import copy
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def fresh_pair_policy():
    from scorp_amd.rasterizer3d import PairPolicy
    PairPolicy.reset()
    yield
    PairPolicy.reset()


def surfel_model(dev, n, deg, seed, **kw):
    from scorp_amd.renderer2d import GaussianModel2D
    from scorp_amd.synthetic import make_gaussians
    m = GaussianModel2D.from_raw(make_gaussians(n, deg, seed, scale_dims=2, **kw), deg, device=dev)
    m.active_sh_degree = deg
    return m


def single_view(m, stack, bg, view, proj, campos):
    """One view through scorp_gs2d_preprocess + scorp_gs2d_render_image (the pre-existing single-view path: nothing to
    differentiate, so the raw-leaf rasterizer takes the image-only render) with the given matrices."""
    from scorp_amd.rasterizer2d import GaussianRasterizationSettings, rasterize_surfels_raw
    s = GaussianRasterizationSettings(image_height=stack.H, image_width=stack.W, tanfovx=stack.tanfovx, tanfovy=stack.tanfovy, bg=bg,
                                      scale_modifier=1.0, viewmatrix=view.contiguous(), projmatrix=proj.contiguous(),
                                      sh_degree=m.active_sh_degree, campos=campos.contiguous(), prefiltered=False, debug=False)
    with torch.no_grad():
        xyz = m.get_xyz
        return rasterize_surfels_raw(xyz, torch.zeros_like(xyz), *m.raw_leaves(), s)    # (color, radii, allmap)


def six_cameras(dev, W=168, H=96):
    """Five ring cameras, one of them close enough that surfels straddle the top and bottom image edges, and a sixth
    that looks away from the object (an empty band)."""
    from scorp_amd.camera import look_at_camera
    from scorp_amd.synthetic import ring_cameras
    cams = ring_cameras(5, W, H, 3, radius=3.0, device=dev)
    fov = cams[0].FoVx
    th = 2 * math.pi * 2 / 5
    cams[2] = look_at_camera((1.2 * math.cos(th), 1.2 * math.sin(th), 0.2), (0, 0, 0), (0, 0, 1), fov, (W, H), device=dev, uid=2)
    cams.append(look_at_camera((3.0, 0.0, 0.5), (6.0, 0.0, 1.0), (0, 0, 1), fov, (W, H), device=dev, uid=5))
    return cams


def assert_stack_equals_singles(m, stack, bg, view, proj, campos, empty_band=None):
    from scorp_amd.multiview import render_stacked
    V, H, W, N = stack.V, stack.H, stack.W, m.get_xyz.shape[0]
    out = render_stacked(m, stack, bg, view, proj, campos)
    assert set(out) == {"render", "allmap", "radii", "num_pairs"}
    assert out["render"].shape == (3, V * H, W) and out["allmap"].shape == (7, V * H, W) and out["radii"].shape == (V, N)
    seen = 0
    for v in range(V):
        color, radii, allmap = single_view(m, stack, bg, view[v], proj[v], campos[v])
        rows = slice(v * H, (v + 1) * H)
        assert torch.equal(out["render"][:, rows], color), f"colour of view {v}"
        for c in range(7):
            assert torch.equal(out["allmap"][c, rows], allmap[c]), f"allmap channel {c} of view {v}"
        assert torch.equal(out["radii"][v], radii), f"radii of view {v}"
        seen += int((radii > 0).sum())
        if v == empty_band:
            assert int((radii > 0).sum()) == 0
            assert torch.equal(out["render"][:, rows], bg.view(3, 1, 1).expand(3, H, W))
            assert not out["allmap"][:, rows].any()
        else:
            assert int((radii > 0).sum()) > 0 and float(allmap[1].max()) > 0.0, f"view {v} shows nothing"
    return out, seen


def test_stacked_surfel_views_equal_single_views_bit_for_bit(dev):
    """V views of one surfel model as ONE stacked image (V x N virtual surfels, V x H rows) equal the V single
    scorp_gs2d_render_image renders bit for bit - colour, the seven allmap channels, radii: the records keep each view's
    own pixel coordinates, so the arithmetic is the same.  5 000 SH-3 surfels in the training layout (19 full LIN
    workgroups and a 136-row tail), 168 x 96 (a half-wide last tile column, six tile rows per band), a close camera whose
    surfels straddle the top and bottom edges of its band, an empty band; then 200 SH-0 surfels (one partial workgroup);
    then replaced matrices (ViewStack.moved).  On the code before stacked surfel views this cannot pass: the 2DGS path
    ignored num_views."""
    from scorp_amd.multiview import ViewStack
    bg = torch.tensor([0.3, 0.1, 0.2], device=dev)
    cams = six_cameras(dev)
    stack = ViewStack(cams, dev)
    assert (stack.V, stack.W, stack.H) == (6, 168, 96)
    m = surfel_model(dev, 5000, 3, 7, extent=1.0, log_scale_mean=math.log(0.04))
    out, _ = assert_stack_equals_singles(m, stack, bg, stack.view, stack.proj, stack.campos, empty_band=5)
    # the close camera's band has surfels on its first and on its last pixel row: they straddle the band's edges
    close = out["allmap"][1, 2 * 96:3 * 96]
    assert float(close[0].max()) > 0.0 and float(close[-1].max()) > 0.0
    small = surfel_model(dev, 200, 0, 11, extent=1.0, log_scale_mean=math.log(0.08))
    assert_stack_equals_singles(small, stack, bg, stack.view, stack.proj, stack.campos, empty_band=5)
    # replaced matrices: the cameras as seen from an object that was rotated about its centre
    rots = np.load(os.path.join(GOLDEN, "rotations_128.npz"))["rotations"]
    R = torch.tensor(rots[17], dtype=torch.float32, device=dev)
    c = m._xyz.detach().mean(0)
    view, proj, campos = stack.moved(R, c - c @ R.T)
    assert not torch.equal(view, stack.view)
    assert_stack_equals_singles(m, stack, bg, view, proj, campos, empty_band=5)   # (a rotation about the centre: still out of sight)


@pytest.mark.parametrize("depth_ratio", [0.0, 0.5, 1.0])
def test_surfel_scoring_render_equals_render_then_score_and_is_bit_repeatable(dev, depth_ratio):
    """scorp_gs2d_render_score (no colour, no normals, no images; the comparison with the target in the epilogue, per-block
    sums added in a fixed order) against the float64 sum of the float32 per-pixel terms formed in torch from
    render_stacked's maps - which the test above holds to the single-view kernel.  Two hypotheses x three views in one
    launch set, band 0 is the target itself.  2e-6 relative: the bound of the 3-D twin for the same reduction tree (only
    the order of the float32 sums differs)."""
    from scorp_amd.multiview import ViewStack, render_stacked, score_stacked, surfel_alpha_depth
    from scorp_amd.rasterizer3d import PairPolicy
    from scorp_amd.synthetic import ring_cameras
    m = surfel_model(dev, 4000, 0, 5, log_scale_mean=math.log(0.05))
    cams = ring_cameras(5, 112, 80, 3, radius=3.4, device=dev)
    bg = torch.zeros(3, device=dev)
    a_t, d_t = surfel_alpha_depth(render_stacked(m, ViewStack(cams[:3], dev), bg)["allmap"], depth_ratio)    # the target: views 0..2
    a_t, d_t = a_t.contiguous(), d_t.contiguous()
    assert float(a_t.max()) > 0.5 and float(d_t.max()) > 1.0
    stack6 = ViewStack([cams[0], cams[1], cams[2], cams[2], cams[3], cams[4]], dev)   # band 0 == the target, band 1 not
    alpha, depth = surfel_alpha_depth(render_stacked(m, stack6, bg)["allmap"], depth_ratio)
    n = a_t.numel()
    terms = ((alpha.view(2, -1) - a_t.view(1, -1)).abs() + (depth.view(2, -1) - d_t.view(1, -1)).abs())     # float32, per pixel
    assert terms.dtype == torch.float32
    ref = terms.double().sum(1) / n
    PairPolicy.mode = "reserve"
    got = []
    for _ in range(2):
        acc = torch.zeros(2, device=dev)
        score_stacked(m, stack6, bg, stack6.view, stack6.proj, stack6.campos, d_t, a_t, acc, 3 * stack6.H, 1.0 / n,
                      depth_ratio=depth_ratio)
        got.append(acc)
    PairPolicy.drain()
    err = (got[0].double() - ref).abs().max()
    print(f"depth_ratio {depth_ratio}: acc {got[0].tolist()} ref {ref.tolist()} |acc - ref| {float(err):.3e}")
    assert torch.equal(got[0], got[1]), "two scoring renders differ"
    assert float(got[0][0]) <= 1e-7 and float(got[0][1]) > 1e-3, got[0]          # band 0 IS the target, band 1 is not
    assert float(err) <= 2e-6 * max(float(ref.abs().max()), 1.0), (got[0], ref)


def sweep_object(dev):
    m = surfel_model(dev, 3000, 0, 5, extent=0.8, log_scale_mean=math.log(0.03))
    with torch.no_grad():
        m._xyz[:, 0] *= 1.6          # an elongated, asymmetric cloud: rotations are distinguishable
        m._xyz[:, 2] *= 0.5
        m._xyz[: 1000, 1] += 0.6
    return m


@pytest.mark.parametrize("depth_ratio", [0.0, 1.0])
def test_surfel_rotation_sweep_recovers_the_planted_rotation(dev, depth_ratio):
    """The 128-rotation sweep of a surfel object: the caller hands over the model and nothing else, the plan takes the
    stacked scoring path (cameras moved, views stacked, scorp_gs2d_render_score), and the eager form (object rotated)
    finds the same rotation.  The largest difference between the two forms' fitness is printed, not asserted: it holds
    pixels whose alpha crosses 1/255 and, at depth_ratio 1, pixels whose median surfel changes."""
    from scorp_amd import renderer2d
    from scorp_amd.align import SweepPlan, render_views, rotation_sweep
    from scorp_amd.rasterizer3d import _GS2D
    from scorp_amd.synthetic import ring_cameras
    from scorp_amd.transforms import gaussians_rotate
    rots = np.load(os.path.join(GOLDEN, "rotations_128.npz"))["rotations"]
    m = sweep_object(dev)
    cams = ring_cameras(6, 128, 128, 9, radius=3.0, device=dev)
    bg = torch.zeros(3, device=dev)
    planted = 93
    tgt_model = copy.copy(m)
    tgt_model._xyz, tgt_model._rotation = m._xyz.detach().clone(), m._rotation.detach().clone()
    tgt_model._features_rest = m._features_rest.detach().clone()
    gaussians_rotate(tgt_model, torch.tensor(rots[planted], dtype=torch.float32, device=dev), fix_center=True)
    targets = render_views(tgt_model, cams, bg, render_fn=renderer2d.render, depth_ratio=depth_ratio)
    plan = SweepPlan(m, cams, targets, bg, depth_ratio=depth_ratio)
    assert plan.stacked is not None and plan.stacked.kind is _GS2D and plan.stacked.depth_ratio == depth_ratio
    assert plan.render_fn is renderer2d.render and plan.graph is None
    ids, fit, best = rotation_sweep(m, rots, cams, targets, bg, plan=plan)
    assert ids.numel() == 128 and best == planted
    ids_e, fit_e, best_e = rotation_sweep(m, rots, cams, targets, bg, use_graph=False, depth_ratio=depth_ratio)   # object rotated, eager
    assert best_e == planted and torch.equal(ids, ids_e)
    print(f"depth_ratio {depth_ratio}: fit[planted] {float(fit[planted, 0]):.3e} runner-up {float(fit[:, 0].sort().values[-2]):.3e} "
          f"max |fit - fit_e| {float((fit - fit_e).abs().max()):.3e}")
    assert torch.equal(tgt_model._features_dc, m._features_dc)    # the model itself is untouched by the sweep
