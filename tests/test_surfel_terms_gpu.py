"""The late iterations' loss terms (train_2dgs.py:100-139) inside the one-call 2DGS view: the kernels of surfel_terms.hip
against the float64 yardstick (tests/surfel_terms_reference.py), their degenerate cases, scorp_gs2d_train_view_ex against
render() + the torch terms + autograd, the optimizer step inside the view bit for bit, the training loop, and an overflowed
pair reservation with the terms active."""
import math

import pytest
import torch

from tests import surfel_terms_reference as ref

pytestmark = pytest.mark.gpu

NAMES = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")
RATIOS = (0.0, 1.0, 0.5)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _depth_maps(dev, H, W, seed):
    """Sensor = 2 + 2 rand with ~10 % zeros, estimate = rand with ~10 % zeros."""
    g = torch.Generator(device=dev).manual_seed(seed)
    sensor = 2.0 + 2.0 * torch.rand(1, H, W, device=dev, generator=g)
    sensor[torch.rand(1, H, W, device=dev, generator=g) < 0.1] = 0.0
    est = torch.rand(1, H, W, device=dev, generator=g)
    est[torch.rand(1, H, W, device=dev, generator=g) < 0.1] = 0.0
    return sensor, est


def _pipe(depth_ratio):
    from scorp_amd.train import PipelineParams
    pipe = PipelineParams()
    pipe.depth_ratio = depth_ratio
    return pipe


def _weights(opt, it):
    """(lambda_depth_sensor, 10 dn_l1_weight, dn_l1_weight after depth_from_iter + 1000)"""
    from scorp_amd.gaussian_model import get_expon_lr_func
    w = get_expon_lr_func(opt.dn_l1_weight_init, opt.dn_l1_weight_final, max_steps=opt.iterations)(it)
    return opt.lambda_depth_sensor, 10 * w, (w if it > opt.depth_from_iter + 1000 else 0.0)


def _model(raw, deg, dev):
    from scorp_amd.renderer2d import GaussianModel2D
    m = GaussianModel2D.from_raw(raw, deg, device=dev)
    m.active_sh_degree = deg
    return m


@pytest.fixture(scope="module")
def real_allmap(dev):
    """The allmap of a real render, 200 x 134 (a partial 64-wide tile, a partial 4-row tile), 6 000 surfels of SH degree 1, its
    camera, and the depth maps - rendered once for the module."""
    from scorp_amd.renderer2d import render
    from scorp_amd.synthetic import make_gaussians, ring_cameras
    raw = make_gaussians(6000, 1, 21, log_scale_mean=math.log(0.04), scale_dims=2)
    cam = ring_cameras(5, 200, 134, 3, radius=3.5, device=dev)[2]
    with torch.no_grad():
        out = render(cam, _model(raw, 1, dev), _pipe(1.0), torch.zeros(3, device=dev))
    sensor, est = _depth_maps(dev, 134, 200, 7)
    return out.allmap.clone(), cam, sensor, est


def _yardstick(allmap, cam, ratio, sensor, est, w):
    from scorp_amd.renderer2d import _camera_rays
    rays_d, rays_o = _camera_rays(cam, allmap.device)
    return ref.surfel_terms_autograd(allmap, cam.world_view_transform, rays_d, rays_o, ratio, sensor, est, *w)


@pytest.mark.parametrize("ratio", RATIOS)
def test_surfel_terms_match_the_float64_yardstick(ratio, real_allmap, dev):
    """Standalone terms on the allmap of a real render.  The two depth terms alone: the set of entries of grad_allmap with a
    nonzero gradient is the yardstick's and each value is within 2e-6 relative (the bounds and the reasoning of
    test_depth_terms_match_the_float64_yardstick: one fp32 rounding of the double-precision uniform, then the depth_ratio mix
    and the quotient's chain, at most five roundings of 6e-8).  With the depth-normal terms on, grad_allmap is held to
    2e-4 of its maximum + 1e-12, what tests/test_gs2d_gpu.py applies to the fused regularisers' backward against its torch
    form (the same chain through the frames of four neighbours, the same fp32 arithmetic).  Each value within 1e-5 relative;
    two calls the same bits; the autograd front-end with upstream 3.0 gives exactly 3.0 times the gradient."""
    from scorp_amd.fused_loss import fused_surfel_terms, surfel_terms
    from scorp_amd.gaussian_model import OptimizationParams2D
    allmap, cam, sensor, est = real_allmap
    H, W = allmap.shape[-2:]
    w_s, w_e, w_n = _weights(OptimizationParams2D(), 8500)
    assert w_n > 0
    # the depth terms alone
    y = _yardstick(allmap, cam, ratio, sensor, est, (w_s, w_e, 0.0))
    assert int(y["Ms"].sum()) > 0.2 * H * W and int(y["Me"].sum()) > 0.2 * H * W      # both masks far from empty
    assert int((allmap[1] == 0).sum()) > 0                                            # ... and the view has empty pixels
    out, g, depth = surfel_terms(allmap, cam, ratio, sensor, est, w_s, w_e, 0.0)
    torch.cuda.synchronize()
    assert torch.equal(depth, y["d"])
    g64, want = g.double(), y["g_allmap"]
    assert torch.isfinite(want).all()
    assert torch.equal(g64 != 0, want != 0)
    nz = want != 0
    rel = ((g64[nz] - want[nz]).abs() / want[nz].abs()).max()
    print(f"depth_ratio {ratio}: depth terms, grad_allmap max relative error {float(rel):.3e} over {int(nz.sum())} entries")
    assert float(rel) <= 2e-6
    for name, got, val in (("total", out[0], y["total"]), ("Ls", out[1], y["Ls"]), ("Le", out[2], y["Le"])):
        print(f"{name}: {float(got):.9g} against {float(val):.9g}")
        assert abs(float(got) - float(val)) <= 1e-5 * abs(float(val)), name
    assert float(out[3]) == 0.0 and float(out[4]) == 0.0 and float(out[5]) == 0.0
    # one term alone
    for s_, e_ in ((sensor, None), (None, est)):
        y1 = _yardstick(allmap, cam, ratio, s_, e_, (w_s if s_ is not None else 0.0, w_e if e_ is not None else 0.0, 0.0))
        o1, g1, _ = surfel_terms(allmap, cam, ratio, s_, e_, w_s if s_ is not None else 0.0, w_e if e_ is not None else 0.0, 0.0)
        assert abs(float(o1[0]) - float(y1["total"])) <= 1e-5 * abs(float(y1["total"]))
        assert torch.equal(g1 != 0, y1["g_allmap"] != 0)
    # with the depth-normal terms
    yn = _yardstick(allmap, cam, ratio, sensor, est, (w_s, w_e, w_n))
    outn, gn, _ = surfel_terms(allmap, cam, ratio, sensor, est, w_s, w_e, w_n)
    torch.cuda.synchronize()
    err, top = float((gn.double() - yn["g_allmap"]).abs().max()), float(yn["g_allmap"].abs().max())
    print(f"depth_ratio {ratio}: all terms, grad_allmap max |difference| {err:.3e} of max {top:.3e}")
    for c in range(7):
        ec, tc = float((gn[c].double() - yn["g_allmap"][c]).abs().max()), float(yn["g_allmap"][c].abs().max())
        print(f"  channel {c}: max |difference| {ec:.3e} of max {tc:.3e}")
    assert torch.isfinite(gn).all() and err <= 2e-4 * top + 1e-12
    for name, got, val in (("total", outn[0], yn["total"]), ("Ls", outn[1], yn["Ls"]), ("Le", outn[2], yn["Le"]),
                           ("Ldn", outn[3], yn["Ldn"]), ("Lrn", outn[4], yn["Lrn"])):
        print(f"{name}: {float(got):.9g} against {float(val):.9g}")
        assert abs(float(got) - float(val)) <= 1e-5 * abs(float(val)), name
    out2, g2, _ = surfel_terms(allmap, cam, ratio, sensor, est, w_s, w_e, w_n)
    assert torch.equal(outn, out2) and torch.equal(gn, g2)
    a = allmap.clone().requires_grad_(True)
    (3.0 * fused_surfel_terms(a, cam, ratio, sensor, est, w_s, w_e, w_n)).backward()
    assert torch.equal(a.grad, 3.0 * gn)


def test_surfel_terms_where_a_workgroup_takes_more_than_one_tile(dev):
    """648 x 418 is 11 x 105 = 1155 tiles of 64 x 4 (both kinds of partial tile), more than the 1024 workgroups pass 1 is
    launched with: 131 of them take two tiles, the others one.  A synthetic allmap (a smooth surface, an empty disc) against the
    yardstick: every value within 1e-5 relative, the surface depth the same bits, two calls the same bits.  grad_allmap is
    held to 2e-4 * (648 / 200) of its maximum + 1e-12: what limits the chain through the frames is the fp32 difference of two
    back-projected points, whose relative error is eps |P| / |P_1 - P_2|, and with the same ring of cameras and the same
    depths the distance between neighbouring points shrinks as 1 / W, so the bound the test above takes at 200 pixels of
    width scales by 648 / 200 here.  Measured with the bound still at 2e-4: 1.286e-7 of 6.419e-4 (2.003e-4), one pixel."""
    from scorp_amd.fused_loss import surfel_terms
    from scorp_amd.synthetic import ring_cameras
    H, W = 418, 648
    cam = ring_cameras(3, W, H, 4, radius=3.0, device=dev)[1]
    g = torch.Generator(device=dev).manual_seed(9)
    rand = lambda *s: torch.rand(*s, device=dev, generator=g)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32),
                            indexing="ij")
    alpha = 0.3 + 0.6 * rand(H, W)
    alpha[(xs - 500) ** 2 + (ys - 90) ** 2 < 70 ** 2] = 0.0      # an empty disc, as a render has empty pixels
    depth = 2.5 + 0.5 * torch.sin(xs / 37.0) + 0.3 * torch.cos(ys / 23.0)   # a smooth surface: the frames stay well conditioned
    n = torch.nn.functional.normalize(torch.randn(3, H, W, device=dev, generator=g), dim=0) * alpha
    allmap = torch.stack([depth * alpha, alpha, n[0], n[1], n[2], (depth + 0.02) * (alpha > 0), 0.01 * rand(H, W)])
    sensor, _ = _depth_maps(dev, H, W, 10)
    # a smooth estimate with an empty band: where white noise happens to make the two difference vectors of a pixel nearly
    # parallel, fp32 keeps no digit of the direction of pred_normal (two pixels of this size's 270 000, 50 % off in their
    # normal gradient against the float64 yardstick), which says nothing about the kernels
    est = (0.5 + 0.3 * torch.sin(xs / 29.0) * torch.cos(ys / 31.0))[None].contiguous()
    est[:, 200:230] = 0.0
    w = (1.5, 2.0, 0.3)
    y = _yardstick(allmap, cam, 0.5, sensor, est, w)
    assert int(y["Ms"].sum()) > 0.2 * H * W and int(y["Me"].sum()) > 0.2 * H * W
    out, ga, d = surfel_terms(allmap, cam, 0.5, sensor, est, *w)
    torch.cuda.synchronize()
    assert torch.equal(d, y["d"])
    for name, got, val in (("total", out[0], y["total"]), ("Ls", out[1], y["Ls"]), ("Le", out[2], y["Le"]),
                           ("Ldn", out[3], y["Ldn"]), ("Lrn", out[4], y["Lrn"])):
        print(f"{name}: {float(got):.9g} against {float(val):.9g}")
        assert abs(float(got) - float(val)) <= 1e-5 * abs(float(val)), name
    err, top = float((ga.double() - y["g_allmap"]).abs().max()), float(y["g_allmap"].abs().max())
    print(f"1155 tiles: grad_allmap max |difference| {err:.3e} of max {top:.3e}")
    for c in range(7):
        dc = (ga[c].double() - y["g_allmap"][c]).abs()
        at = int(dc.argmax())
        print(f"  channel {c}: max |difference| {float(dc.max()):.3e} at (x {at % W}, y {at // W}) of max "
              f"{float(y['g_allmap'][c].abs().max()):.3e}")
    assert torch.isfinite(ga).all() and err <= 2e-4 * (W / 200) * top + 1e-12
    out2, g2, _ = surfel_terms(allmap, cam, 0.5, sensor, est, *w)
    assert torch.equal(out, out2) and torch.equal(ga, g2)


@pytest.mark.parametrize("case", ["sensor_all_zero", "est_all_zero", "est_constant", "sees_nothing"])
def test_degenerate_depth_terms_are_nan_with_zero_gradients(case, real_allmap, dev):
    """A depth term whose mask is empty or whose range is zero reports NaN, contributes a zero gradient, and nothing fails."""
    from scorp_amd.fused_loss import surfel_terms
    allmap, cam, sensor, est = real_allmap
    if case == "sensor_all_zero":
        sensor, est = torch.zeros_like(sensor), None
    elif case == "est_all_zero":
        sensor, est = None, torch.zeros_like(est)
    elif case == "est_constant":
        sensor, est = None, torch.full_like(est, 0.5)
    else:
        allmap = torch.zeros_like(allmap)
    out, g, _ = surfel_terms(allmap, cam, 0.5, sensor, est, 1.5 if sensor is not None else 0.0, 2.0 if est is not None else 0.0, 0.0)
    torch.cuda.synchronize()
    assert math.isnan(float(out[0]))
    assert math.isnan(float(out[1])) == (sensor is not None) and math.isnan(float(out[2])) == (est is not None)
    assert float(g.abs().max()) == 0.0


def test_a_view_that_sees_nothing_moves_only_the_scales(dev):
    """Through the view, every surfel outside the frustum and every term on: the depth terms read NaN, the depth-normal and
    isotropic terms are finite, the scaling gradient is the isotropic one (2e-6 relative against the float64 closed form)
    and every other gradient is exactly zero - no NaN reaches a parameter."""
    from scorp_amd.rasterizer3d import PairPolicy
    from scorp_amd.synthetic import make_gaussians, ring_cameras
    from scorp_amd.train_view import train_view2d
    raw = make_gaussians(1500, 1, 5, log_scale_mean=math.log(0.03), scale_dims=2)
    raw["xyz"] = raw["xyz"] + 1000.0
    cam = ring_cameras(3, 96, 80, 4, radius=3.0, device=dev)[0]
    m = _model(raw, 1, dev)
    sensor, est = _depth_maps(dev, 80, 96, 9)
    lam = 5e-4
    pkg = train_view2d(cam, m, _pipe(0.5), torch.zeros(3, device=dev), torch.rand(3, 80, 96, device=dev), 0.2, 0.05, 100.0,
                       depth_sensor=sensor, depth_est=est, lambda_depth_sensor=1.5, weight_depth_est=2.0, weight_depth_normal=0.3,
                       lambda_isotropic=lam)
    PairPolicy.drain()
    assert int(pkg["radii"].max()) == 0
    assert math.isnan(float(pkg["depth_sensor_loss"])) and math.isnan(float(pkg["depth_est_loss"])) and math.isnan(float(pkg["loss"]))
    assert float(pkg["depth_normal_loss"]) == 1.0 and float(pkg["render_normal_loss"]) == 1.0
    val, g_iso = ref.isotropic2_autograd(m._scaling, lam)
    assert abs(float(pkg["isotropic_loss"]) - float(val)) <= 1e-5 * float(val)
    for n in NAMES:
        grad = getattr(m, n).grad
        assert torch.isfinite(grad).all(), n
        if n != "_scaling":
            assert float(grad.abs().max()) == 0.0, n
    rel = ((m._scaling.grad.double() - g_iso).abs() / g_iso.abs().clamp_min(1e-300))[g_iso != 0].max()
    assert float(rel) <= 2e-6


def _torch_total(pkg, cam, model, gt, sensor, est, w_s, w_e, w_n, lam, ln, ld):
    """render()'s package -> the loss of train_2dgs.py:93-150 in the package's torch forms, and its parts."""
    from scorp_amd.fused_loss import fused_l1_ssim_loss
    from scorp_amd.loss import depth_normal_losses, depth_normalize_, isotropic_loss, l1_loss
    from scorp_amd.renderer2d import surfel_regularizers
    rd = pkg["render_depth"]
    parts = {"photometric_loss": fused_l1_ssim_loss(pkg["render"], gt, 0.2)}
    zero = torch.zeros((), device=rd.device)
    parts["depth_sensor_loss"] = parts["depth_est_loss"] = parts["depth_normal_loss"] = parts["render_normal_loss"] = zero
    parts["isotropic_loss"] = zero
    if sensor is not None:
        mask = (sensor > 0.3) & (sensor < 7) & (rd > 0.0)
        parts["depth_sensor_loss"] = l1_loss(rd[mask], sensor[mask])
    if est is not None:
        mask = (rd > 0.0) & (est > 0.0)
        parts["depth_est_loss"] = l1_loss(depth_normalize_(rd[mask]), depth_normalize_(est[mask]))
        if w_n:
            parts["depth_normal_loss"], parts["render_normal_loss"] = depth_normal_losses(pkg, cam, est)
    if lam:
        parts["isotropic_loss"] = isotropic_loss(model.get_scaling)
    parts["normal_loss"], parts["dist_loss"] = surfel_regularizers(pkg, ln, ld)
    total = (parts["photometric_loss"] + w_s * parts["depth_sensor_loss"] + w_e * parts["depth_est_loss"]
             + w_n * (parts["depth_normal_loss"] + parts["render_normal_loss"]) + lam * parts["isotropic_loss"]
             + parts["normal_loss"] + parts["dist_loss"])
    return total, parts


VIEW_CASES = [("all", r) for r in RATIOS] + [(only, 0.5) for only in ("sensor", "est", "normal", "iso")]


@pytest.mark.parametrize("which,ratio", VIEW_CASES)
def test_train_view2d_with_terms_equals_render_losses_backward(which, ratio, dev):
    """train_view2d(terms...) against render() + fused_l1_ssim_loss + the torch terms + surfel_regularizers + backward() on a
    twin model under the exact, deterministic backward: image, allmap and radii the same bits, every loss part within 1e-5
    relative, every parameter gradient within 2e-3 of its maximum + 1e-12 - the tolerance of
    test_train_view2d_equals_render_loss_regularizers_backward (tests/test_train_gpu.py)."""
    from scorp_amd import rasterizer3d as R
    from scorp_amd.gaussian_model import OptimizationParams2D
    from scorp_amd.rasterizer3d import PairPolicy
    from scorp_amd.renderer2d import render
    from scorp_amd.synthetic import make_gaussians, ring_cameras
    from scorp_amd.train_view import train_view2d
    raw = make_gaussians(3000, 1, 23, log_scale_mean=math.log(0.05), scale_dims=2)
    cam = ring_cameras(3, 96, 80, 4, radius=3.0, device=dev)[1]
    bg, pipe = torch.tensor([0.1, 0.3, 0.2], device=dev), _pipe(ratio)
    gt = torch.rand(3, 80, 96, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    sensor, est = _depth_maps(dev, 80, 96, 6)
    opt = OptimizationParams2D()
    w_s, w_e, w_n = _weights(opt, 8500)
    lam, ln, ld = opt.lambda_isotropic, opt.lambda_normal, 100.0
    if which == "sensor":
        est, w_e, w_n, lam = None, 0.0, 0.0, 0.0
    elif which == "est":
        sensor, w_s, w_n, lam = None, 0.0, 0.0, 0.0
    elif which == "normal":
        sensor, w_s, w_e, lam = None, 0.0, 0.0, 0.0
    elif which == "iso":
        sensor, est, w_s, w_e, w_n = None, None, 0.0, 0.0, 0.0
    a, b = _model(raw, 1, dev), _model(raw, 1, dev)
    PairPolicy.reset()
    try:
        with R.backward_precision("exact_fp32_deterministic"):
            pa = render(cam, a, pipe, bg)
            la, parts = _torch_total(pa, cam, a, gt, sensor, est, w_s, w_e, w_n, lam, ln, ld)
            la.backward()
            pb = train_view2d(cam, b, pipe, bg, gt, 0.2, ln, ld, depth_sensor=sensor, depth_est=est, lambda_depth_sensor=w_s,
                              weight_depth_est=w_e, weight_depth_normal=w_n, lambda_isotropic=lam)
        PairPolicy.drain()
    finally:
        PairPolicy.reset()
    assert torch.equal(pa["render"], pb["render"]) and torch.equal(pa["radii"], pb["radii"]) and torch.equal(pa.allmap, pb["allmap"])
    if sensor is not None or est is not None:
        assert torch.equal(pa["render_depth"], pb["render_depth"])
    else:
        assert pb["render_depth"] is None
    for k, want in list(parts.items()) + [("loss", la)]:
        got, want = float(pb[k]), float(want.detach())
        print(f"{which} {ratio} {k}: view {got:.9g}, torch {want:.9g}")
        assert abs(got - want) <= 1e-5 * abs(want), k
    for n in NAMES:
        ga, gb = getattr(a, n).grad, getattr(b, n).grad
        assert gb is not None and gb.shape == ga.shape, n
        err, top = float((ga - gb).abs().max()), float(ga.abs().max())
        print(f"{which} {ratio} {n}: max |difference| {err:.3e} of max {top:.3e}")
        assert err <= 2e-3 * top + 1e-12, n
    va, vb = pa["viewspace_points"].grad, pb["viewspace_points"].grad
    assert float((va - vb).abs().max()) <= 2e-3 * float(va.abs().max()) + 1e-12
    if lam:   # the rows nothing else reaches carry the isotropic gradient alone: the float64 closed form, 2e-6 relative
        hidden = pb["radii"] == 0
        assert int(hidden.sum()) > 10
        g_iso = ref.isotropic2_gradient_closed_form(b._scaling, lam)[hidden]
        nz = g_iso != 0
        rel = ((b._scaling.grad.double()[hidden] - g_iso).abs()[nz] / g_iso.abs()[nz]).max()
        print(f"isotropic gradient on {int(hidden.sum())} invisible rows: max relative error {float(rel):.3e}")
        assert float(rel) <= 2e-6


@pytest.mark.parametrize("deg,n", [(3, 1500), (1, 700)])
def test_step_inside_the_2dgs_view_with_terms_equals_fused_adam_on_the_written_gradients(deg, n, dev):
    """Under the deterministic backward, three iterations with every term on: train_view2d(optimizer=, stats=, terms...)
    against the same view writing its gradients + accumulate_view_stats + FusedAdam.step().  Parameters, both moments and the
    statistics are the SAME BITS (1500 = five blocks of the linear SH layout and a partial one; degree 1: the padded layout)."""
    from scorp_amd import rasterizer3d as R
    from scorp_amd.gaussian_model import OptimizationParams2D
    from scorp_amd.rasterizer3d import PairPolicy
    from scorp_amd.synthetic import make_gaussians, ring_cameras
    from scorp_amd.train_view import train_view2d
    raw = make_gaussians(n, deg, 33, log_scale_mean=math.log(0.05), scale_dims=2)
    cams = ring_cameras(3, 96, 80, 5, radius=3.2, device=dev)
    gts = [torch.rand(3, 80, 96, device=dev, generator=torch.Generator(device=dev).manual_seed(k)) for k in range(3)]
    maps = [_depth_maps(dev, 80, 96, 40 + k) for k in range(3)]
    bg, pipe = torch.zeros(3, device=dev), _pipe(0.5)
    res = []
    PairPolicy.reset()
    try:
        with R.backward_precision("deterministic"):
            for in_view in (False, True):
                m = _model(raw, deg, dev)
                opt = OptimizationParams2D()
                m.training_setup(opt)
                for it in range(3):
                    m.update_learning_rate(it + 1)
                    w_s, w_e, w_n = _weights(opt, 8501 + it)
                    terms = dict(depth_sensor=maps[it][0], depth_est=maps[it][1], lambda_depth_sensor=w_s, weight_depth_est=w_e,
                                 weight_depth_normal=w_n, lambda_isotropic=opt.lambda_isotropic)
                    if in_view:
                        pkg = train_view2d(cams[it], m, pipe, bg, gts[it], 0.2, 0.05, 100.0, optimizer=m.optimizer,
                                           stats=(m.max_radii2D, m.xyz_gradient_accum, m.denom), **terms)
                        assert pkg["optimizer_stepped"] and pkg["stats_accumulated"]
                        assert all(getattr(m, nm).grad is None for nm in NAMES)
                    else:
                        pkg = train_view2d(cams[it], m, pipe, bg, gts[it], 0.2, 0.05, 100.0, **terms)
                        assert not pkg["optimizer_stepped"]
                        m.accumulate_view_stats(pkg["viewspace_points"], pkg["visibility_filter"], pkg["radii"])
                        m.optimizer.step()
                        m.optimizer.zero_grad(set_to_none=True)
                    assert math.isfinite(float(pkg["loss"])) and float(pkg["depth_sensor_loss"]) > 0
                    assert float(pkg["isotropic_loss"]) > 0 and float(pkg["depth_normal_loss"]) > 0
                    assert int((pkg["radii"] == 0).sum()) > 0      # rows that take the step with the isotropic gradient alone
                PairPolicy.drain()
                assert m.optimizer.take_skipped() == 0
                st = [m.optimizer.state[getattr(m, nm)] for nm in NAMES]
                res.append(([getattr(m, nm).detach().clone() for nm in NAMES], [s_["exp_avg"].clone() for s_ in st],
                            [s_["exp_avg_sq"].clone() for s_ in st],
                            [m.max_radii2D.clone(), m.xyz_gradient_accum.clone(), m.denom.clone()]))
    finally:
        PairPolicy.reset()
    (pa, ma, va, sa), (pb, mb, vb, sb) = res
    assert float(sa[2].sum()) > 0
    for group, xa, xb in (("parameter", pa, pb), ("exp_avg", ma, mb), ("exp_avg_sq", va, vb)):
        for nm, x, y in zip(NAMES, xa, xb):
            assert torch.equal(x, y), f"{group} {nm}: {float((x - y).abs().max()):.3e}"
    for nm, x, y in zip(("max_radii2D", "xyz_gradient_accum", "denom"), sa, sb):
        assert torch.equal(x, y), nm


def test_late_surfel_iterations_with_fused_views_match_the_autograd_loop(dev):
    """Three iterations from 8500 (every term on, the depth-normal ones included) with fused_view=True against three with
    fused_view=False on equal models: losses within 1e-5 relative, every leaf within 2e-3 of its maximum + 1e-12 (the
    tolerance of the view-against-autograd test above), and the fused iterations took the step inside the view.
    Three Adam steps move a leaf by about three learning rates, far less than 2e-3 of its maximum for _xyz and _scaling, so
    the DISTANCE MOVED is held as well: per leaf, mean |fused - autograd| <= 2e-3 of mean |autograd - start|.  Both loops run
    the same deterministic fp32 backward on upstream maps that agree to fp32 rounding, and an Adam step follows a relative
    error of the gradient one to one, so the bulk of the entries agrees to ~1e-6 of its step; an entry whose gradient is a
    sum that cancels (to a sign flip at the worst: twice its step) is rare, which is why the mean and not the maximum is
    held - 2e-3 leaves room for one entry in a thousand to flip, while a wrong weight, a missing term or a gradient added
    twice re-signs or re-scales the steps of a large share of the entries."""
    from scorp_amd import rasterizer3d as R
    from scorp_amd.gaussian_model import OptimizationParams2D
    from scorp_amd.rasterizer3d import PairPolicy
    from scorp_amd.renderer2d import render
    from scorp_amd.synthetic import make_gaussians, ring_cameras
    from scorp_amd.train import training_iteration
    from scorp_amd.train_view import train_view2d
    raw = make_gaussians(3000, 1, 23, log_scale_mean=math.log(0.05), scale_dims=2)
    cams = ring_cameras(3, 96, 80, 4, radius=3.0, device=dev)
    gts = [torch.rand(3, 80, 96, device=dev, generator=torch.Generator(device=dev).manual_seed(k)) for k in range(3)]
    maps = [_depth_maps(dev, 80, 96, 50 + k) for k in range(3)]
    bg, pipe = torch.zeros(3, device=dev), _pipe(0.5)
    out, seen = [], []

    def recording_view(*a, **kw):
        pkg = train_view2d(*a, **kw)
        seen.append((pkg, kw))
        return pkg

    PairPolicy.reset()
    try:
        with R.backward_precision("exact_fp32_deterministic"):
            for fused in (False, True):
                m = _model(raw, 1, dev)
                start = [getattr(m, nm).detach().clone() for nm in NAMES]
                opt = OptimizationParams2D()
                opt.random_background, opt.lambda_dist = False, 100.0
                m.training_setup(opt)
                losses = []
                for k in range(3):
                    kw = dict(fused_view=True, view_fn=recording_view) if fused else {}
                    loss, _ = training_iteration(m, cams[k], gts[k], opt, pipe, bg, 8500 + k, densify=False, render_fn=render,
                                                 surfels=True, gt_depth=maps[k][0], gt_depth_est=maps[k][1], **kw)
                    losses.append(float(loss.detach()))
                PairPolicy.drain()
                out.append((losses, [getattr(m, nm).detach().clone() for nm in NAMES]))
    finally:
        PairPolicy.reset()
    (la, pa), (lb, pb) = out
    print("autograd loop:", la)
    print("fused views:  ", lb)
    assert all(math.isfinite(x) for x in la + lb)
    assert all(abs(x - y) <= 1e-5 * abs(x) for x, y in zip(la, lb)), (la, lb)
    for nm, x, y in zip(NAMES, pa, pb):
        err, top = float((x - y).abs().max()), float(x.abs().max())
        print(f"{nm}: max |difference| {err:.3e} of max {top:.3e}")
        assert err <= 2e-3 * top + 1e-12, nm
    for nm, x, y, x0 in zip(NAMES, pa, pb, start):
        off, moved = float((x - y).abs().mean()), float((x - x0).abs().mean())
        print(f"{nm}: mean |difference| {off:.3e} of mean distance moved {moved:.3e}")
        assert moved > 0 and off <= 2e-3 * moved, nm
    assert len(seen) == 3
    for pkg, kw in seen:
        assert pkg["optimizer_stepped"] and kw["weight_depth_normal"] > 0 and kw["lambda_isotropic"] > 0
        assert float(pkg["depth_normal_loss"]) > 0 and float(pkg["render_normal_loss"]) > 0


def test_an_overflowed_view_with_terms_skips_the_step_and_masks_the_statistics(dev):
    """A far too small pair reservation with every term active: the view says so in its device word, the step inside the view
    moves no parameter, no moment and no statistic - the isotropic gradient of the invisible rows included - and the loop
    masks the view's visibility filter."""
    from scorp_amd.gaussian_model import OptimizationParams2D
    from scorp_amd.rasterizer3d import PairPolicy
    from scorp_amd.renderer2d import render
    from scorp_amd.synthetic import make_gaussians, ring_cameras
    from scorp_amd.train import training_iteration
    PairPolicy.reset()
    try:
        m = _model(make_gaussians(3000, 1, 4, log_scale_mean=math.log(0.05), scale_dims=2), 1, dev)
        opt = OptimizationParams2D()
        opt.random_background = False
        m.training_setup(opt)
        cam = ring_cameras(3, 96, 80, 2, radius=3.0, device=dev)[1]
        gt, bg = torch.rand(3, 80, 96, device=dev), torch.zeros(3, device=dev)
        sensor, est = _depth_maps(dev, 80, 96, 11)
        PairPolicy.set_context(3000, 80, 96, 64)          # far too few pairs for this view
        before = [getattr(m, nm).detach().clone() for nm in NAMES]
        loss, pkg = training_iteration(m, cam, gt, opt, _pipe(0.5), bg, 8501, render_fn=render, surfels=True, fused_view=True,
                                       gt_depth=sensor, gt_depth_est=est)
        assert pkg["optimizer_stepped"] and int(pkg["overflow"]) != 0
        assert not bool(pkg["visibility_filter"].any())
        for nm, b in zip(NAMES, before):
            assert torch.equal(b, getattr(m, nm).detach()), nm
            assert float(m.optimizer.state[getattr(m, nm)]["exp_avg"].abs().sum()) == 0.0, nm
        assert float(m.denom.sum()) == 0.0 and float(m.max_radii2D.sum()) == 0.0
        assert m.optimizer.take_skipped() == 1
        with pytest.raises(RuntimeError):
            PairPolicy.drain()                                       # reports the overflow, grows the reservation
    finally:
        PairPolicy.reset()
