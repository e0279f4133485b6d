"""The late iterations' loss terms (train_3dgs.py:109-150) inside the one-call 3DGS view: the depth-term kernels against
the float64 yardstick (tests/view_terms_reference.py), their degenerate cases, scorp_gs3d_train_view_ex against render() +
the torch terms + autograd, the optimizer step inside the view bit for bit, and the training loop."""
import math

import pytest
import torch

from tests import view_terms_reference as ref

pytestmark = pytest.mark.gpu

NAMES = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


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


def _weights(opt, it):
    from scorp_amd.gaussian_model import get_expon_lr_func
    return opt.lambda_depth_sensor, 10 * get_expon_lr_func(opt.dn_l1_weight_init, opt.dn_l1_weight_final, max_steps=opt.iterations)(it)


def _raw_render(dev, n=6000, deg=3, seed=21):
    """depth_raw / alpha of a real render (the rasterizer's un-normalised outputs)."""
    from scorp_amd.gaussian_model import GaussianModel
    from scorp_amd.renderer import render
    from scorp_amd.synthetic import make_gaussians, ring_cameras
    from scorp_amd.train import PipelineParams
    raw = make_gaussians(n, deg, seed, log_scale_mean=math.log(0.03))
    cam = ring_cameras(5, 200, 136, 3, radius=3.5, device=dev)[2]
    m = GaussianModel.from_raw(raw, deg, device=dev)
    m.active_sh_degree = deg
    pipe = PipelineParams()
    pipe.raw_outputs = True
    with torch.no_grad():
        out = render(cam, m, pipe, torch.zeros(3, device=dev))
    return out["render_depth_raw"].clone(), out["render_alpha"].clone()


def test_depth_terms_match_the_float64_yardstick(dev):
    """Standalone depth terms on the maps of a real render: the set of pixels with a nonzero gradient is the yardstick's, each
    gradient value within 2e-6 relative (at most four fp32 roundings of 6e-8 with margin for the division), each term's value
    within 1e-5 relative, two calls the same bits."""
    from scorp_amd.fused_loss import depth_terms, fused_depth_terms
    from scorp_amd.gaussian_model import OptimizationParams
    depth_raw, alpha = _raw_render(dev)
    H, W = depth_raw.shape[-2:]
    sensor, est = _depth_maps(dev, H, W, 7)
    w_s, w_e = _weights(OptimizationParams(), 7500)
    r = ref.rendered_depth(depth_raw, alpha)
    y = ref.depth_terms_autograd(r, sensor, est, w_s, w_e)
    assert int(y["Ms"].sum()) > 0.2 * H * W and int(y["Me"].sum()) > 0.2 * H * W      # both masks far from empty
    assert int((alpha == 0).sum()) > 0                                                # ... and the view has empty pixels
    yd, ya = ref.tail_gradients(y["g_r"], depth_raw, alpha)
    out, gd, ga = depth_terms(depth_raw, alpha, sensor, est, w_s, w_e)
    torch.cuda.synchronize()
    for name, got, want in (("g_depth_raw", gd, yd), ("g_alpha", ga, ya)):
        got64 = got.double()
        assert torch.equal(got64 != 0, want != 0), name
        nz = want != 0
        rel = ((got64[nz] - want[nz]).abs() / want[nz].abs()).max()
        print(f"{name}: max relative error {float(rel):.3e} over {int(nz.sum())} pixels")
        assert float(rel) <= 2e-6, name
    for name, got, want in (("total", out[0], y["total"]), ("Ls", out[1], y["Ls"]), ("Le", out[2], y["Le"])):
        print(f"{name}: {float(got):.9g} against {float(want):.9g}")
        assert abs(float(got) - float(want)) <= 1e-5 * abs(float(want)), name
    assert float(out[3]) == 0.0
    out2, gd2, ga2 = depth_terms(depth_raw, alpha, sensor, est, w_s, w_e)
    assert torch.equal(out, out2) and torch.equal(gd, gd2) and torch.equal(ga, ga2)
    # one term alone, and the autograd front-end with an upstream gradient
    for s_, e_ in ((sensor, None), (None, est)):
        y1 = ref.depth_terms_autograd(r, s_, e_, w_s, w_e)
        o1, gd1, _ = depth_terms(depth_raw, alpha, s_, e_, w_s if s_ is not None else 0.0, w_e if e_ is not None else 0.0)
        assert abs(float(o1[0]) - float(y1["total"])) <= 1e-5 * abs(float(y1["total"]))
        y1d, _ = ref.tail_gradients(y1["g_r"], depth_raw, alpha)
        assert torch.equal(gd1 != 0, y1d != 0)
    d, a = depth_raw.clone().requires_grad_(True), alpha.clone().requires_grad_(True)
    (3.0 * fused_depth_terms(d, a, sensor, est, w_s, w_e)).backward()
    assert torch.equal(d.grad, 3.0 * gd.view_as(d)) and torch.equal(a.grad, 3.0 * ga.view_as(a))


@pytest.mark.parametrize("case", ["sensor_all_zero", "est_all_zero", "est_constant", "sees_nothing"])
def test_degenerate_depth_terms_are_nan_with_zero_gradients(case, dev):
    """A term whose mask is empty or whose range is zero reports NaN, contributes a zero gradient, and nothing fails."""
    from scorp_amd.fused_loss import depth_terms
    depth_raw, alpha = _raw_render(dev, n=2000)
    H, W = depth_raw.shape[-2:]
    sensor, est = _depth_maps(dev, H, W, 8)
    if case == "sensor_all_zero":
        sensor, est = torch.zeros_like(sensor), None
    elif case == "est_all_zero":
        sensor, est = None, torch.zeros_like(est)
    elif case == "est_constant":
        sensor, est = None, torch.full_like(est, 0.5)
    else:
        depth_raw, alpha = torch.zeros_like(depth_raw), torch.zeros_like(alpha)
    out, gd, ga = depth_terms(depth_raw, alpha, sensor, est, 1.5 if sensor is not None else 0.0, 2.0 if est is not None else 0.0)
    torch.cuda.synchronize()
    assert math.isnan(float(out[0]))
    assert math.isnan(float(out[1])) == (sensor is not None) and math.isnan(float(out[2])) == (est is not None)
    assert float(gd.abs().max()) == 0.0 and float(ga.abs().max()) == 0.0


def test_a_view_that_sees_nothing_moves_only_the_scales(dev):
    """Through the view: every Gaussian outside the frustum.  The depth terms read NaN, the isotropic term is finite, the
    scaling gradient is the isotropic one and every other gradient is exactly zero - no NaN reaches a parameter."""
    from scorp_amd.gaussian_model import GaussianModel
    from scorp_amd.rasterizer3d import PairPolicy
    from scorp_amd.synthetic import make_gaussians, ring_cameras
    from scorp_amd.train import PipelineParams
    from scorp_amd.train_view import train_view
    raw = make_gaussians(1500, 1, 5, log_scale_mean=math.log(0.03))
    raw["xyz"] = raw["xyz"] + 1000.0
    cam = ring_cameras(3, 96, 80, 4, radius=3.0, device=dev)[0]
    m = GaussianModel.from_raw(raw, 1, device=dev)
    m.active_sh_degree = 1
    sensor, est = _depth_maps(dev, 80, 96, 9)
    lam = 5e-4
    pkg = train_view(cam, m, PipelineParams(), torch.zeros(3, device=dev), torch.rand(3, 80, 96, device=dev), 0.2,
                     depth_sensor=sensor, depth_est=est, lambda_depth_sensor=1.5, weight_depth_est=2.0, lambda_isotropic=lam)
    PairPolicy.drain()
    assert int(pkg["radii"].max()) == 0
    assert math.isnan(float(pkg["depth_sensor_loss"])) and math.isnan(float(pkg["depth_est_loss"])) and math.isnan(float(pkg["loss"]))
    val, g_iso = ref.isotropic_autograd(m._scaling, lam)
    assert abs(float(pkg["isotropic_loss"]) - float(val)) <= 1e-5 * float(val)
    for n in NAMES:
        grad = getattr(m, n).grad
        assert torch.isfinite(grad).all(), n
        if n != "_scaling":
            assert float(grad.abs().max()) == 0.0, n
    rel = ((m._scaling.grad.double() - g_iso).abs() / g_iso.abs().clamp_min(1e-300))[g_iso != 0].max()
    assert float(rel) <= 2e-6


def test_train_view_with_terms_equals_render_losses_backward(dev):
    """train_view(terms...) against render() + fused_l1_ssim_loss + depth_losses + lambda * isotropic_loss(get_scaling) +
    backward() on a twin model: images, radii, visibility the same bits; total loss within 1e-5 max(1, |loss|); every gradient
    within 2e-3 of its maximum (view against autograd: float-atomics order).  That tolerance would hide a missing isotropic
    term, so on the rows with radii == 0 the scaling gradient is held to the float64 closed form within 2e-6 relative, and
    every other leaf's gradient is exactly zero there."""
    from scorp_amd.fused_loss import fused_l1_ssim_loss
    from scorp_amd.gaussian_model import GaussianModel, OptimizationParams
    from scorp_amd.loss import depth_losses, isotropic_loss
    from scorp_amd.rasterizer3d import PairPolicy
    from scorp_amd.renderer import render
    from scorp_amd.synthetic import make_gaussians, ring_cameras
    from scorp_amd.train import PipelineParams
    from scorp_amd.train_view import train_view
    raw = make_gaussians(6000, 3, 21, log_scale_mean=math.log(0.03))
    cam = ring_cameras(5, 200, 136, 3, radius=3.5, device=dev)[2]
    bg, pipe = torch.tensor([0.1, 0.3, 0.2], device=dev), PipelineParams()
    gt = torch.rand(3, 136, 200, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    sensor, est = _depth_maps(dev, 136, 200, 6)
    opt, it = OptimizationParams(), 7500
    w_s, w_e = _weights(opt, it)
    lam = opt.lambda_isotropic
    a = GaussianModel.from_raw(raw, 3, device=dev); a.active_sh_degree = 3
    b = GaussianModel.from_raw(raw, 3, device=dev); b.active_sh_degree = 3
    pa = render(cam, a, pipe, bg)
    la = fused_l1_ssim_loss(pa["render"], gt, 0.2) + depth_losses(pa["render_depth"], it, opt, sensor, est) \
        + lam * isotropic_loss(a.get_scaling)
    la.backward()
    pb = train_view(cam, b, pipe, bg, gt, 0.2, depth_sensor=sensor, depth_est=est, lambda_depth_sensor=w_s, weight_depth_est=w_e,
                    lambda_isotropic=lam)
    PairPolicy.drain()
    for k in ("render", "radii", "visibility_filter", "render_depth", "render_alpha"):
        assert torch.equal(pa[k], pb[k]), k
    la_, lb_ = float(la.detach()), float(pb["loss"])
    print(f"total loss: autograd {la_:.9g}, view {lb_:.9g}")
    assert abs(la_ - lb_) <= 1e-5 * max(1.0, abs(la_))
    for n in NAMES:
        ga, gb = getattr(a, n).grad, getattr(b, n).grad
        assert gb is not None and gb.shape == ga.shape, n
        err, top = float((ga - gb).abs().max()), float(ga.abs().max())
        print(f"{n}: max |difference| {err:.3e} of max {top:.3e}")
        assert err <= 2e-3 * top + 1e-12, n
    va, vb = pa["viewspace_points"].grad, pb["viewspace_points"].grad
    assert float((va - vb).abs().max()) <= 2e-3 * float(va.abs().max()) + 1e-12
    hidden = pb["radii"] == 0
    assert int(hidden.sum()) > 10
    g_iso = ref.isotropic_gradient_closed_form(b._scaling, lam)[hidden]
    got = b._scaling.grad.double()[hidden]
    assert bool((g_iso != 0).all())
    rel = ((got - g_iso).abs() / g_iso.abs()).max()
    print(f"isotropic gradient on {int(hidden.sum())} invisible rows: max relative error {float(rel):.3e}")
    assert float(rel) <= 2e-6
    for n in NAMES:
        if n != "_scaling":
            assert float(getattr(b, n).grad[hidden].abs().max()) == 0.0, n
    # the three values the result carries, unweighted
    y = ref.depth_terms_autograd(pa["render_depth"].detach(), sensor, est, w_s, w_e)
    val, _ = ref.isotropic_autograd(b._scaling, lam)
    for k, want in (("depth_sensor_loss", y["Ls"]), ("depth_est_loss", y["Le"]), ("isotropic_loss", val)):
        assert abs(float(pb[k]) - float(want)) <= 1e-5 * abs(float(want)), k


@pytest.mark.parametrize("deg,n", [(3, 3000), (1, 1500)])
def test_step_inside_the_view_with_terms_equals_fused_adam_on_the_written_gradients(deg, n, dev):
    """Under the deterministic backward, four iterations with a moving learning rate and all three terms on:
    train_view(optimizer=, stats=, terms...) against the same view writing its gradients + accumulate_view_stats +
    FusedAdam.step().  Parameters, both moments and the statistics are the SAME BITS (3000 = 11 blocks of the linear SH layout
    and a partial one; degree 1 takes the padded layout)."""
    from scorp_amd import rasterizer3d as R
    from scorp_amd.gaussian_model import GaussianModel, OptimizationParams
    from scorp_amd.rasterizer3d import PairPolicy
    from scorp_amd.synthetic import make_gaussians, ring_cameras
    from scorp_amd.train import PipelineParams
    from scorp_amd.train_view import train_view
    raw = make_gaussians(n, deg, 31, log_scale_mean=math.log(0.05))
    cams = ring_cameras(4, 160, 112, 5, radius=3.2, device=dev)
    gts = [torch.rand(3, 112, 160, device=dev, generator=torch.Generator(device=dev).manual_seed(k)) for k in range(4)]
    maps = [_depth_maps(dev, 112, 160, 40 + k) for k in range(4)]
    bg, pipe = torch.tensor([0.1, 0.2, 0.3], device=dev), PipelineParams()
    res = []
    PairPolicy.reset()
    try:
        with R.backward_precision("deterministic"):
            for in_view in (False, True):
                m = GaussianModel.from_raw(raw, deg, device=dev)
                m.active_sh_degree = deg
                opt = OptimizationParams()
                m.training_setup(opt)
                for it in range(4):
                    m.update_learning_rate(it + 1)
                    w_s, w_e = _weights(opt, 7001 + it)
                    terms = dict(depth_sensor=maps[it][0], depth_est=maps[it][1], lambda_depth_sensor=w_s, weight_depth_est=w_e,
                                 lambda_isotropic=opt.lambda_isotropic)
                    if in_view:
                        pkg = train_view(cams[it], m, pipe, bg, gts[it], 0.2, optimizer=m.optimizer,
                                         stats=(m.max_radii2D, m.xyz_gradient_accum, m.denom), **terms)
                        assert pkg["optimizer_stepped"] and pkg["stats_accumulated"]
                        assert all(getattr(m, nm).grad is None for nm in NAMES)
                    else:
                        pkg = train_view(cams[it], m, pipe, bg, gts[it], 0.2, **terms)
                        assert not pkg["optimizer_stepped"]
                        m.accumulate_view_stats(pkg["viewspace_points"], pkg["visibility_filter"], pkg["radii"])
                        m.optimizer.step()
                        m.optimizer.zero_grad(set_to_none=True)
                    assert math.isfinite(float(pkg["loss"])) and float(pkg["depth_sensor_loss"]) > 0 and float(pkg["isotropic_loss"]) > 0
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
    for nm, x, y in zip(NAMES, pa, pb):
        assert torch.equal(x, y), f"parameter {nm}: {float((x - y).abs().max()):.3e}"
    for nm, x, y in zip(NAMES, ma, mb):
        assert torch.equal(x, y), f"exp_avg of {nm}"
    for nm, x, y in zip(NAMES, va, vb):
        assert torch.equal(x, y), f"exp_avg_sq of {nm}"
    for nm, x, y in zip(("max_radii2D", "xyz_gradient_accum", "denom"), sa, sb):
        assert torch.equal(x, y), nm


def test_training_with_fused_views_and_terms_matches_the_autograd_loop(dev):
    """train(..., fused_view=True) against the autograd loop over 40 iterations with depth_from_iter = 10 and per-camera
    depth lists: losses within 2e-3 |x| + 1e-6, and the late iterations stay in the one-call view - the last iteration's
    package says optimizer_stepped."""
    import numpy as np
    from scorp_amd.gaussian_model import GaussianModel, OptimizationParams
    from scorp_amd.synthetic import make_gaussians, ring_cameras
    from scorp_amd.train import PipelineParams, render_views_gt, train
    from scorp_amd.train_view import train_view
    raw = make_gaussians(3000, 1, 13, extent=1.0, log_scale_mean=math.log(0.05))
    raw["opacity"] += 1.5
    teacher = GaussianModel.from_raw(raw, 1, device=dev)
    teacher.active_sh_degree = 1
    raw2 = {k: v.copy() for k, v in raw.items()}
    raw2["features_dc"] += np.random.default_rng(14).normal(0, 0.6, raw2["features_dc"].shape).astype(np.float32)
    cams = ring_cameras(6, 160, 120, 4, radius=3.0, device=dev)
    gts = render_views_gt(teacher, cams)
    maps = [_depth_maps(dev, 120, 160, 60 + k) for k in range(6)]
    sensors, ests = [s for s, _ in maps], [e for _, e in maps]
    out, pkgs = [], []

    def recording_view(*a, **kw):
        pkg = train_view(*a, **kw)
        pkgs.append((pkg, kw))
        return pkg

    for fused in (False, True):
        student = GaussianModel.from_raw(raw2, 1, device=dev)
        student.active_sh_degree = 1
        opt = OptimizationParams()
        opt.densify_from_iter, opt.densification_interval, opt.opacity_reset_interval = 20, 100, 10_000   # statistics, no densify step
        opt.random_background, opt.depth_from_iter = False, 10
        kw = dict(fused_view=True, view_fn=recording_view) if fused else {}
        out.append(train(student, cams, gts, opt, PipelineParams(), iterations=40, scene_extent=3.0, gt_depths=sensors,
                         gt_depth_ests=ests, **kw))
    la, lb = out
    print("autograd loop:", [round(x, 6) for x in la])
    print("fused views:  ", [round(x, 6) for x in lb])
    assert len(la) == len(lb) == 40 and all(math.isfinite(x) for x in la + lb)
    assert all(abs(x - y) <= 2e-3 * abs(x) + 1e-6 for x, y in zip(la, lb)), (la, lb)
    assert len(pkgs) >= 40                                    # every iteration went through the view (plus a first-view retry)
    last_pkg, last_kw = pkgs[-1]
    assert last_pkg["optimizer_stepped"]
    assert last_kw["lambda_isotropic"] == OptimizationParams().lambda_isotropic and "depth_sensor" in last_kw and "depth_est" in last_kw
    assert float(last_pkg["depth_sensor_loss"]) > 0
