"""The one-call 3DGS view reads its SH rows once: the per-Gaussian forward stores d(colour)/d(view direction) (nine floats
per visible Gaussian of a full workgroup, behind the backward's scratch layout) and the per-Gaussian backward of the same
call reads those instead of the rows.  The separate calls (render() + fused_l1_ssim_loss() + backward(), the autograd
route) cannot know that a matching forward wrote them and read the rows as they always did.

Same build, two paths: under the deterministic backward (no atomic order) every output of `train_view` - maps, loss,
every gradient tensor - equals the autograd route BIT FOR BIT, for model sizes around the 256-Gaussian workgroup (a
partial workgroup alone, exactly one full one, full + partial, several), on a scene with Gaussians behind the camera and
outside the frustum (nothing stored, nothing used) and with one or all three colour channels clamped at 0 (the clamp bit
zeroes the colour gradient in front of the Jacobian).  The fallbacks - a scratch buffer without room for the nine planes,
SH degrees 0 - 2, the isotropic term, the optimizer step on the SH leaves inside the view, an overflowed pair
reservation - keep working and keep their bits.  (tests/test_train_gpu.py holds the in-view optimizer step to the separate
step over several iterations; with this change its two sides take the two paths.)"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

W, H = 96, 64
NAMES = ("_xyz", "_features_dc", "_features_rest", "_opacity", "_scaling", "_rotation")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _raw(n, deg, seed=7):
    """Camera INSIDE the cloud (ring radius 1.2, extent 1.5): part of the Gaussians lies behind it or beside the frustum.
    Every 5th Gaussian has its red dc coefficient at -6 (SH_C0 * -6 + 0.5 < 0 whatever the 0.1-sized rest adds: clamped),
    every 7th all three."""
    from scorp_amd.synthetic import make_gaussians
    raw = make_gaussians(n, deg, seed, extent=1.5, log_scale_mean=math.log(0.08))
    raw["xyz"][0] = 0.0                      # the look-at point: N = 1 is a visible Gaussian
    raw["opacity"] += 1.0
    raw["features_dc"][::5, 0, 0] = -6.0
    raw["features_dc"][::7, 0, :] = -6.0
    if n > 1:
        raw["features_dc"][0] = 0.3
    return raw


def _setup(dev, seed=3):
    from scorp_amd.synthetic import ring_cameras
    cam = ring_cameras(4, W, H, seed, radius=1.2, device=dev)[1]
    gt = torch.rand(3, H, W, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))
    return cam, gt, torch.tensor([0.2, 0.1, 0.3], device=dev)


def _model(raw, deg, dev):
    from scorp_amd.gaussian_model import GaussianModel
    m = GaussianModel.from_raw(raw, deg, device=dev)
    m.active_sh_degree = deg
    return m


def _autograd_route(raw, deg, dev, cam, gt, bg):
    from scorp_amd.fused_loss import fused_l1_ssim_loss
    from scorp_amd.renderer import render
    from scorp_amd.train import PipelineParams
    m = _model(raw, deg, dev)
    pkg = render(cam, m, PipelineParams(), bg)
    loss = fused_l1_ssim_loss(pkg["render"], gt, 0.2)
    loss.backward()
    return m, pkg, loss


def _assert_same_bits(ma, pa, la, mb, pb, skip=()):
    for k in ("render", "radii", "visibility_filter", "render_depth", "render_alpha"):
        assert torch.equal(pa[k], pb[k]), k
    assert float(la) == float(pb["loss"] if "photometric_loss" not in pb else pb["photometric_loss"])
    for nm in NAMES:
        if nm in skip:
            continue
        ga, gb = getattr(ma, nm).grad, getattr(mb, nm).grad
        assert gb is not None and ga.shape == gb.shape, nm
        assert torch.equal(ga, gb), f"{nm}: max |diff| {float((ga - gb).abs().max()):.3e} of {float(ga.abs().max()):.3e}"
    assert torch.equal(pa["viewspace_points"].grad, pb["viewspace_points"].grad)


def _parent_scratch_bytes(L):
    """The library's own size function minus the nine planes (include/scorp_gs.h): the scratch layout alone."""
    real = L.scorp_gs3d_backward_scratch_bytes_ex

    def small(n, w, h, capacity, flags):
        return real(n, w, h, capacity, flags) - 36 * ((max(int(n), 1) + 255) // 256 * 256)
    return small


@pytest.mark.parametrize("n", [1, 255, 256, 257, 513, 1000])
def test_view_with_stored_jacobian_equals_the_autograd_route_bit_for_bit(n, dev):
    from scorp_amd import _C
    from scorp_amd.rasterizer3d import PairPolicy, backward_precision
    from scorp_amd.train import PipelineParams
    from scorp_amd.train_view import train_view
    raw = _raw(n, 3)
    cam, gt, bg = _setup(dev)
    L = _C.lib()
    # the buffer train_view sizes holds the planes: the new path is the one that runs
    flags = _C.BACKWARD_DETERMINISTIC
    assert L.scorp_gs3d_backward_scratch_bytes_ex(n, W, H, 4096, flags) == \
        _parent_scratch_bytes(L)(n, W, H, 4096, flags) + 36 * ((n + 255) // 256 * 256)
    with backward_precision("deterministic"):
        ma, pa, la = _autograd_route(raw, 3, dev, cam, gt, bg)
        mb = _model(raw, 3, dev)
        pb = train_view(cam, mb, PipelineParams(), bg, gt, 0.2)
        PairPolicy.drain()
    _assert_same_bits(ma, pa, la, mb, pb)
    vis = pa["visibility_filter"]
    if n == 1000:   # the contents the mask logic is about are really there
        assert bool(vis.any()) and not bool(vis.all())
        assert bool(vis[::5].any()) and bool(vis[::7].any())
        dc = mb._features_dc.grad[:, 0, :]
        assert float(dc[35::35].abs().max()) == 0.0                    # all three channels clamped (Gaussian 0 has its own colour)
        seen = vis.clone(); seen[::7] = False
        assert float(dc[seen][:, 1:].abs().max()) > 0.0
        red_only = torch.zeros_like(vis); red_only[5::5] = True; red_only[::7] = False
        assert float(dc[red_only][:, 0].abs().max()) == 0.0 and float(dc[red_only & vis][:, 1:].abs().max()) > 0.0
        assert float(mb._xyz.grad[~vis].abs().max()) == 0.0
    assert all(bool(torch.isfinite(getattr(mb, nm).grad).all()) for nm in NAMES)


def test_scratch_without_the_planes_takes_the_old_path(dev, monkeypatch):
    from scorp_amd import _C
    from scorp_amd.rasterizer3d import PairPolicy, backward_precision
    from scorp_amd.train import PipelineParams
    from scorp_amd.train_view import train_view
    raw = _raw(513, 3)
    cam, gt, bg = _setup(dev)
    L = _C.lib()
    with backward_precision("deterministic"):
        ma, pa, la = _autograd_route(raw, 3, dev, cam, gt, bg)
        monkeypatch.setattr(L, "scorp_gs3d_backward_scratch_bytes_ex", _parent_scratch_bytes(L))
        mb = _model(raw, 3, dev)
        pb = train_view(cam, mb, PipelineParams(), bg, gt, 0.2)
        PairPolicy.drain()
    _assert_same_bits(ma, pa, la, mb, pb)


@pytest.mark.parametrize("deg", [0, 1, 2])
def test_lower_sh_degrees_keep_their_path_and_their_bits(deg, dev):
    from scorp_amd.rasterizer3d import PairPolicy, backward_precision
    from scorp_amd.train import PipelineParams
    from scorp_amd.train_view import train_view
    raw = _raw(600, deg)
    cam, gt, bg = _setup(dev)
    with backward_precision("deterministic"):
        ma, pa, la = _autograd_route(raw, deg, dev, cam, gt, bg)
        mb = _model(raw, deg, dev)
        pb = train_view(cam, mb, PipelineParams(), bg, gt, 0.2)
        PairPolicy.drain()
    _assert_same_bits(ma, pa, la, mb, pb, skip=("_features_rest",) if deg == 0 else ())


def test_isotropic_term_with_and_without_the_planes(dev, monkeypatch):
    """lambda_isotropic != 0 selects the ISO instantiation of the per-Gaussian backward.  The term only adds to the scaling
    gradient: everything else equals the autograd route of the photometric loss bit for bit, and the scaling gradient
    equals the one of the same view run on a scratch buffer without the planes (rows read a second time)."""
    from scorp_amd import _C
    from scorp_amd.rasterizer3d import PairPolicy, backward_precision
    from scorp_amd.train import PipelineParams
    from scorp_amd.train_view import train_view
    raw = _raw(513, 3)
    cam, gt, bg = _setup(dev)
    L = _C.lib()
    with backward_precision("deterministic"):
        ma, pa, la = _autograd_route(raw, 3, dev, cam, gt, bg)
        mb = _model(raw, 3, dev)
        pb = train_view(cam, mb, PipelineParams(), bg, gt, 0.2, lambda_isotropic=0.3)
        monkeypatch.setattr(L, "scorp_gs3d_backward_scratch_bytes_ex", _parent_scratch_bytes(L))
        mc = _model(raw, 3, dev)
        pc = train_view(cam, mc, PipelineParams(), bg, gt, 0.2, lambda_isotropic=0.3)
        PairPolicy.drain()
    _assert_same_bits(ma, pa, la, mb, pb, skip=("_scaling",))
    _assert_same_bits(ma, pa, la, mc, pc, skip=("_scaling",))
    assert torch.equal(mb._scaling.grad, mc._scaling.grad)
    assert not torch.equal(mb._scaling.grad, ma._scaling.grad)      # the term is there
    assert float(pb["isotropic_loss"]) == float(pc["isotropic_loss"]) > 0.0


def test_optimizer_step_on_the_sh_leaves_inside_the_view_reads_the_rows(dev):
    """`optimizer=` with SH moments: the epilogue updates the SH leaves from the rows it staged, so the view keeps the old
    path.  One iteration against the separate step on the gradients the (new-path) view wrote: same parameter bits."""
    from scorp_amd.gaussian_model import OptimizationParams
    from scorp_amd.rasterizer3d import PairPolicy, backward_precision
    from scorp_amd.train import PipelineParams
    from scorp_amd.train_view import train_view
    raw = _raw(513, 3)
    cam, gt, bg = _setup(dev)
    out = []
    PairPolicy.reset()
    try:
        with backward_precision("deterministic"):
            for in_view in (False, True):
                m = _model(raw, 3, dev)
                m.training_setup(OptimizationParams())
                m.update_learning_rate(1)
                if in_view:
                    pkg = train_view(cam, m, PipelineParams(), bg, gt, 0.2, optimizer=m.optimizer)
                    assert pkg["optimizer_stepped"]
                else:
                    train_view(cam, m, PipelineParams(), bg, gt, 0.2)
                    m.optimizer.step()
                PairPolicy.drain()
                out.append([getattr(m, nm).detach().clone() for nm in NAMES])
    finally:
        PairPolicy.reset()
    for nm, a, b in zip(NAMES, *out):
        assert torch.equal(a, b), nm
    assert not torch.equal(out[0][2], torch.as_tensor(raw["features_rest"], device=dev))


def test_overflowed_view_flags_it_and_the_rerun_has_the_bits(dev):
    """A reservation far too small: the view says so in its overflow word, drain() raises and grows the reservation as
    before, and the same view run again equals the autograd route bit for bit."""
    from scorp_amd.rasterizer3d import PairPolicy, backward_precision
    from scorp_amd.train import PipelineParams
    from scorp_amd.train_view import train_view
    n = 1000
    raw = _raw(n, 3)
    cam, gt, bg = _setup(dev)
    PairPolicy.reset()
    try:
        with backward_precision("deterministic"):
            ma, pa, la = _autograd_route(raw, 3, dev, cam, gt, bg)
            PairPolicy.set_context(n, H, W, 64)
            mb = _model(raw, 3, dev)
            pb = train_view(cam, mb, PipelineParams(), bg, gt, 0.2)
            assert int(pb["overflow"]) != 0
            assert all(bool(torch.isfinite(getattr(mb, nm).grad).all()) for nm in NAMES)
            assert torch.equal(pa["radii"], pb["radii"])            # the per-Gaussian forward ran in full
            with pytest.raises(RuntimeError):
                PairPolicy.drain()
            mc = _model(raw, 3, dev)
            pc = train_view(cam, mc, PipelineParams(), bg, gt, 0.2)
            assert int(pc["overflow"]) == 0
            PairPolicy.drain()
        _assert_same_bits(ma, pa, la, mc, pc)
    finally:
        PairPolicy.reset()
