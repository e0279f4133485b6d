"""The late iterations' loss terms inside the one-call 2DGS view (scorp_gs2d_train_view_ex, ScorpGs2dViewTerms): what can be
checked without a GPU - the ABI, the argument checks (they run before any launch), the float64 yardstick the GPU tests use
against finite differences and against the package's own torch formulation, and the routing of training_iteration."""
import ctypes
import os
import subprocess

import pytest
import torch

from tests import surfel_terms_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("scorp_gs2d_view_terms_workspace_bytes", "scorp_gs2d_train_view_ex", "scorp_gs2d_surfel_terms")


@pytest.fixture(scope="module")
def L():
    from scorp_amd import _C, build
    build.build()
    return _C.lib()


def test_new_symbols_are_declared_exported_and_bound(L):
    from scorp_amd import _C
    txt = open(os.path.join(ROOT, "include", "scorp_gs.h")).read()
    for name in NEW:
        assert name + "(" in txt and name in _C.EXPORTS and hasattr(L, name), name


def test_view_terms_struct_has_the_headers_size(tmp_path):
    from scorp_amd import _C
    fields = ("weight_depth_normal", "lambda_isotropic", "out_terms6", "out_depth", "grad_depth", "grad_normal", "workspace_bytes")
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scorp_gs.h"\nint main(void) { printf("%zu'
                   + " %zu" * len(fields) + '\\n", sizeof(ScorpGs2dViewTerms)'
                   + "".join(f", offsetof(ScorpGs2dViewTerms, {f})" for f in fields) + "); return 0; }\n")
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    T = _C.ScorpGs2dViewTerms
    assert got == [ctypes.sizeof(T)] + [getattr(T, f).offset for f in fields]


def test_workspace_bytes_is_monotone_and_small(L):
    f = L.scorp_gs2d_view_terms_workspace_bytes
    assert f(0, 0, 0) > 0 and f(1, 1, 0) > 0
    sizes = [(64, 64, 0), (64, 64, 1000), (640, 480, 1000), (1600, 1200, 1000), (1600, 1200, 1_000_000)]
    vals = [f(*s) for s in sizes]
    assert all(a <= b for a, b in zip(vals, vals[1:])), vals
    assert vals[0] < vals[-1] <= 256 * 1024       # per-workgroup partial sums: three per 64 x 4 tile at the most


def _dummy_view(_C, keep):
    """A view that passes every check of scorp_gs2d_train_view itself: dummy non-NULL pointers, never dereferenced because
    the terms are checked before anything is launched."""
    d = 0x10000
    inp = _C.ScorpGs3dInputs(num_gaussians=100, sh_degree=1, sh_coeffs=4, image_width=64, image_height=48, tanfovx=1.0,
                             tanfovy=1.0, scale_modifier=1.0, bg=d, viewmatrix=d, projmatrix=d, campos=d, means3D=d, shs=d,
                             opacities=d, scales=d, rotations=d, shs_rest=d, raw_params=7)
    grads = _C.ScorpGs3dGrads()
    keep += [inp, grads]
    v = _C.ScorpGs2dTrainView()
    v.inputs, v.grads = ctypes.addressof(inp), ctypes.addressof(grads)
    for n in ("out_radii", "state", "pairs", "out_color", "out_allmap", "gt", "rays_d", "rays_o", "out_loss3", "out_reg2",
              "loss_workspace", "reg_workspace", "grad_color", "grad_allmap", "backward_scratch"):
        setattr(v, n, d)
    return v, inp


@pytest.mark.parametrize("case, reason", [
    ("out_terms6", b"out_terms6"), ("sensor_map", b"lambda_depth_sensor without depth_sensor"),
    ("est_map", b"weight_depth_est without depth_est"), ("normal_without_est", b"weight_depth_normal without depth_est"),
    ("out_depth", b"out_depth"), ("grad_depth", b"grad_depth"), ("grad_normal", b"grad_normal"), ("grad_allmap", b"grad_allmap"),
    ("workspace", b"workspace"), ("workspace_small", b"too small"), ("workspace_misaligned", b"misaligned"),
    ("iso_layout", b"training layout")])
def test_train_view_ex_refuses_missing_buffers_before_any_launch(L, case, reason):
    from scorp_amd import _C
    keep = []
    v, inp = _dummy_view(_C, keep)
    d = 0x10000
    t = _C.ScorpGs2dViewTerms()
    t.depth_sensor = t.depth_est = t.out_terms6 = t.out_depth = t.grad_depth = t.grad_normal = t.workspace = d
    t.lambda_depth_sensor, t.weight_depth_est, t.weight_depth_normal, t.lambda_isotropic = 1.5, 2.0, 0.2, 5e-4
    t.workspace_bytes = L.scorp_gs2d_view_terms_workspace_bytes(64, 48, 100)
    if case == "out_terms6":
        t.out_terms6 = None
    elif case == "sensor_map":
        t.depth_sensor = None
    elif case == "est_map":
        t.depth_est, t.weight_depth_normal = None, 0.0
    elif case == "normal_without_est":
        t.depth_est, t.weight_depth_est = None, 0.0
    elif case == "workspace_small":
        t.workspace_bytes -= 1
    elif case == "workspace_misaligned":
        t.workspace = 0x10004
    elif case == "iso_layout":
        inp.shs_rest = None
    elif case == "grad_allmap":
        v.grad_allmap, v.lambda_normal, v.lambda_dist = None, 0.0, 0.0
    else:
        setattr(t, case, None)
    rc = L.scorp_gs2d_train_view_ex(ctypes.byref(v), ctypes.byref(t), None)
    assert rc == _C.ERR_INVALID
    assert reason in L.scorp_last_error(), L.scorp_last_error()


def _small_case(H=10, W=12, seed=5):
    """A 12 x 10 allmap with positive alpha, a camera's ray table, a sensor and an estimate map (CPU, float32)."""
    from oracle.surfel_maps_ref import camera_rays
    from scorp_amd.synthetic import ring_cameras
    cam = ring_cameras(3, W, H, 4, radius=3.0, device="cpu")[1]
    g = torch.Generator().manual_seed(seed)
    alpha = 0.3 + 0.6 * torch.rand(H, W, generator=g)
    depth = 2.0 + torch.rand(H, W, generator=g)
    n = torch.nn.functional.normalize(torch.randn(3, H, W, generator=g), dim=0) * alpha
    allmap = torch.stack([depth * alpha, alpha, n[0], n[1], n[2], depth + 0.1 * torch.rand(H, W, generator=g),
                          0.01 * torch.rand(H, W, generator=g)])
    sensor = 2.0 + 1.5 * torch.rand(1, H, W, generator=g)
    sensor[0, 0, :3] = 0.0
    est = 0.2 + torch.rand(1, H, W, generator=g)
    est[0, 1, :2] = 0.0
    rays_d, rays_o = camera_rays(cam.world_view_transform, cam.full_proj_transform, W, H)
    return cam, allmap, rays_d, rays_o, sensor, est


@pytest.mark.parametrize("depth_ratio", [0.0, 1.0, 0.5])
def test_yardstick_agrees_with_float64_finite_differences(depth_ratio):
    """d total / d allmap by autograd against central differences in float64 (h = 1e-6), every one of the 7 x 120 entries -
    except the channels that carry the depth of the two pixels which attain the extrema of the estimate mask, where the
    reference detaches min / max (image_utils.py:87-91) and a difference quotient does not; the alpha that weights
    surf_normal is held fixed, as render() detaches it.  3e-7 of the gradient's maximum:
    h^2 times a third derivative of order one, plus 1e-16 / h of rounding."""
    from oracle.surfel_maps_ref import surfel_maps_ref
    cam, allmap, rays_d, rays_o, sensor, est = _small_case()
    w = (1.5, 2.0, 0.3)
    y = ref.surfel_terms_autograd(allmap, cam.world_view_transform, rays_d, rays_o, depth_ratio, sensor, est, *w)
    assert int(y["Ms"].sum()) > 60 and int(y["Me"].sum()) > 60 and float(y["Ldn"]) > 0 and float(y["Lrn"]) > 0
    a64 = allmap.double()
    v64, rd64, ro64 = cam.world_view_transform.double(), rays_d.double(), rays_o.double()

    def f(a):    # the total with surf_normal weighted by the UNPERTURBED alpha: what `alpha.detach()` means for a quotient
        _, rn, _, dd, sn = surfel_maps_ref(a, v64, rd64, ro64, depth_ratio)
        return float(ref.terms_from_maps(dd, rn, sn / a[1:2] * a64[1:2], rd64, ro64, sensor, est, *w, y["Ms"], y["Me"])[0])

    d = y["d"].double()[0]
    dm = torch.where(y["Me"][0], d, torch.full_like(d, float("nan")))
    extremal = (dm == dm[y["Me"][0]].min()) | (dm == dm[y["Me"][0]].max())
    assert int(extremal.sum()) == 2
    g, h, worst = y["g_allmap"], 1e-6, 0.0
    for c in range(7):
        for i in range(allmap.shape[1]):
            for j in range(allmap.shape[2]):
                if extremal[i, j] and c in (0, 1, 5):
                    continue
                ap, am = a64.clone(), a64.clone()
                ap[c, i, j] += h
                am[c, i, j] -= h
                worst = max(worst, abs((f(ap) - f(am)) / (2 * h) - float(g[c, i, j])))
    print(f"depth_ratio {depth_ratio}: max |autograd - finite difference| {worst:.3e} of max {float(g.abs().max()):.3e}")
    assert worst <= 3e-7 * float(g.abs().max())


def test_depth_normal_losses_and_the_isotropic_closed_form_agree_with_the_yardstick():
    """loss.depth_normal_losses (the package's torch form of train_2dgs.py:126-134, what the autograd branch uses) run in
    float64 on the yardstick's maps gives the yardstick's two values (1e-12); the [N,2] isotropic closed form of
    include/scorp_gs.h equals float64 autograd, with zeros for equal scales."""
    from oracle.surfel_maps_ref import surfel_maps_ref
    from scorp_amd.loss import depth_normal_losses, isotropic_loss
    cam, allmap, rays_d, rays_o, sensor, est = _small_case()
    y = ref.surfel_terms_autograd(allmap, cam.world_view_transform, rays_d, rays_o, 0.5, None, est, 0.0, 0.0, 1.0)
    _, rn, _, _, sn = surfel_maps_ref(allmap.double(), cam.world_view_transform.double(), rays_d.double(), rays_o.double(), 0.5)
    cam64 = type("Cam", (), {})()
    cam64.resolution = cam.resolution
    cam64.world_view_transform, cam64.full_proj_transform = cam.world_view_transform.double(), cam.full_proj_transform.double()
    import scorp_amd.renderer2d as R2
    old = R2._camera_rays
    R2._camera_rays = lambda view, dev: (rays_d.double(), rays_o.double())
    try:
        ldn, lrn = depth_normal_losses({"surf_normal": sn, "render_normal": rn}, cam64, est.double())
    finally:
        R2._camera_rays = old
    assert abs(float(ldn) - float(y["Ldn"])) <= 1e-12 and abs(float(lrn) - float(y["Lrn"])) <= 1e-12
    raw = torch.randn(500, 2, generator=torch.Generator().manual_seed(4)) * 0.7 - 3.0
    raw[:7] = raw[:7, :1]
    val, g_auto = ref.isotropic2_autograd(raw, 5e-4)
    assert abs(float(val) - float(isotropic_loss(torch.exp(raw.float()).double()))) <= 1e-12 * float(val)
    g_closed = ref.isotropic2_gradient_closed_form(raw, 5e-4)
    assert float((g_closed - g_auto).abs().max()) <= 1e-12 * float(g_auto.abs().max())
    assert float(g_closed[:7].abs().max()) == 0.0 and float(g_closed.abs().max()) > 0


class _FakeCam:
    def __init__(self, k):
        self.k = k


def _stand_in(calls):
    def view(cam, pc, pipe, bg, gt_image, lambda_dssim, lambda_normal, lambda_dist, **kw):
        calls.append((cam, gt_image, lambda_normal, lambda_dist, kw))
        radii = torch.ones(pc.get_xyz.shape[0], dtype=torch.int32)
        return {"loss": torch.tensor(0.25), "overflow": torch.zeros(1, dtype=torch.int32), "radii": radii,
                "visibility_filter": radii > 0, "viewspace_points": None, "render": gt_image, "optimizer_stepped": False}
    return view


def _surfel_model(opt):
    from scorp_amd.renderer2d import GaussianModel2D
    from scorp_amd.synthetic import make_gaussians
    m = GaussianModel2D.from_raw(make_gaussians(40, 1, 3, scale_dims=2), 1, device="cpu")
    m.training_setup(opt)
    return m


def test_late_surfel_iterations_go_through_the_one_call_view():
    """training_iteration(surfels=True, fused_view=True, view_fn=stand-in): at 7500 the view gets the sensor, estimate and
    isotropic keywords and weight_depth_normal == 0, at 8500 weight_depth_normal == dn_l1_weight(8500), at 6000 none of them."""
    from scorp_amd.gaussian_model import OptimizationParams2D, get_expon_lr_func
    from scorp_amd.train import PipelineParams, training_iteration
    import scorp_amd.train as T
    opt = OptimizationParams2D()
    opt.random_background = False
    m = _surfel_model(opt)
    sensor, est, gt = torch.rand(1, 8, 8) + 2, torch.rand(1, 8, 8), torch.rand(3, 8, 8)
    calls = []

    def no_render(*a, **k):
        raise AssertionError("the iteration left the one-call view for render() + autograd")

    old = T.depth_losses, T.depth_normal_losses
    T.depth_losses = T.depth_normal_losses = no_render
    try:
        for it in (7500, 8500, 6000):
            loss, _ = training_iteration(m, _FakeCam(0), gt, opt, PipelineParams(), torch.zeros(3), it, densify=False,
                                         surfels=True, fused_view=True, view_fn=_stand_in(calls), gt_depth=sensor,
                                         gt_depth_est=est)
            assert float(loss) == 0.25
    finally:
        T.depth_losses, T.depth_normal_losses = old
    assert len(calls) == 3
    dn = get_expon_lr_func(opt.dn_l1_weight_init, opt.dn_l1_weight_final, max_steps=opt.iterations)
    for it, (_, _, ln, ld, kw) in zip((7500, 8500), calls):
        assert kw["depth_sensor"] is sensor and kw["depth_est"] is est
        assert kw["lambda_depth_sensor"] == opt.lambda_depth_sensor and kw["weight_depth_est"] == 10 * dn(it)
        assert kw["lambda_isotropic"] == opt.lambda_isotropic > 0
        assert kw["weight_depth_normal"] == (dn(it) if it == 8500 else 0.0) and dn(8500) > 0
        assert ln == opt.lambda_normal and ld == opt.lambda_dist
    _, _, ln, ld, kw = calls[2]
    assert not any(k in kw for k in ("depth_sensor", "depth_est", "lambda_depth_sensor", "weight_depth_est",
                                     "weight_depth_normal", "lambda_isotropic"))
    assert ln == 0.0 and ld == opt.lambda_dist


def test_train_hands_each_camera_its_own_depth_maps_to_the_surfel_view():
    """train(surfels=True, gt_depths=, gt_depth_ests=): per-camera lists, indexed like gt_images."""
    from scorp_amd.gaussian_model import OptimizationParams2D
    from scorp_amd.train import train
    import scorp_amd.train as T
    opt = OptimizationParams2D()
    opt.random_background, opt.depth_from_iter = False, 0
    m = _surfel_model(opt)
    cams = [_FakeCam(k) for k in range(4)]
    gts = [torch.full((3, 8, 8), float(k)) for k in range(4)]
    sensors = [torch.full((1, 8, 8), 10.0 + k) for k in range(4)]
    ests = [torch.full((1, 8, 8), 20.0 + k) if k != 2 else None for k in range(4)]
    calls = []
    old = T._drain_reservation
    T._drain_reservation = lambda **kw: True       # (the reservation bookkeeping of real views: nothing is pending here)
    try:
        losses = train(m, cams, gts, opt, iterations=8, surfels=True, fused_view=True, view_fn=_stand_in(calls), densify=False,
                       gt_depths=sensors, gt_depth_ests=ests)
    finally:
        T._drain_reservation = old
    assert losses == [0.25] * 8 and sorted(c.k for c, *_ in calls) == [0, 0, 1, 1, 2, 2, 3, 3]
    for cam, gt, _, _, kw in calls:
        k = cam.k
        assert float(gt[0, 0, 0]) == float(k) and float(kw["depth_sensor"][0, 0, 0]) == 10.0 + k
        assert (kw.get("depth_est") is None) if k == 2 else float(kw["depth_est"][0, 0, 0]) == 20.0 + k
