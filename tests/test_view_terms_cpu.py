"""The late iterations' loss terms inside the one-call 3DGS view (scorp_gs3d_train_view_ex, ScorpGs3dViewTerms): what
can be checked without a GPU - the ABI, the argument checks (they run before any launch), the float64 yardstick the GPU
tests use against the package's own torch formulation and the closed forms the header states, and the routing of
training_iteration."""
import ctypes
import math
import os
import subprocess

import pytest
import torch

from tests import view_terms_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from scorp_amd import _C, build
    build.build()
    return _C.lib()


def test_new_symbols_are_declared_exported_and_bound(L):
    from scorp_amd import _C
    txt = open(os.path.join(ROOT, "include", "scorp_gs.h")).read()
    for name in ("scorp_gs3d_view_terms_workspace_bytes", "scorp_gs3d_train_view_ex", "scorp_gs3d_depth_terms"):
        assert name + "(" in txt and name in _C.EXPORTS and hasattr(L, name), name
    assert "SCORP_DEPTH_SENSOR_MIN 0.3f" in txt and "SCORP_DEPTH_SENSOR_MAX 7.0f" in txt


def test_view_terms_struct_has_the_headers_size(tmp_path):
    from scorp_amd import _C
    src = tmp_path / "t.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "scorp_gs.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", '
                   'sizeof(ScorpGs3dViewTerms), offsetof(ScorpGs3dViewTerms, lambda_isotropic), '
                   'offsetof(ScorpGs3dViewTerms, out_terms4), offsetof(ScorpGs3dViewTerms, workspace_bytes)); return 0; }\n')
    exe = tmp_path / "t"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    size, o_iso, o_out, o_wsb = (int(x) for x in subprocess.check_output([str(exe)]).split())
    T = _C.ScorpGs3dViewTerms
    assert (size, o_iso, o_out, o_wsb) == (ctypes.sizeof(T), T.lambda_isotropic.offset, T.out_terms4.offset, T.workspace_bytes.offset)


def test_workspace_bytes_is_monotone_and_nonzero(L):
    f = L.scorp_gs3d_view_terms_workspace_bytes
    assert f(0, 0, 0) > 0 and f(1, 1, 0) > 0
    sizes = [(64, 64, 0), (64, 64, 1000), (640, 480, 1000), (1600, 1200, 1000), (1600, 1200, 1_000_000), (4096, 4096, 8_000_000)]
    vals = [f(*s) for s in sizes]
    assert all(a <= b for a, b in zip(vals, vals[1:])), vals
    assert vals[0] < vals[-1] <= 64 * 1024       # per-workgroup partial sums: kilobytes, whatever the image


def _dummy_view(_C, keep):
    """A view that passes every check of scorp_gs3d_train_view itself: dummy non-NULL pointers, never dereferenced because
    the terms are checked before anything is launched."""
    d = 0x10000
    inp = _C.ScorpGs3dInputs(num_gaussians=100, sh_degree=1, sh_coeffs=4, image_width=64, image_height=48, tanfovx=1.0,
                             tanfovy=1.0, scale_modifier=1.0, bg=d, viewmatrix=d, projmatrix=d, campos=d, means3D=d, shs=d,
                             opacities=d, scales=d, rotations=d, shs_rest=d, raw_params=7)
    grads = _C.ScorpGs3dGrads()
    keep += [inp, grads]
    v = _C.ScorpGs3dTrainView()
    v.inputs, v.grads = ctypes.addressof(inp), ctypes.addressof(grads)
    for n in ("out_radii", "state", "pairs", "out_color", "out_depth_raw", "out_alpha", "out_depth", "out_visible", "gt", "out_loss3",
              "loss_workspace", "grad_color", "backward_scratch"):
        setattr(v, n, d)
    return v, inp


def _full_terms(_C, L):
    d = 0x10000
    t = _C.ScorpGs3dViewTerms()
    t.depth_sensor = t.depth_est = t.out_terms4 = t.grad_depth_raw = t.grad_alpha = t.workspace = d
    t.lambda_depth_sensor, t.weight_depth_est, t.lambda_isotropic = 1.5, 2.0, 5e-4
    t.workspace_bytes = L.scorp_gs3d_view_terms_workspace_bytes(64, 48, 100)
    return t


@pytest.mark.parametrize("case, reason", [
    ("out_terms4", b"out_terms4"), ("sensor_map", b"lambda_depth_sensor without depth_sensor"),
    ("est_map", b"weight_depth_est without depth_est"), ("grad_depth_raw", b"grad_depth_raw"), ("grad_alpha", b"grad_alpha"),
    ("out_depth", b"out_depth"), ("workspace", b"workspace"), ("workspace_small", b"too small"),
    ("workspace_misaligned", b"misaligned"), ("iso_layout", b"training layout")])
def test_train_view_ex_refuses_missing_buffers_before_any_launch(L, case, reason):
    """Each missing buffer is SCORP_ERR_INVALID with a message.  No GPU is needed and the dummy pointers are never touched:
    the checks run before the first launch."""
    from scorp_amd import _C
    keep = []
    v, inp = _dummy_view(_C, keep)
    t = _full_terms(_C, L)
    if case == "out_terms4":
        t.out_terms4 = None
    elif case == "sensor_map":
        t.depth_sensor = None
    elif case == "est_map":
        t.depth_est = None
    elif case == "grad_depth_raw":
        t.grad_depth_raw = None
    elif case == "grad_alpha":
        t.grad_alpha = None
    elif case == "out_depth":
        v.out_depth = None
    elif case == "workspace":
        t.workspace = None
    elif case == "workspace_small":
        t.workspace_bytes -= 1
    elif case == "workspace_misaligned":
        t.workspace = 0x10004
    elif case == "iso_layout":
        inp.shs_rest = None
    rc = L.scorp_gs3d_train_view_ex(ctypes.byref(v), ctypes.byref(t), None)
    assert rc == _C.ERR_INVALID
    assert reason in L.scorp_last_error(), L.scorp_last_error()


def _seeded_case(seed=3, H=40, W=56):
    g = torch.Generator().manual_seed(seed)
    alpha = torch.rand(H, W, generator=g)
    alpha[torch.rand(H, W, generator=g) < 0.15] = 0.0            # empty pixels: 0 / 0
    depth_raw = alpha * (1.5 + 3.0 * torch.rand(H, W, generator=g))
    sensor = 2.0 + 2.0 * torch.rand(H, W, generator=g)
    sensor[torch.rand(H, W, generator=g) < 0.1] = 0.0
    est = torch.rand(H, W, generator=g)
    est[torch.rand(H, W, generator=g) < 0.1] = 0.0
    return depth_raw, alpha, sensor, est


def test_yardstick_agrees_with_the_torch_formulation_and_the_closed_forms():
    """The float64 yardstick against scorp_amd.loss.depth_losses + isotropic_loss run in float64 (same expressions, the
    package's own code), and the closed forms of include/scorp_gs.h against float64 autograd: 1e-12."""
    from scorp_amd.gaussian_model import OptimizationParams, get_expon_lr_func
    from scorp_amd.loss import depth_losses, isotropic_loss
    depth_raw, alpha, sensor, est = _seeded_case()
    opt, it = OptimizationParams(), 7500
    w_s = opt.lambda_depth_sensor
    w_e = 10 * get_expon_lr_func(opt.dn_l1_weight_init, opt.dn_l1_weight_final, max_steps=opt.iterations)(it)
    r = ref.rendered_depth(depth_raw, alpha)
    y = ref.depth_terms_autograd(r, sensor, est, w_s, w_e)
    assert int(y["Ms"].sum()) > 100 and int(y["Me"].sum()) > 100
    # the package's formulation in float64 on the same float32 depth (the masks are taken on r, the float render() returns)
    r64 = r.double().requires_grad_(True)
    total = depth_losses(r64, it, opt, sensor.double(), est.double())
    assert abs(float(total.detach()) - float(y["total"])) <= 1e-12 * abs(float(y["total"]))
    total.backward()
    assert float((r64.grad - y["g_r"]).abs().max()) <= 1e-12 * float(y["g_r"].abs().max())
    # ... and the tail, r = nan_to_num(depth_raw / alpha), by autograd with the yardstick's gradient as the upstream one
    d64, a64 = depth_raw.double().requires_grad_(True), alpha.double().requires_grad_(True)
    (torch.nan_to_num(d64 / a64, 0, 0) * y["g_r"]).sum().backward()
    gd, ga = ref.tail_gradients(y["g_r"], depth_raw, alpha)
    # (autograd leaves 0 * inf = NaN at the empty pixels, which the rasterizer never reads: compared where alpha > 0)
    ok = alpha > 0
    assert float((d64.grad[ok] - gd[ok]).abs().max()) <= 1e-12 * float(gd.abs().max())
    assert float((a64.grad[ok] - ga[ok]).abs().max()) <= 1e-12 * float(ga.abs().max())
    assert float(gd[~ok].abs().max()) == 0.0 and float(ga[~ok].abs().max()) == 0.0 and float(gd.abs().max()) > 0
    # closed form of the gradient with respect to r
    gc = ref.depth_gradient_closed_form(r, sensor, est, w_s, w_e)
    assert float((gc - y["g_r"]).abs().max()) <= 1e-12 * float(gc.abs().max())
    assert torch.equal(gc != 0, y["g_r"] != 0)
    # isotropic regulariser
    raw = torch.randn(500, 3, generator=torch.Generator().manual_seed(4)) * 0.7 - 3.0
    raw[:7] = raw[:7, :1]                                           # a few isotropic Gaussians: sign(0) = 0
    lam = opt.lambda_isotropic
    val, g_auto = ref.isotropic_autograd(raw, lam)
    s64 = torch.exp(raw.float()).double()
    assert abs(float(val) - float(isotropic_loss(s64))) <= 1e-12 * float(val)
    g_closed = ref.isotropic_gradient_closed_form(raw, lam)
    assert float((g_closed - g_auto).abs().max()) <= 1e-12 * float(g_auto.abs().max())
    assert float(g_closed[:7].abs().max()) == 0.0


class _FakeCam:
    def __init__(self, k):
        self.k = k


def test_late_iterations_go_through_the_one_call_view():
    """training_iteration at iteration 7500 (> depth_from_iter) with fused_view=True: the view is called ONCE and receives
    the terms that apply - lambda_isotropic, the two maps, lambda_depth_sensor and weight_depth_est = 10 * dn_l1_weight(7500) -
    instead of the iteration leaving for render() + autograd."""
    from scorp_amd.gaussian_model import GaussianModel, OptimizationParams, get_expon_lr_func
    from scorp_amd.synthetic import make_gaussians
    from scorp_amd.train import PipelineParams, training_iteration
    m = GaussianModel.from_raw(make_gaussians(40, 1, 3), 1, device="cpu")
    opt = OptimizationParams()
    opt.random_background = False
    m.training_setup(opt)
    sensor, est, gt = torch.rand(1, 8, 8) + 2, torch.rand(1, 8, 8), torch.rand(3, 8, 8)
    calls = []

    def view(cam, pc, pipe, bg, gt_image, lambda_dssim, **kw):
        calls.append(kw)
        N = pc.get_xyz.shape[0]
        radii = torch.ones(N, dtype=torch.int32)
        return {"loss": torch.tensor(0.25), "overflow": torch.zeros(1, dtype=torch.int32), "radii": radii,
                "visibility_filter": radii > 0, "viewspace_points": None, "render": gt_image, "optimizer_stepped": False}

    def no_render(*a, **k):
        raise AssertionError("the iteration left the one-call view for render() + autograd")

    import scorp_amd.train as T
    it = 7500
    old = T.depth_losses
    T.depth_losses = no_render
    try:
        loss, pkg = training_iteration(m, _FakeCam(0), gt, opt, PipelineParams(), torch.zeros(3), it, densify=False,
                                       fused_view=True, view_fn=view, gt_depth=sensor, gt_depth_est=est)
    finally:
        T.depth_losses = old
    assert len(calls) == 1 and float(loss) == 0.25
    kw = calls[0]
    assert kw["lambda_isotropic"] == opt.lambda_isotropic == 0.0005
    assert kw["depth_sensor"] is sensor and kw["depth_est"] is est
    assert kw["lambda_depth_sensor"] == opt.lambda_depth_sensor
    w = get_expon_lr_func(opt.dn_l1_weight_init, opt.dn_l1_weight_final, max_steps=opt.iterations)(it)
    assert kw["weight_depth_est"] == 10 * w and 0.75 < 10 * w < 2.5 and math.isfinite(w)
    # before depth_from_iter, and with no term that applies, the view gets none of them
    calls.clear()
    training_iteration(m, _FakeCam(0), gt, opt, PipelineParams(), torch.zeros(3), 6999, densify=False, fused_view=True,
                       view_fn=view, gt_depth=sensor, gt_depth_est=est)
    assert len(calls) == 1 and not any(k in calls[0] for k in ("lambda_isotropic", "depth_sensor", "depth_est"))


def test_train_hands_each_camera_its_own_depth_maps():
    """train(gt_depths=, gt_depth_ests=): per-camera lists, indexed like gt_images."""
    from scorp_amd.gaussian_model import GaussianModel, OptimizationParams
    from scorp_amd.synthetic import make_gaussians
    from scorp_amd.train import train
    m = GaussianModel.from_raw(make_gaussians(40, 1, 3), 1, device="cpu")
    opt = OptimizationParams()
    opt.random_background, opt.depth_from_iter = False, 0
    cams = [_FakeCam(k) for k in range(4)]
    gts = [torch.full((3, 8, 8), float(k)) for k in range(4)]
    sensors = [torch.full((1, 8, 8), 10.0 + k) for k in range(4)]
    ests = [torch.full((1, 8, 8), 20.0 + k) if k != 2 else None for k in range(4)]
    seen = []

    def view(cam, pc, pipe, bg, gt_image, lambda_dssim, **kw):
        seen.append((cam.k, float(gt_image[0, 0, 0]), float(kw["depth_sensor"][0, 0, 0]),
                     None if kw.get("depth_est") is None else float(kw["depth_est"][0, 0, 0])))
        N = pc.get_xyz.shape[0]
        radii = torch.ones(N, dtype=torch.int32)
        return {"loss": torch.tensor(0.5), "overflow": torch.zeros(1, dtype=torch.int32), "radii": radii,
                "visibility_filter": radii > 0, "viewspace_points": None, "render": gt_image, "optimizer_stepped": False}

    import scorp_amd.train as T
    old = T._drain_reservation
    T._drain_reservation = lambda **kw: True       # (the reservation bookkeeping of real views: nothing is pending here)
    try:
        losses = train(m, cams, gts, opt, iterations=8, fused_view=True, view_fn=view, densify=False, gt_depths=sensors,
                       gt_depth_ests=ests)
    finally:
        T._drain_reservation = old
    assert losses == [0.5] * 8 and sorted(k for k, *_ in seen) == [0, 0, 1, 1, 2, 2, 3, 3]
    for k, g, s, e in seen:
        assert g == float(k) and s == 10.0 + k and e == (None if k == 2 else 20.0 + k)
