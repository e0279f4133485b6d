"""Pins the yardstick of the loss kernels (tests/loss_reference.py) without a GPU: against the values captured from the
reference's own loss_utils, against closed forms, against finite differences, and loss.hip's window against torch's.

Window: the numpy float32 restatement of make_window() (exp in double, rounded to float32, a sequential float32 sum, a
divide) is NOT scorp_amd.loss.gaussian(11, 1.5): the largest difference is 1 ulp, in nine of the eleven taps.  The
sequential float32 sum is 3.7592325, torch's `g.sum()` 3.7592328 (the correctly rounded sum), so every tap of loss.hip is
larger by 6e-8 of itself before its own rounding.  The float64 reference of the GPU tests therefore uses the taps
loss.hip builds (loss_ref(window="kernel")).  Between the two windows the float64 gradient moves by 0.2 to 0.4 e_ref
(3e-7 to 6e-7 of max |grad|) and the mean SSIM by 1e-8 to 2e-8: printed by the window test below.

Which term of the bound binds (printed per case by test_sweep_references_are_finite_and_say_which_term_binds): for the
gradient 4 e_ref in 294 of 344 cases at lam = 0.2 and 337 of 344 at lam = 1, the 16-ulp floor at lam = 0 (all but one);
for L1 and the mean SSIM the floor; for the loss value the floor in about half the cases at lam = 0.2, 4 e_ref or
4 e_order at lam = 1."""
import numpy as np
import pytest
import torch

from tests import loss_reference as ref

# The dropped-tap mutant (tests/loss_reference.py::ssim_dropped_tap) in float64, as a share of max |grad|, at the four shapes
# of test_bound_catches_a_dropped_tap_row_at_the_strip_seam: lam = 1: 6.2e-4 (1x23x64), 6.4e-4 (3x47x133); lam = 0.2, where
# the L1 term's 0.8 / N sets max |grad|: 3.7e-4 (1x29x70), 1.3e-3 (4x51x65 masked).  With other random images the same four
# shapes gave 5.2e-4, 6.9e-4, 3.3e-4, 4.1e-4.  The smaller figure per lam is the one every sweep case of that lam is held
# to: its bound must be below a twentieth of it.
MUTANT_SHARE = {0.2: 3.3e-4, 1.0: 5.2e-4}


def test_reference_reproduces_the_golden_loss_and_gradient(golden):
    """g3 of ref_helpers.npz is a float32 run of the reference's own loss_utils: the float64 run with torch's window is
    within float32 rounding of it, and the float32 run is it."""
    a, b = torch.tensor(golden["g3_a"]), torch.tensor(golden["g3_b"])
    values, grad = ref.loss_ref(a, b, 0.2, window="torch")
    values32, grad32 = ref.loss_ref(a, b, 0.2, dtype=torch.float32, window="torch")
    g = torch.tensor(golden["g3_grad_a"]).double()
    scale = float(g.abs().max())
    print(f"golden: loss {float(golden['g3_loss']):.9f} f64 {float(values[0]):.9f} f32 {float(values32[0]):.9f}; grad f64 "
          f"{float((grad - g).abs().max()) / scale:.2e} f32 {float((grad32.double() - g).abs().max()) / scale:.2e} of max|grad|")
    assert abs(float(values[0]) - float(golden["g3_loss"])) < 2e-7
    assert float((grad - g).abs().max()) < 1e-5 * scale
    assert abs(float(values32[0]) - float(golden["g3_loss"])) < 2e-7
    assert float((grad32.double() - g).abs().max()) < 1e-5 * scale


def test_restated_ssim_is_ssim_torch():
    """ssim_windowed with the window of `create_window` gives the bits of `ssim_torch`, value and gradient, in both dtypes:
    the kernel-window reference differs from the torch formulation in its eleven taps and in nothing else."""
    from scorp_amd.loss import create_window, ssim_torch
    x, y, _ = ref.make_case((3, 29, 70), 7)
    for dtype in (torch.float64, torch.float32):
        a, b = x.to(dtype).requires_grad_(True), x.to(dtype).requires_grad_(True)
        s1, s2 = ref.ssim_windowed(a, y.to(dtype), create_window(11, 3).to(dtype)), ssim_torch(b, y.to(dtype))
        s1.backward(); s2.backward()
        assert torch.equal(s1, s2) and torch.equal(a.grad, b.grad)


def test_closed_forms():
    x, y, mask = ref.make_case((3, 24, 30), 1, "levels")
    for m in (None, mask):
        values, grad = ref.loss_ref(x, x.clone(), 0.2, m)
        assert abs(float(values[2]) - 1.0) < 1e-15 and float(values[1]) == 0.0 and abs(float(values[0])) < 1e-15
    # a pixel whose whole window sees constants a, b: SSIM = (2ab + C1) / (a^2 + b^2 + C1) (both variances and the covariance vanish)
    # ssim_torch returns only means, so the map is restated here and tied to the reference by its mean
    a, b, c1 = 0.7, 0.3, 0.01 ** 2
    ca, cb = torch.full((1, 21, 25), a, dtype=torch.float64), torch.full((1, 21, 25), b, dtype=torch.float64)
    import torch.nn.functional as F
    from scorp_amd.loss import create_window
    w = create_window(11, 1).double()
    conv = lambda t: F.conv2d(t, w, padding=5)
    mu1, mu2 = conv(ca), conv(cb)
    s1, s2, s12 = conv(ca * ca) - mu1 * mu1, conv(cb * cb) - mu2 * mu2, conv(ca * cb) - mu1 * mu2
    ssim_map = ((2 * mu1 * mu2 + c1) * (2 * s12 + 0.03 ** 2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + 0.03 ** 2))
    # (the float32 window sums to S = 1 - O(1e-7), which leaves a constant a "variance" a^2 S (1 - S) = O(1e-7) against
    # C2 = 9e-4: the closed form holds to O(1e-4) of 1 - SSIM, not to rounding)
    s = float(w.sum())
    assert abs(s - 1) < 5e-7
    assert float((ssim_map[:, 5:-5, 5:-5] - (2 * a * b + c1) / (a * a + b * b + c1)).abs().max()) < 2e-5
    exact = ((2 * s * s * a * b + c1) * (2 * a * b * s * (1 - s) + 0.03 ** 2)) / ((s * s * (a * a + b * b) + c1) * ((a * a + b * b) * s * (1 - s) + 0.03 ** 2))
    assert float((ssim_map[:, 5:-5, 5:-5] - exact).abs().max()) < 1e-12
    # ... and the mean the reference takes is the mean of that map
    assert abs(float(ref.loss_ref(ca, cb, 1.0, window="torch")[0][2]) - float(ssim_map.mean())) < 1e-15
    z = torch.zeros(2, 13, 17)
    for dtype in (torch.float64, torch.float32):
        values, grad = ref.loss_ref(z, z, 1.0, dtype=dtype)
        assert float(values[2]) == 1.0 and float(values[0]) == 0.0 and float(grad.abs().max()) == 0.0


def test_reference_gradient_by_finite_differences():
    g = torch.Generator().manual_seed(3)
    x = torch.rand((1, 6, 7), generator=g, dtype=torch.float64)
    y = (x + 0.05 + 0.1 * torch.rand((1, 6, 7), generator=g, dtype=torch.float64)) * torch.where(torch.rand((1, 6, 7), generator=g) > 0.5, 1.0, 0.5)
    assert float((x - y).abs().min()) > 1e-3          # |x - y| is not differentiable at x == y
    mask = torch.tensor(ref.MASK_LEVELS, dtype=torch.float64)[torch.randint(1, 4, (1, 6, 7), generator=g)]
    from scorp_amd.loss import l1_loss, ssim_torch
    for lam in (0.2, 1.0):
        for m in (None, mask):
            f = lambda t: (1 - lam) * l1_loss(t if m is None else t * m, y if m is None else y * m) + lam * (
                1 - ssim_torch(t if m is None else t * m, y if m is None else y * m))
            xg = x.clone().requires_grad_(True)
            assert torch.autograd.gradcheck(f, (xg,), eps=1e-6, atol=1e-7, rtol=1e-5)
            (by_autograd,) = torch.autograd.grad(f(xg), xg)
            assert torch.equal(by_autograd, ref.loss_ref(x, y, lam, m, window="torch")[1])      # loss_ref is that function


def test_window_of_the_kernels_is_one_ulp_from_the_window_of_torch():
    from scorp_amd.loss import gaussian
    mine, theirs = ref.window_restated(), gaussian(11, 1.5).numpy()
    assert mine.dtype == theirs.dtype == np.float32
    ulps = np.abs(mine.view(np.int32).astype(np.int64) - theirs.view(np.int32).astype(np.int64))
    print("window: largest difference", int(ulps.max()), "ulp, in", int((ulps > 0).sum()), "taps")
    assert int(ulps.max()) <= 1 and np.array_equal(mine, mine[::-1])
    # what the ulp is worth: the float64 reference with either window, against e_ref
    for shape, lam in (((1, 23, 64), 1.0), ((3, 47, 133), 0.2), ((1, 5, 7), 1.0)):
        x, y, _, r = ref.sweep_reference(shape, lam, None) if shape in ref.sweep_shapes() else (*ref.make_case(shape, 1), None)
        r = r or ref.Reference(x, y, lam)
        v, g = ref.loss_ref(x, y, lam, window="torch")
        moved = float((g - r.grad).abs().max())
        print(f"window {shape} lam {lam}: gradient {moved:.2e} = {moved / r.e_grad:.2f} e_ref = {moved / r.grad_scale:.1e} max|grad|; "
              f"mean SSIM {float(abs(v[2] - r.values[2])):.1e}")
        assert moved < r.tol_grad      # below the bound, so it cannot be what a failing case is about


def test_sweep_covers_the_tile_totals_of_the_xcd_map():
    totals = sorted({ref.tile_total(s) for s in ref.sweep_shapes()})
    print("backward tile totals in the sweep:", totals)
    assert {1, 7, 8, 9, 17} <= set(totals)
    assert len(set(ref.sweep_shapes())) == len(ref.sweep_shapes()) == 12 * 13 + 12 + 4


@pytest.mark.parametrize("shape", ref.sweep_shapes(), ids=lambda s: "x".join(map(str, s)))
def test_sweep_references_are_finite_and_say_which_term_binds(shape):
    for lam in ref.LAMBDAS:
        for kind in ref.MASK_KINDS:
            x, y, mask, r = ref.sweep_reference(shape, lam, kind)
            b = r.binds()
            print(f"loss-bound {shape} lam {lam} {'masked' if kind else 'plain'}: grad e_ref {r.e_grad:.3e} bound {r.tol_grad:.3e} "
                  f"= {r.tol_grad / max(r.grad_scale, 1e-300):.2e} max|grad| ({b['grad']}); values e_ref "
                  + " ".join(f"{e:.2e}" for e in r.e_values) + " (" + " ".join(b[n] for n in r.NAMES) + ")")
            assert all(np.isfinite(v) for v in [r.e_grad, r.tol_grad, *r.e_values, *r.tol_values])
            assert bool(torch.isfinite(r.grad).all()) and bool(torch.isfinite(r.values).all())
            if lam >= 0.2 and r.grad_scale > 0:
                # the mutant argument: the bound is below 1/20 of what a dropped tap row moves the gradient by
                assert r.tol_grad < MUTANT_SHARE[lam] / 20 * r.grad_scale, (shape, lam, kind, r.tol_grad / r.grad_scale)


@pytest.mark.parametrize("shape,lam,kind", [((1, 23, 64), 1.0, None), ((1, 29, 70), 0.2, None), ((3, 47, 133), 1.0, None),
                                            ((4, 51, 65), 0.2, "levels")])
def test_bound_catches_a_dropped_tap_row_at_the_strip_seam(shape, lam, kind):
    """In float64, without any kernel: output row 23 (the first of the second forward strip; at H = 23 the last row, 22)
    loses the topmost tap row of its window.  The gradient moves by more than 20 bounds."""
    from scorp_amd.loss import l1_loss
    x, y, mask = ref.make_case(shape, ref.shape_seed(shape), kind)
    r = ref.Reference(x, y, lam, mask)
    xd = x.double().requires_grad_(True)
    xm, ym = (xd, y.double()) if mask is None else (xd * mask.double(), y.double() * mask.double())
    wrong = (1 - lam) * l1_loss(xm, ym) + lam * (1 - ref.ssim_dropped_tap(xm, ym, min(23, shape[1] - 1)))
    (g,) = torch.autograd.grad(wrong, xd)
    moved = float((g - r.grad).abs().max())
    print(f"mutant {shape} lam {lam}: gradient moved {moved:.3e} = {moved / r.grad_scale:.2e} max|grad| = {moved / r.e_grad:.0f} e_ref; "
          f"bound {r.tol_grad:.3e}")
    assert moved >= MUTANT_SHARE[lam] * r.grad_scale
    assert moved > 20 * r.tol_grad
