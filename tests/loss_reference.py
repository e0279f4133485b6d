"""Yardstick of the fused L1 + SSIM loss (scorp_amd/csrc/loss.hip, scorp_amd.fused_loss): the torch formulation
`(1 - lam) * l1_loss(x m, y m) + lam * (1 - ssim_torch(x m, y m))` of scorp_amd.loss on the CPU with a dtype argument, the
cases the tests run it on, and the bound the kernels are held to.  Not a test module: tests/test_loss_*.py import it.

The float64 run is the reference.  Its window is made of eleven float32 taps cast to double; the float32 taps are part
of the definition.  They are the taps loss.hip's make_window() builds (window_restated), which are 1 ulp from those of
`gaussian(11, 1.5)` in nine places (see loss_ref and tests/test_loss_cpu.py); loss_ref(window="torch") is `ssim_torch`
itself.  The float32 run exists only to measure e_ref = max |float32 - float64|, the error of a float32 evaluation of the
same sums in another order.

bound = max(4 e_ref, 2^-20 max |ref64|).  The factor 4 is the convention of the TSDF tests: the kernel and the float32 run
are both float32 evaluations of the same sums in a different order, and the kernel's two hardware reciprocals are 1 ulp
each.  The second term is a floor of 16 float32 ulps of the largest value: at lam = 0 the float32 run is nearly exact
(sign / N), while the kernel's `go * (float)(1 / N) * mk * g` rounds four times.
"""
import functools
import itertools
import math

import numpy as np
import torch
import torch.nn.functional as F

from scorp_amd.loss import l1_loss, ssim_torch

LAMBDAS = (0.0, 0.2, 1.0)
MASK_KINDS = (None, "levels")
MASK_LEVELS = (0.0, 0.25, 0.5, 1.0)

# The forward works in strips of 64 columns x 23 rows with a 5-pixel halo (lanes 0-9 carry columns cx0+59 .. cx0+68), the
# backward in 32x32 tiles dealt in eighths to the 8 XCDs.  Every H with every W at C = 1, then C = 3 and 4 at SWEEP_MULTI.
SWEEP_H = (1, 5, 6, 11, 22, 23, 24, 28, 29, 46, 47, 51)
SWEEP_W = (1, 5, 6, 11, 59, 63, 64, 65, 69, 70, 74, 128, 133)
SWEEP_MULTI = ((23, 64), (24, 65), (47, 133), (33, 33), (32, 96), (65, 70))
# Backward tile totals C * ceil(W / 32) * ceil(H / 32):  C = 1: 1, 2, 3, 4, 5, 6, 8, 10;  C = 3: 6, 9, 30, 12, 9, 27;
# C = 4: 8, 12, 40, 16, 12, 36.  7 and 17 are in neither, so four more shapes: 7 as seven channels of one tile and as
# seven tiles in a row, 17 likewise (17 tiles: three per XCD, the last XCD's share cut short).
SWEEP_EXTRA = ((7, 6, 11), (1, 29, 200), (17, 5, 6), (1, 11, 530))


def sweep_shapes():
    return ([(1, h, w) for h, w in itertools.product(SWEEP_H, SWEEP_W)]
            + [(c, h, w) for c in (3, 4) for h, w in SWEEP_MULTI] + list(SWEEP_EXTRA))


def tile_total(shape):
    c, h, w = shape
    return c * ((w + 31) // 32) * ((h + 31) // 32)


def shape_seed(shape):
    c, h, w = shape
    return (c * 1000 + h) * 1000 + w


def make_case(shape, seed, mask_kind=None):
    """(x, y, mask) as float32 CPU tensors: x = rand, y = clamp(x + 0.1 randn, 0, 1), y == x on the top-left H//2 x W//3
    block (there sign(x - y) = 0 and the L1 gradient must be exactly zero).  x and y do not depend on mask_kind.

    The mask ("levels") takes values in {0, 0.25, 0.5, 1} only.  Multiplying by a power of two is exact in float32, so
    x m - y m has the same sign in float32 and in float64, and "masked" and "multiplied by the mask beforehand, the
    gradient scaled by the mask afterwards" give identical bits: the bit comparisons of the GPU tests and the float64
    comparison see the same function."""
    c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=g)
    y = (x + 0.1 * torch.randn(shape, generator=g)).clamp(0, 1)
    y[:, : h // 2, : w // 3] = x[:, : h // 2, : w // 3]
    levels = torch.tensor(MASK_LEVELS)[torch.randint(0, len(MASK_LEVELS), (1, h, w), generator=g)]
    assert mask_kind in MASK_KINDS
    return x, y, (levels if mask_kind == "levels" else None)


def window2d(taps, channels, dtype):
    """[C, 1, 11, 11] from eleven float32 taps, the way `create_window` forms it: the float32 outer product, cast.  At
    float64 the products are exact instead (the kernels apply the window separably and never round a product of two
    taps), which differs from the cast by 2^-24 per tap at the most."""
    t = torch.as_tensor(np.asarray(taps, dtype=np.float32))
    w = torch.outer(t.double(), t.double()) if dtype == torch.float64 else torch.outer(t, t).to(dtype)
    return w.expand(channels, 1, 11, 11).contiguous()


def ssim_windowed(x, y, window):
    """`ssim_torch` statement for statement, with the window given: [C, H, W] -> mean SSIM."""
    c = x.size(-3)
    conv = lambda t: F.conv2d(t, window, padding=5, groups=c)
    mu1, mu2 = conv(x), conv(y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = conv(x * x) - mu1_sq
    sigma2_sq = conv(y * y) - mu2_sq
    sigma12 = conv(x * y) - mu1_mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu1_mu2 + c1) * (2 * sigma12 + c2)) / ((mu1_sq + mu2_sq + c1) * (sigma1_sq + sigma2_sq + c2))).mean()


def loss_ref(x, y, lam, mask=None, dtype=torch.float64, window="kernel"):
    """-> (values [3] = (loss, L1, mean SSIM), d loss / d x), both of `dtype`, on the CPU.  The inputs are cast, so the
    float64 run starts from the same float32 numbers as the kernels.

    window = "torch": `ssim_torch` itself, whose window is the float32 one of `create_window` cast to `dtype`.
    window = "kernel" (what the GPU tests compare with): the same statements with the eleven float32 taps loss.hip's
    make_window() builds (window_restated below).  Those are NOT the taps of `gaussian(11, 1.5)`: make_window() sums
    the taps one after the other in float32 and arrives 1 ulp below torch's `g.sum()` (which is the correctly rounded
    sum here), so nine of its eleven taps are 1 ulp larger.  The float32 taps are part of the definition either way."""
    xd = x.detach().to("cpu", dtype).requires_grad_(True)
    yd = y.detach().to("cpu", dtype)
    xm, ym = xd, yd
    if mask is not None:
        md = mask.detach().to("cpu", dtype).expand(1, *xd.shape[-2:])
        xm, ym = xd * md, yd * md
    l1 = l1_loss(xm, ym)
    assert window in ("kernel", "torch")
    ss = ssim_torch(xm, ym) if window == "torch" else ssim_windowed(xm, ym, window2d(window_restated(), xd.size(-3), dtype))
    loss = (1 - lam) * l1 + lam * (1 - ss)
    (grad,) = torch.autograd.grad(loss, xd)
    return torch.stack([loss, l1, ss]).detach(), grad


def tolerance(ref64, ref32):
    """max(4 e_ref, 2^-20 max |ref64|), e_ref = max |ref32 - ref64|: over a whole map, or of one value."""
    e_ref = float((ref32.double() - ref64).abs().max())
    return max(4 * e_ref, 2.0 ** -20 * float(ref64.abs().max()))


class Reference:
    """The float64 and float32 runs of one (x, y, lam, mask), and the bounds that follow from them.

    The loss value alone has the bound max(4 max(e_ref, e_order), floor), e_order = |kernel_order_values - float64|: at
    lam = 1 the loss is 1 - mean SSIM, a small difference that inherits the absolute error of a mean SSIM near 1, and
    the kernels' float32 order (kernel_order_values: no kernel involved) is that far from float64 where torch's order
    happens not to be.  See tests/test_loss_gpu.py for the cases where it binds."""
    NAMES = ("loss", "l1", "ssim")

    def __init__(self, x, y, lam, mask=None):
        self.values, self.grad = loss_ref(x, y, lam, mask, torch.float64)
        self.values32, self.grad32 = loss_ref(x, y, lam, mask, torch.float32)
        self.e_grad = float((self.grad32.double() - self.grad).abs().max())
        self.e_values = [float(abs(self.values32[i].double() - self.values[i])) for i in range(3)]
        self.tol_grad = tolerance(self.grad, self.grad32)
        self.tol_values = [tolerance(self.values[i], self.values32[i]) for i in range(3)]
        self.e_order = abs(float(kernel_order_values(x, y, lam, mask)[0]) - float(self.values[0]))
        self.tol_values[0] = max(self.tol_values[0], 4 * self.e_order)
        self.grad_scale = float(self.grad.abs().max())

    def binds(self):
        """Which term of the bound binds: per quantity "4e_ref" or "floor", for the loss value also "4e_order"."""
        pick = lambda e, tol: "4e_ref" if 4 * e >= tol else "floor"
        b = {"grad": pick(self.e_grad, self.tol_grad), **{n: pick(self.e_values[i], self.tol_values[i]) for i, n in enumerate(self.NAMES)}}
        if 4 * self.e_order >= self.tol_values[0] and self.e_order > self.e_values[0]:
            b["loss"] = "4e_order"
        return b

    def errors(self, values, grad, scale=1.0):
        """|got - ref64|: the gradient's maximum over the map (the gradient divided by `scale` in double first), then the
        three values."""
        v = values.detach().cpu().double().reshape(3)
        g = grad.detach().cpu().double() / scale
        return float((g - self.grad).abs().max()), [float(abs(v[i] - self.values[i])) for i in range(3)]

    def check(self, values, grad, what, scale=1.0, which=("grad", "loss", "l1", "ssim")):
        """Prints every figure, then asserts the quantities named in `which` against their bounds (all of them are
        looked at before the assertion).  `scale`: the upstream gradient the caller's backward ran with."""
        err_g, err_v = self.errors(values, grad, scale)
        b = self.binds()
        print(f"loss-ref {what}: grad err {err_g:.3e} e_ref {self.e_grad:.3e} bound {self.tol_grad:.3e} ({b['grad']}) max|grad| "
              f"{self.grad_scale:.3e}; " + "; ".join(f"{n} err {err_v[i]:.3e} e_ref {self.e_values[i]:.3e} bound {self.tol_values[i]:.3e} ({b[n]})"
                                                     for i, n in enumerate(self.NAMES)) + f"; e_order {self.e_order:.3e}")
        missed = [f"{what}: gradient {err_g:.3e} from float64, bound {self.tol_grad:.3e}"] if "grad" in which and not err_g <= self.tol_grad else []
        missed += [f"{what}: {n} {err_v[i]:.3e} from float64, bound {self.tol_values[i]:.3e}" for i, n in enumerate(self.NAMES)
                   if n in which and not err_v[i] <= self.tol_values[i]]
        assert not missed, "; ".join(missed)
        return missed


@functools.lru_cache(maxsize=None)
def sweep_reference(shape, lam, mask_kind):
    """The reference of one sweep case, computed once per process and left unchanged: (x, y, mask, Reference)."""
    x, y, mask = make_case(shape, shape_seed(shape), mask_kind)
    return x, y, mask, Reference(x, y, lam, mask)


def window_restated():
    """loss.hip's make_window() in numpy float32, in its order: exp in double, rounded to float32, a sequential float32
    sum, then a float32 divide of every tap."""
    w = [np.float32(math.exp(-float((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5))) for i in range(11)]
    s = np.float32(0.0)
    for v in w:
        s = np.float32(s + v)
    return np.array([np.float32(v / s) for v in w], dtype=np.float32)


def _fma(a, b, c):
    """float32 a * b + c with the product unrounded, as the tap sums compile to: the product of two float32 numbers is
    exact in double, and the double sum is rounded once more on its way to float32."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def kernel_order_values(x, y, lam, mask=None):
    """The three values (loss, L1, mean SSIM) by a numpy float32 restatement of loss.hip's forward and finalize, operation
    by operation in the kernel's order: (x m, y m, fma(y, y, x^2), xy) per pixel, eleven horizontal taps left to right and
    then eleven vertical taps top to bottom as fused multiply-adds, then ssim_pixel() of loss.hip, which rounds every
    operation on its own: ONE combined second moment (B2 = (E[x^2 + y^2] - mu1^2 - mu2^2) + C2, where torch subtracts
    twice), A1 A2 times the product of two reciprocals; float32 sums per lane down a 64 x 23 strip and across its 64
    lanes as a butterfly, the strips' sums in double, lambda a float32.

    What it cannot restate is the hardware reciprocal.  The kernel refines it by one Newton step, which is the correctly
    rounded reciprocal in all but rare cases; here it is a correctly rounded float32 divide.  So this measures e_order =
    |these values - float64|, the error of THIS float32 order, without any kernel."""
    f32 = np.float32
    xm, ym = x.detach().cpu().numpy().astype(f32), y.detach().cpu().numpy().astype(f32)
    if mask is not None:
        m = np.broadcast_to(mask.detach().cpu().numpy().astype(f32).reshape(1, *xm.shape[-2:]), xm.shape)
        xm, ym = xm * m, ym * m
    c, h, w = xm.shape
    taps = window_restated()
    moments = []
    for plane in (xm, ym, _fma(ym, ym, xm * xm), xm * ym):
        pad = np.zeros((c, h + 10, w + 10), f32)
        pad[:, 5:5 + h, 5:5 + w] = plane
        hor = np.zeros((c, h + 10, w), f32)
        for k in range(11):
            hor = _fma(taps[k], pad[:, :, k:k + w], hor)
        ver = np.zeros((c, h, w), f32)
        for k in range(11):
            ver = _fma(taps[k], hor[:, k:k + h, :], ver)
        moments.append(ver)
    m1, m2, ess, e12 = moments
    c1, c2 = f32(0.01) * f32(0.01), f32(0.03) * f32(0.03)
    m1s, m2s, m12 = m1 * m1, m2 * m2, m1 * m2
    s12 = e12 - m12
    a1, a2, b1, b2 = f32(2) * m12 + c1, f32(2) * s12 + c2, m1s + m2s + c1, (ess - m1s - m2s) + c2
    inv = (f32(1) / b1) * (f32(1) / b2)
    ssim = a1 * a2 * inv
    assert ssim.dtype == f32

    def strip_sums(v):      # per wave: every lane down its rows, then the lanes' butterfly; lane 0's sum, all waves in double
        sy, sx = -(-h // 23), -(-w // 64)
        full = np.zeros((c, sy * 23, sx * 64), f32)
        full[:, :h, :w] = v
        lanes = full.reshape(c, sy, 23, sx, 64)
        acc = np.zeros((c, sy, sx, 64), f32)
        for r in range(23):
            acc = acc + lanes[:, :, r]
        idx = np.arange(64)
        for off in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[..., idx ^ off]
        return float(acc[..., 0].astype(np.float64).sum())
    n = float(c * h * w)
    l1, ss, lam32 = strip_sums(np.abs(xm - ym)) / n, strip_sums(ssim) / n, float(f32(lam))
    return np.array([(1.0 - lam32) * l1 + lam32 * (1.0 - ss), l1, ss]).astype(f32)


def ssim_dropped_tap(x, y, row):
    """A deliberately wrong mean SSIM in the dtype of x: output row `row` loses the outermost (topmost) tap row of its 11x11
    window, as an off-by-one halo at a strip seam would do.  What the bounds have to catch; see test_loss_cpu.py."""
    c = x.size(-3)
    full = window2d(window_restated(), c, x.dtype)
    cut = full.clone()
    cut[:, :, 0, :] = 0
    sel = torch.zeros(x.shape[-2], 1, dtype=torch.bool)
    sel[row] = True

    def conv(t):
        return torch.where(sel, F.conv2d(t, cut, padding=5, groups=c), F.conv2d(t, full, padding=5, groups=c))
    mu1, mu2 = conv(x), conv(y)
    s1, s2, s12 = conv(x * x) - mu1 * mu1, conv(y * y) - mu2 * mu2, conv(x * y) - mu1 * mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))).mean()
