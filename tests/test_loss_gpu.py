"""GPU parity of the fused L1+SSIM loss: against the golden values captured from the reference's own
loss_utils (tests/golden/ref_helpers.npz, G3), against the torch formulation on ragged / masked inputs, and against the
float64 yardstick of tests/loss_reference.py (bound max(4 e_ref, 2^-20 max |ref64|), see there) at the shapes where the
kernels' strips (64 columns x 23 rows, 5-pixel halo), tiles (32 x 32, dealt to 8 XCDs) and partial-sum loops end."""
import ctypes

import numpy as np
import pytest
import torch

from tests import loss_reference as lossref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def test_fused_loss_matches_reference_golden(golden, dev):
    from scorp_amd.fused_loss import fused_l1_ssim_loss
    a = torch.tensor(golden["g3_a"], device=dev, requires_grad=True)
    b = torch.tensor(golden["g3_b"], device=dev)
    loss = fused_l1_ssim_loss(a, b, 0.2)
    loss.backward()
    assert abs(loss.item() - float(golden["g3_loss"])) < 2e-6
    np.testing.assert_allclose(a.grad.cpu().numpy(), golden["g3_grad_a"], atol=2e-9, rtol=2e-3)


@pytest.mark.parametrize("shape,masked,lam", [((3, 97, 131), False, 0.2), ((3, 64, 64), True, 0.2), ((1, 33, 200), False, 0.5),
                                             ((3, 1200, 1600), False, 0.2), ((3, 5, 7), True, 0.8)])
def test_fused_loss_matches_torch_formulation(shape, masked, lam, dev):
    from scorp_amd.fused_loss import fused_l1_ssim_loss
    from scorp_amd.loss import l1_loss, ssim_torch as ssim
    g = torch.Generator(device=dev).manual_seed(shape[1])
    x = torch.rand(shape, device=dev, generator=g)
    y = (x + 0.1 * torch.randn(shape, device=dev, generator=g)).clamp(0, 1)
    y[:, : shape[1] // 2, : shape[2] // 3] = x[:, : shape[1] // 2, : shape[2] // 3]      # exact-equal region: sign(0) = 0
    mask = (torch.rand((1,) + shape[1:], device=dev, generator=g) > 0.3).float() if masked else None
    up = torch.tensor(1.7, device=dev)
    x1 = x.clone().requires_grad_(True)
    fused = fused_l1_ssim_loss(x1, y, lam, mask)
    parts = fused.grad_fn.parts
    (fused * up).backward()
    if shape[1] * shape[2] <= 200 * 300:      # (a float64 CPU convolution at 1200x1600 is too slow for a test)
        lossref.Reference(x, y, lam, mask).check(parts, x1.grad, f"parity {shape} lam {lam}", scale=up.item())
    x2 = x.clone().requires_grad_(True)
    xm, ym = (x2 * mask, y * mask) if masked else (x2, y)
    ref = (1 - lam) * l1_loss(xm, ym) + lam * (1 - ssim(xm, ym))
    (ref * up).backward()
    got = fused_l1_ssim_loss(x, y, lam, mask)
    assert abs(got.item() - ref.item()) < 5e-6
    scale = x2.grad.abs().max().item()
    assert (x1.grad - x2.grad).abs().max().item() < 2e-3 * scale


@pytest.mark.parametrize("shape,box", [((3, 200, 300), (60, 120, 100, 180)), ((3, 1200, 1600), (500, 700, 640, 980)),
                                       ((1, 97, 131), (0, 9, 120, 131)), ((3, 64, 200), (0, 0, 0, 0))])
def test_masked_loss_over_mostly_empty_mask_takes_the_same_values(shape, box, dev):
    """A mask that is one object's silhouette (post_refine_gs.py:103-111) leaves most strips / tiles of the image empty; the
    kernels answer those from constants.  Against the torch formulation, and BIT FOR BIT against the same kernels run the
    long way round (no mask, inputs multiplied by it beforehand): the loss value, and the gradient = unmasked gradient x mask."""
    from scorp_amd.fused_loss import fused_l1_ssim_loss
    from scorp_amd.loss import l1_loss, ssim_torch as ssim
    lam = 0.2
    g = torch.Generator(device=dev).manual_seed(shape[2])
    x = torch.rand(shape, device=dev, generator=g)
    y = (x + 0.1 * torch.randn(shape, device=dev, generator=g)).clamp(0, 1)
    mask = torch.zeros((1,) + shape[1:], device=dev)
    mask[:, box[0]:box[1], box[2]:box[3]] = (torch.rand((1, box[1] - box[0], box[3] - box[2]), device=dev, generator=g) > 0.1).float()
    x1 = x.clone().requires_grad_(True)
    l_masked = fused_l1_ssim_loss(x1, y, lam, mask)
    l_masked.backward()
    xm = (x * mask).requires_grad_(True)
    l_plain = fused_l1_ssim_loss(xm, y * mask, lam)
    l_plain.backward()
    assert l_masked.item() == l_plain.item()
    assert torch.equal(x1.grad, xm.grad * mask)
    if shape[1] * shape[2] <= 200 * 300:
        lossref.Reference(x, y, lam, mask).check(l_masked.grad_fn.parts, x1.grad, f"mostly empty mask {shape} box {box}")
    x2 = x.clone().requires_grad_(True)
    ref = (1 - lam) * l1_loss(x2 * mask, y * mask) + lam * (1 - ssim(x2 * mask, y * mask))
    ref.backward()
    assert abs(l_masked.item() - ref.item()) < 5e-6
    assert (x1.grad - x2.grad).abs().max().item() <= 2e-3 * max(x2.grad.abs().max().item(), 1e-12)


def test_ssim_by_the_reference_name_is_served_by_the_hip_kernels(dev):
    """`scorp_amd.loss.ssim(image, gt)` as train_3dgs.py:107 calls it: value and gradient of the torch formulation, from the HIP
    loss kernels; other argument forms (a window size, per-image means, a batch dimension, CPU tensors) take the torch form."""
    from scorp_amd.loss import l1_loss, ssim, ssim_torch
    g = torch.Generator(device=dev).manual_seed(5)
    x = torch.rand((3, 120, 200), device=dev, generator=g)
    y = (x + 0.1 * torch.randn((3, 120, 200), device=dev, generator=g)).clamp(0, 1)
    x1, x2 = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    a = 0.8 * l1_loss(x1, y) + 0.2 * (1.0 - ssim(x1, y))
    b = 0.8 * l1_loss(x2, y) + 0.2 * (1.0 - ssim_torch(x2, y))
    assert type(ssim(x1, y).grad_fn).__name__ != type(ssim_torch(x2, y).grad_fn).__name__   # (not the same graph)
    a.backward(); b.backward()
    assert abs(a.item() - b.item()) < 5e-6
    assert (x1.grad - x2.grad).abs().max().item() < 2e-3 * x2.grad.abs().max().item()
    assert abs(ssim(x, y, 7).item() - ssim_torch(x, y, 7).item()) == 0.0                       # torch form
    assert torch.equal(ssim(x[None], y[None], 11, False), ssim_torch(x[None], y[None], 11, False))
    assert abs(ssim(x.cpu(), y.cpu()).item() - ssim_torch(x.cpu(), y.cpu()).item()) == 0.0


def test_host_patched_reference_ssim_runs_on_the_hip_kernels(dev):
    """scorp_amd.hostpatch.patch_ssim (SCORP_AMD_ACCELERATE=1): a module-level torch `ssim` - here a clone of the torch formulation
    in a module of its own, standing in for gs3dgs/utils/loss_utils.py - keeps its function object and answers GPU calls of the
    training shape from the HIP loss kernels: same value and gradient as its original code (kept as `ssim_torch`)."""
    import inspect
    import types
    import scorp_amd.loss as L
    from scorp_amd.hostpatch import patch_ssim
    mod = types.ModuleType("standin.loss_utils")
    exec(compile(inspect.getsource(L), "standin_loss_utils.py", "exec"), mod.__dict__)
    mod.ssim = types.FunctionType(mod.ssim_torch.__code__, mod.__dict__, "ssim", mod.ssim_torch.__defaults__)
    early = mod.ssim
    assert patch_ssim(mod) and mod.ssim is early and not patch_ssim(mod)
    g = torch.Generator(device=dev).manual_seed(11)
    x = torch.rand((3, 150, 170), device=dev, generator=g)
    y = (x + 0.1 * torch.randn((3, 150, 170), device=dev, generator=g)).clamp(0, 1)
    x1, x2 = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    a, b = early(x1, y), mod.ssim_torch(x2, y)
    assert any("FusedL1SSIM" in type(f[0]).__name__ for f in a.grad_fn.next_functions if f[0] is not None)   # (1 - fused loss)
    a.backward(); b.backward()
    assert abs(a.item() - b.item()) < 5e-6
    assert (x1.grad - x2.grad).abs().max().item() < 2e-3 * x2.grad.abs().max().item()
    assert torch.equal(early(x, y, 7), mod.ssim_torch(x, y, 7))            # other arguments: the original code


def _fused(x, y, lam, mask, dev):
    """-> (the three values (loss, L1, mean SSIM) [3], d loss / d x), through the autograd wrapper."""
    from scorp_amd.fused_loss import fused_l1_ssim_loss
    xg = x.to(dev).detach().requires_grad_(True)                  # (keeps the strides of x)
    assert xg.stride() == x.stride()
    loss = fused_l1_ssim_loss(xg, y.to(dev), lam, None if mask is None else mask.to(dev))
    parts = loss.grad_fn.parts
    loss.backward()
    return parts, xg.grad


def _sweep(shape, dev, which):
    missed = []
    for lam in lossref.LAMBDAS:
        for kind in lossref.MASK_KINDS:
            x, y, mask, r = lossref.sweep_reference(shape, lam, kind)
            values, grad = _fused(x, y, lam, mask, dev)
            try:
                r.check(values, grad, f"sweep {shape} lam {lam} {'masked' if kind else 'plain'}", which=which)
            except AssertionError as e:      # (every case of the shape is run and printed before the test fails)
                missed.append(str(e))
    assert not missed, "\n".join(missed)


@pytest.mark.parametrize("shape", lossref.sweep_shapes(), ids=lambda s: "x".join(map(str, s)))
def test_edge_sweep_against_float64(shape, dev):
    """Every H with every W of loss_reference.SWEEP_H / SWEEP_W at C = 1, C = 3 and 4 at SWEEP_MULTI, and SWEEP_EXTRA for
    the tile totals 7 and 17; each at lam = 0, 0.2, 1, plain and under the four-level mask: the gradient, the L1 value
    and the mean SSIM against float64.  (The third value, the loss itself: the next test.)"""
    _sweep(shape, dev, ("grad", "l1", "ssim"))


# The loss value, measured on an MI355X.  At lam = 1 it is 1 - mean SSIM: 1 ulp of a mean SSIM near 1 (6e-8) is many ulps
# of the difference, and the bound max(4 e_ref, 2^-20 |loss|) is 1.6e-8 .. 1e-7 there.
#   With bare hardware reciprocals (v_rcp_f32: 1 ulp, erring to one side) the forward kernel was over that bound in 35 of
#   the 1032 sweep cases, by up to 2.1e-7 absolute (1x51x1 plain: 8.4e-8 against a bound of 1.6e-8, 1x23x1 plain: 2.1e-7
#   against 9.8e-8): every pixel of a 51- to 3000-pixel image 1 ulp low.  loss.hip::ssim_pixel now gives each reciprocal one
#   Newton step and rounds every operation of the SSIM expression on its own, in the order written.
#   With that the kernel returns, in ALL 1032 sweep cases, the float32 number that the numpy restatement of its order
#   (tests/loss_reference.py::kernel_order_values, reciprocals as correctly rounded divides) returns: |kernel - float64| =
#   e_order.  What is left over 4 e_ref is therefore the rounding of this float32 order (one combined second moment, the
#   product of two reciprocals), shown without a kernel, and the loss value is held to max(4 max(e_ref, e_order), floor).
#   e_order is the binding term in 46 sweep cases, all of them images of fewer than 4500 pixels, e.g.
#   (kernel = e_order | e_ref, units of 1e-8): 1x1x1 m (lam 0.2) 1.19 | 0;  1x5x64 m 8.78 | 0.72;  1x6x59 p 7.03 | 0.61;
#   1x11x1 p 10.2 | 2.01;  1x23x1 p 12.8 | 2.44;  1x28x70 m 4.64 | 0.015;  1x46x1 m 6.25 | 0.48;  3x23x64 m 3.55 | 0.36;
#   and in the older tests at (3, 5, 7) lam 0.8 and under the mostly empty masks (the all-zero mask: mean SSIM 1 - 2^-23
#   where float64 and float32 torch both give exactly 1).  Worst |kernel - float64| / bound of the loss value: 0.25.
@pytest.mark.parametrize("shape", lossref.sweep_shapes(), ids=lambda s: "x".join(map(str, s)))
def test_edge_sweep_loss_value_against_float64(shape, dev):
    """The same sweep, the loss value out[0] = (1 - lam) L1 + lam (1 - mean SSIM): bound max(4 max(e_ref, e_order), floor);
    see the comment above for what it found."""
    _sweep(shape, dev, ("loss",))


_SENTINEL = 0xFF      # (as float32 a NaN: a read outside a region would not go unnoticed either)


class _Carved:
    """`nbytes` in the middle of a larger allocation filled with the sentinel byte, `lead` >= 256 bytes before it and at
    least 256 after it."""

    def __init__(self, nbytes, lead, dev):
        self.whole = torch.full((lead + nbytes + 300,), _SENTINEL, dtype=torch.uint8, device=dev)
        assert lead >= 256 and self.whole.data_ptr() % 256 == 0
        self.lead, self.nbytes = lead, nbytes
        self.ptr = ctypes.c_void_p(self.whole.data_ptr() + lead)

    def region(self):
        return self.whole[self.lead:self.lead + self.nbytes]

    def floats(self):
        return self.region().view(torch.float32)

    def guards_intact(self):
        return bool((self.whole[:self.lead] == _SENTINEL).all()) and bool((self.whole[self.lead + self.nbytes:] == _SENTINEL).all())


def _abi_call(x, y, mask, lam, dev, need_backward=1, grad_out="null", backward=True):
    """One forward (+ backward) through the C ABI with workspace, grad_img and out_loss3 carved out of sentinel-filled
    allocations -> (workspace, out_loss3, grad_img) as _Carved."""
    from scorp_amd import _C
    L = _C.lib()
    C, H, W = x.shape
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(_C.current_stream_ptr())
    ws_bytes = L.scorp_loss_workspace_bytes(C, H, W)
    ws, out, grad = _Carved(ws_bytes, 272, dev), _Carved(12, 268, dev), _Carved(4 * C * H * W, 260, dev)   # 16-, 4-, 4-aligned
    assert ws.ptr.value % 16 == 0 and ws.ptr.value % 32 != 0
    _C.check(L.scorp_loss_l1_ssim_forward(p(x), p(y), p(mask), C, H, W, lam, out.ptr, ws.ptr, ws_bytes, need_backward, stream),
             "scorp_loss_l1_ssim_forward")
    if backward:
        go = None if grad_out == "null" else torch.tensor([grad_out], dtype=torch.float32, device=dev)
        _C.check(L.scorp_loss_l1_ssim_backward(p(x), p(y), p(mask), C, H, W, lam, ws.ptr, p(go), grad.ptr, stream),
                 "scorp_loss_l1_ssim_backward")
    torch.cuda.synchronize()
    return ws, out, grad


@pytest.mark.parametrize("shape,kind", [((1, 1, 1), None), ((3, 24, 65), "levels"), ((1, 47, 133), None)])
def test_c_abi_calls_stay_inside_their_buffers_and_repeat_their_bits(shape, kind, dev):
    lam = 0.2
    x, y, mask, r = lossref.sweep_reference(shape, lam, kind)
    x, y, mask = x.to(dev), y.to(dev), None if mask is None else mask.to(dev)
    n = shape[0] * shape[1] * shape[2]
    ws, out, grad = _abi_call(x, y, mask, lam, dev)
    for c in (ws, out, grad):
        assert c.guards_intact()
    r.check(out.floats(), grad.floats().reshape(shape), f"C ABI {shape}")
    values, g = _fused(x, y, lam, mask, dev)                      # the wrapper makes the same two calls
    assert torch.equal(values, out.floats()) and torch.equal(g.reshape(-1), grad.floats())
    # a second identical call: the same bits everywhere (no atomics), the workspace included
    ws2, out2, grad2 = _abi_call(x, y, mask, lam, dev)
    assert torch.equal(ws2.whole, ws.whole) and torch.equal(out2.whole, out.whole) and torch.equal(grad2.whole, grad.whole)
    # grad_out = NULL is grad_out = 1.0
    ws3, out3, grad3 = _abi_call(x, y, mask, lam, dev, grad_out=1.0)
    assert torch.equal(grad3.whole, grad.whole) and grad3.guards_intact()
    # need_backward = 0: the derivative maps are not written, the values are the same bits
    ws4, out4, _ = _abi_call(x, y, mask, lam, dev, need_backward=0, backward=False)
    assert bool((ws4.region()[:12 * n] == _SENTINEL).all())
    assert not bool((ws.region()[:12 * n] == _SENTINEL).all())
    assert torch.equal(out4.whole, out.whole) and ws4.guards_intact() and out4.guards_intact()


# shape 1x69x192: strip rows at 0, 23, 46, strip columns at 0, 64, 128; the middle strip's support (its rows and columns
# +- 5) is rows 18 .. 50, columns 59 .. 132.  Then the seams of the backward's 32x32 tiles.
_EXIT_PIXELS = ([(r, 96) for r in (17, 18, 50, 51)] + [(34, c) for c in (58, 59, 132, 133)]
                + [(18, 59), (50, 132), (17, 58), (51, 133)] + [(31, 31), (32, 32), (31, 32)])


@pytest.mark.parametrize("pixel", _EXIT_PIXELS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_masked_early_exit_at_its_boundary(pixel, dev):
    """The mask's only live pixel (x = 1, y = 0 there) 5 and 6 pixels from a strip: a strip that answers from constants
    one pixel too eagerly has other derivative maps than the unmasked kernels on pre-multiplied inputs, which never take the
    exit: the three values and the gradient are theirs bit for bit, and the gradient is the float64 one."""
    shape, lam = (1, 69, 192), 1.0
    x, y, _ = lossref.make_case(shape, lossref.shape_seed(shape))
    x[0, pixel[0], pixel[1]], y[0, pixel[0], pixel[1]] = 1.0, 0.0
    mask = torch.zeros((1,) + shape[1:])
    mask[0, pixel[0], pixel[1]] = 1.0
    values, grad = _fused(x, y, lam, mask, dev)
    values_plain, grad_plain = _fused(x * mask, y * mask, lam, None, dev)
    assert torch.equal(values, values_plain)
    assert torch.equal(grad, grad_plain * mask.to(dev))
    assert grad[0, pixel[0], pixel[1]].item() != 0.0 and int((grad != 0).sum()) == 1
    lossref.Reference(x, y, lam, mask).check(values, grad, f"early exit, live pixel {pixel}", which=("grad",))


@pytest.mark.parametrize("masked", (False, True))
def test_more_partial_sums_than_one_trip_of_the_finalize_loop(masked, dev):
    """1 x 94209 x 1: 4097 strips of one column, one more than loss_finalize_kernel's 1024 threads x 4 loads take in one
    trip.  Masked: only rows 47000 .. 47100 live, every other strip answers from constants."""
    shape, lam = (1, 94209, 1), 0.2
    x, y, _ = lossref.make_case(shape, lossref.shape_seed(shape))
    mask = None
    if masked:
        mask = torch.zeros(shape)
        mask[0, 47000:47101, 0] = 1.0
    values, grad = _fused(x, y, lam, mask, dev)
    lossref.Reference(x, y, lam, mask).check(values, grad, f"4097 partials {'masked' if masked else 'plain'}")


def test_mask_and_image_forms_the_wrapper_accepts(dev):
    """A mask as [H, W], [1, H, W] or bool, and a non-contiguous image: the bits of the plain call."""
    shape, lam = (3, 29, 70), 0.2
    x, y, mask = lossref.make_case(shape, lossref.shape_seed(shape), "levels")
    values, grad = _fused(x, y, lam, mask, dev)
    v2, g2 = _fused(x, y, lam, mask[0], dev)
    assert torch.equal(v2, values) and torch.equal(g2, grad)
    binary = mask > 0.3
    vb, gb = _fused(x, y, lam, binary.float(), dev)
    for form in (binary, binary[0]):
        v3, g3 = _fused(x, y, lam, form, dev)
        assert form.dtype == torch.bool and torch.equal(v3, vb) and torch.equal(g3, gb)
    xt = x.to(dev).transpose(1, 2).contiguous().transpose(1, 2)  # the same numbers, strides (H W, 1, H)
    assert not xt.is_contiguous() and torch.equal(xt.cpu(), x)
    v4, g4 = _fused(xt, y, lam, mask, dev)
    assert torch.equal(v4, values) and torch.equal(g4, grad)
