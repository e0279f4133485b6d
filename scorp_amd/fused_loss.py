"""Fused L1 + SSIM training loss on the HIP library (scorp_amd/csrc/loss.hip).

`fused_l1_ssim_loss(image, gt, lambda_dssim, mask)` equals
`(1-lambda) * l1_loss(image*mask, gt*mask) + lambda * (1 - ssim(image*mask, gt*mask))` of scorp_amd.loss /
gs3dgs/utils/loss_utils.py, differentiable w.r.t. `image`, in two kernels instead of ~10 convolutions.

`fused_depth_terms(depth_raw, alpha, sensor, est, lambda_depth_sensor, weight_depth_est)` equals
`loss.depth_losses(nan_to_num(depth_raw / alpha, 0, 0), ...)` of train_3dgs.py:109-134 - the sensor-depth L1 and the min-max
normalised L1 against an estimated depth - differentiable w.r.t. the rasterizer's two raw maps, without the boolean-mask
indexings (and their host synchronisations) of the torch formulation (scorp_amd/csrc/depth_terms.hip).

`fused_surfel_terms(allmap, viewpoint_camera, depth_ratio, ...)` is the 2DGS form (train_2dgs.py:100-134): the same two depth
terms on the surface depth of the rasterizer's allmap plus the two depth-normal terms against the normal of the estimated
depth, differentiable w.r.t. allmap (scorp_amd/csrc/surfel_terms.hip).
"""
import ctypes

import torch

from . import _C


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(_C.current_stream_ptr())


class _FusedL1SSIM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, gt, lambda_dssim, mask):
        L = _C.lib()
        if not image.is_cuda:
            raise RuntimeError("fused_l1_ssim_loss needs GPU tensors (scorp_amd has no CPU path)")
        image = image.contiguous().float()
        gt = gt.contiguous().float()
        if mask is not None:
            mask = mask.expand(1, *image.shape[-2:]).contiguous().float()
        C, H, W = image.shape
        ws_bytes = L.scorp_loss_workspace_bytes(C, H, W)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=image.device)
        out = torch.empty(3, dtype=torch.float32, device=image.device)
        need_bwd = 1 if ctx.needs_input_grad[0] else 0
        _C.check(L.scorp_loss_l1_ssim_forward(_p(image), _p(gt), _p(mask), C, H, W, float(lambda_dssim), _p(out), _p(ws),
                                              ws_bytes, need_bwd, _stream()), "scorp_loss_l1_ssim_forward")
        ctx.lambda_dssim = float(lambda_dssim)
        ctx.has_mask = mask is not None
        ctx.save_for_backward(image, gt, mask if mask is not None else torch.empty(0, device=image.device), ws)
        ctx.parts = out
        return out[0]      # a view of the three-float result: no copy kernel

    @staticmethod
    def backward(ctx, grad_out):
        L = _C.lib()
        image, gt, mask, ws = ctx.saved_tensors
        mask = mask if ctx.has_mask else None
        C, H, W = image.shape
        grad = torch.empty_like(image)
        go = grad_out.contiguous().float().reshape(1)
        _C.check(L.scorp_loss_l1_ssim_backward(_p(image), _p(gt), _p(mask), C, H, W, ctx.lambda_dssim, _p(ws), _p(go),
                                               _p(grad), _stream()), "scorp_loss_l1_ssim_backward")
        return grad, None, None, None


def fused_l1_ssim_loss(image, gt, lambda_dssim=0.2, mask=None):
    return _FusedL1SSIM.apply(image, gt, lambda_dssim, mask)


def depth_terms(depth_raw, alpha, sensor=None, est=None, lambda_depth_sensor=0.0, weight_depth_est=0.0):
    """scorp_gs3d_depth_terms, no autograd: (out4, g_depth_raw, g_alpha) with out4 = {weighted sum, sensor term, estimate
    term, 0} on the device and the two gradient maps (upstream gradient 1) shaped like their inputs."""
    L = _C.lib()
    if not depth_raw.is_cuda:
        raise RuntimeError("depth_terms needs GPU tensors (scorp_amd has no CPU path)")
    H, W = depth_raw.shape[-2:]
    prep = lambda t: None if t is None else t.detach().contiguous().float()
    d, a, s_, e = prep(depth_raw), prep(alpha), prep(sensor), prep(est)
    for t in (d, a, s_, e):
        if t is not None and t.numel() != H * W:
            raise ValueError(f"depth_terms: maps of {H} x {W} expected, got {tuple(t.shape)}")
    ws_bytes = L.scorp_gs3d_view_terms_workspace_bytes(W, H, 0)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=d.device)
    out = torch.empty(4, dtype=torch.float32, device=d.device)
    g_depth, g_alpha = torch.empty_like(d), torch.empty_like(a)
    _C.check(L.scorp_gs3d_depth_terms(W, H, _p(d), _p(a), _p(s_), _p(e), float(lambda_depth_sensor), float(weight_depth_est),
                                      _p(out), _p(g_depth), _p(g_alpha), _p(ws), ws_bytes, _stream()), "scorp_gs3d_depth_terms")
    return out, g_depth, g_alpha


class _FusedDepthTerms(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth_raw, alpha, sensor, est, lambda_depth_sensor, weight_depth_est):
        out, g_depth, g_alpha = depth_terms(depth_raw, alpha, sensor, est, lambda_depth_sensor, weight_depth_est)
        ctx.save_for_backward(g_depth, g_alpha)
        ctx.parts = out      # {weighted sum, sensor term, estimate term, 0}
        return out[0]

    @staticmethod
    def backward(ctx, grad_out):
        g_depth, g_alpha = ctx.saved_tensors
        return (g_depth * grad_out if ctx.needs_input_grad[0] else None,
                g_alpha * grad_out if ctx.needs_input_grad[1] else None, None, None, None, None)


def fused_depth_terms(depth_raw, alpha, sensor=None, est=None, lambda_depth_sensor=0.0, weight_depth_est=0.0):
    """lambda_depth_sensor * Ls + weight_depth_est * Le on the rasterizer's raw depth and alpha maps (see the module
    docstring; weight_depth_est = 10 * dn_l1_weight(iteration)).  A term whose mask is empty or whose range is zero reads NaN
    and has a zero gradient (include/scorp_gs.h, ScorpGs3dViewTerms)."""
    return _FusedDepthTerms.apply(depth_raw, alpha, sensor, est, lambda_depth_sensor, weight_depth_est)


def surfel_terms(allmap, viewpoint_camera, depth_ratio, sensor=None, est=None, lambda_depth_sensor=0.0, weight_depth_est=0.0,
                 weight_depth_normal=0.0):
    """scorp_gs2d_surfel_terms, no autograd: (out6, g_allmap, surf_depth) with out6 = {weighted sum, sensor term, estimate
    term, depth-normal term, render-normal term, 0} on the device, the gradient with respect to allmap [7,H,W] for an upstream
    gradient of 1, and the surface depth [1,H,W] the terms were taken on."""
    from .renderer2d import _camera_rays
    L = _C.lib()
    if not allmap.is_cuda:
        raise RuntimeError("surfel_terms needs GPU tensors (scorp_amd has no CPU path)")
    H, W = allmap.shape[-2:]
    prep = lambda t: None if t is None else t.detach().contiguous().float()
    am, s_, e = prep(allmap), prep(sensor), prep(est)
    if am.numel() != 7 * H * W:
        raise ValueError(f"surfel_terms: allmap of [7, {H}, {W}] expected, got {tuple(allmap.shape)}")
    for t in (s_, e):
        if t is not None and t.numel() != H * W:
            raise ValueError(f"surfel_terms: maps of {H} x {W} expected, got {tuple(t.shape)}")
    rays_d, rays_o = _camera_rays(viewpoint_camera, am.device)
    view = viewpoint_camera.world_view_transform.contiguous().float()
    ws_bytes = L.scorp_gs2d_view_terms_workspace_bytes(W, H, 0)
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=am.device)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=am.device)
    out, depth, g_depth, g_allmap = new(6), new(1, H, W), new(H, W), new(7, H, W)
    g_normal = new(3, H, W) if weight_depth_normal else None
    _C.check(L.scorp_gs2d_surfel_terms(W, H, _p(am), _p(view), _p(rays_d), _p(rays_o), float(depth_ratio), _p(s_), _p(e),
                                       float(lambda_depth_sensor), float(weight_depth_est), float(weight_depth_normal), _p(out),
                                       _p(depth), _p(g_depth), _p(g_normal), _p(g_allmap), _p(ws), ws_bytes, _stream()),
             "scorp_gs2d_surfel_terms")
    return out, g_allmap, depth


class _FusedSurfelTerms(torch.autograd.Function):
    @staticmethod
    def forward(ctx, allmap, camera, depth_ratio, sensor, est, lambda_depth_sensor, weight_depth_est, weight_depth_normal):
        out, g_allmap, _ = surfel_terms(allmap, camera, depth_ratio, sensor, est, lambda_depth_sensor, weight_depth_est,
                                        weight_depth_normal)
        ctx.save_for_backward(g_allmap)
        ctx.shape = allmap.shape
        ctx.parts = out      # {weighted sum, sensor, estimate, depth-normal, render-normal, 0}
        return out[0]

    @staticmethod
    def backward(ctx, grad_out):
        (g_allmap,) = ctx.saved_tensors
        return ((g_allmap * grad_out).view(ctx.shape) if ctx.needs_input_grad[0] else None,) + (None,) * 7


def fused_surfel_terms(allmap, viewpoint_camera, depth_ratio, sensor=None, est=None, lambda_depth_sensor=0.0,
                       weight_depth_est=0.0, weight_depth_normal=0.0):
    """lambda_depth_sensor * Ls + weight_depth_est * Le + weight_depth_normal * (Ldn + Lrn) on the 2DGS rasterizer's allmap
    (see the module docstring; weight_depth_est = 10 * dn_l1_weight(iteration), weight_depth_normal = dn_l1_weight(iteration)
    after depth_from_iter + 1000).  A depth term whose mask is empty or whose range is zero reads NaN and has a zero gradient
    (include/scorp_gs.h, ScorpGs2dViewTerms)."""
    return _FusedSurfelTerms.apply(allmap, viewpoint_camera, depth_ratio, sensor, est, lambda_depth_sensor, weight_depth_est,
                                   weight_depth_normal)
