"""`diff_surfel_rasterization`-compatible front-end (2DGS) over libscorp_gs.so.

Same names / call signature as the module imported at gs2dgs/gaussian_renderer/__init__.py:14 and called at :51-67,
:111-120: `GaussianRasterizer(raster_settings)(means3D, means2D, shs, colors_precomp, opacities, scales[N,2],
rotations, cov3D_precomp[N,9]) -> (color[3,H,W], radii[N], allmap[7,H,W])`.
"""
import torch
import torch.nn as nn

from . import _C
from . import rasterizer3d as R3
# GaussianRasterizationSettings, LAST_NUM_PAIRS_LOG, PairPolicy: kept as names of this module (re-exported)
from .rasterizer3d import GaussianRasterizationSettings, LAST_NUM_PAIRS_LOG, PairPolicy, _prep, _ptr, _stream  # noqa: F401


def rasterize_surfels_raw(means3D, means2D, f_dc, f_rest, opacity_raw, scaling_raw, rotation_raw, raster_settings):
    """Raw-leaf variant (logit opacity, log scale[N,2], un-normalised quaternion, dc/rest split): see rasterizer3d."""
    R3._tls.grad_mode = torch.is_grad_enabled()
    return R3._RasterizeRaw.apply(means3D, means2D, f_dc, f_rest, opacity_raw, scaling_raw, rotation_raw, raster_settings,
                                  R3._GS2D)


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions):
        with torch.no_grad():
            vm = self.raster_settings.viewmatrix
            return (positions @ vm[:3, 2] + vm[3, 2]) > 0.2

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None):
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception("Please provide excatly one of either SHs or precomputed colors!")
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
        R3._tls.grad_mode = torch.is_grad_enabled()
        return R3._Rasterize.apply(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                   self.raster_settings, R3._GS2D)


class _SurfelMaps(torch.autograd.Function):
    """allmap -> (render_alpha, render_normal, render_dist, surf_depth, surf_normal): the per-pixel tail of
    gs2dgs/gaussian_renderer/__init__.py:131-160 as one HIP kernel each way (scorp_gs2d_maps_forward/backward)."""

    @staticmethod
    def forward(ctx, allmap, viewmatrix, rays_d, rays_o, depth_ratio):
        L = _C.lib()
        allmap = _prep(allmap, "allmap")
        _, H, W = allmap.shape
        dev = allmap.device
        out = torch.empty((9, H, W), dtype=torch.float32, device=dev)   # alpha | normal(3) | dist | depth | surf_normal(3)
        ra, rn, rd, sd, sn = out[0:1], out[1:4], out[4:5], out[5:6], out[6:9]
        _C.check(L.scorp_gs2d_maps_forward(W, H, _ptr(allmap), _ptr(viewmatrix), _ptr(rays_d), _ptr(rays_o),
                                           float(depth_ratio), _ptr(ra), _ptr(rn), _ptr(rd), _ptr(sd), _ptr(sn), _stream()),
                 "scorp_gs2d_maps_forward")
        ctx.save_for_backward(allmap, viewmatrix, rays_d, rays_o, sd)
        ctx.depth_ratio = float(depth_ratio)
        ctx.set_materialize_grads(False)
        return ra, rn, rd, sd, sn

    @staticmethod
    def backward(ctx, g_ra, g_rn, g_rd, g_sd, g_sn):
        L = _C.lib()
        allmap, viewmatrix, rays_d, rays_o, sd = ctx.saved_tensors
        _, H, W = allmap.shape
        gs = [None if g is None else _prep(g, "grad") for g in (g_ra, g_rn, g_rd, g_sd, g_sn)]
        g_allmap = torch.empty_like(allmap)
        _C.check(L.scorp_gs2d_maps_backward(W, H, _ptr(allmap), _ptr(viewmatrix), _ptr(rays_d), _ptr(rays_o), ctx.depth_ratio,
                                            _ptr(sd), _ptr(gs[0]), _ptr(gs[1]), _ptr(gs[2]), _ptr(gs[3]), _ptr(gs[4]),
                                            _ptr(g_allmap), _stream()), "scorp_gs2d_maps_backward")
        return g_allmap, None, None, None, None


def surfel_maps(allmap, viewmatrix, rays_d, rays_o, depth_ratio):
    """(render_alpha[1,H,W], render_normal[3,H,W], render_dist[1,H,W], surf_depth[1,H,W], surf_normal[3,H,W])."""
    if not allmap.is_cuda:
        raise RuntimeError("surfel_maps needs CUDA/HIP tensors: scorp_amd has no CPU fallback")
    return _SurfelMaps.apply(allmap, _prep(viewmatrix, "viewmatrix"), _prep(rays_d, "rays_d"), _prep(rays_o, "rays_o"),
                             depth_ratio)


class _SurfelRegularizers(torch.autograd.Function):
    """(normal_loss, dist_loss) of train_2dgs.py:142-150 straight from allmap: scorp_gs2d_regularizers_forward/backward."""

    @staticmethod
    def forward(ctx, allmap, viewmatrix, rays_d, rays_o, depth_ratio, lambda_normal, lambda_dist):
        L = _C.lib()
        allmap = _prep(allmap, "allmap")
        _, H, W = allmap.shape
        out = torch.empty(2, dtype=torch.float32, device=allmap.device)
        wb = L.scorp_gs2d_regularizers_workspace_bytes(W, H)
        ws = torch.empty(wb, dtype=torch.uint8, device=allmap.device)
        _C.check(L.scorp_gs2d_regularizers_forward(W, H, _ptr(allmap), _ptr(viewmatrix), _ptr(rays_d), _ptr(rays_o),
                                                   float(depth_ratio), float(lambda_normal), float(lambda_dist), _ptr(out),
                                                   _ptr(ws), wb, _stream()), "scorp_gs2d_regularizers_forward")
        ctx.save_for_backward(allmap, viewmatrix, rays_d, rays_o)
        ctx.consts = (float(depth_ratio), float(lambda_normal), float(lambda_dist))
        return out

    @staticmethod
    def backward(ctx, g_out):
        L = _C.lib()
        allmap, viewmatrix, rays_d, rays_o = ctx.saved_tensors
        _, H, W = allmap.shape
        g_out = _prep(g_out, "grad")
        g_allmap = torch.empty_like(allmap)
        dr, ln, ld = ctx.consts
        _C.check(L.scorp_gs2d_regularizers_backward(W, H, _ptr(allmap), _ptr(viewmatrix), _ptr(rays_d), _ptr(rays_o), dr, ln, ld,
                                                    _ptr(g_out), _ptr(g_allmap), _stream()), "scorp_gs2d_regularizers_backward")
        return g_allmap, None, None, None, None, None, None


def surfel_regularizer_losses(allmap, viewmatrix, rays_d, rays_o, depth_ratio, lambda_normal, lambda_dist):
    """tensor[2] = (lambda_normal * mean(1 - render_normal . surf_normal), lambda_dist * mean(render_dist))."""
    if not allmap.is_cuda:
        raise RuntimeError("surfel_regularizer_losses needs CUDA/HIP tensors: scorp_amd has no CPU fallback")
    return _SurfelRegularizers.apply(allmap, _prep(viewmatrix, "viewmatrix"), _prep(rays_d, "rays_d"), _prep(rays_o, "rays_o"),
                                     depth_ratio, lambda_normal, lambda_dist)
