"""float64 torch yardstick for the loss terms of the late 2DGS iterations (train_2dgs.py:100-139) on the rasterizer's allmap:
the sensor-depth L1 (:101-109), the min-max-normalised L1 against an estimated depth (:114-124), the two depth-normal terms
against the normal of the estimated depth (:126-134 over point_utils.py:9-37) and the isotropic regulariser on [N,2] scales
(:136-139).  The five render maps are formed as oracle/surfel_maps_ref.py states them, under float64 autograd.  Not a test
module: tests/test_surfel_terms_*.py import it.

Every mask decision is taken on the float32 maps, as the reference takes it; the arithmetic after the masks is float64.
"""
import torch

from oracle.surfel_maps_ref import depth_to_normal, surfel_maps_ref


def masks(d, sensor, est):
    ms = None if sensor is None else (sensor > 0.3) & (sensor < 7) & (d > 0.0)
    me = None if est is None else (d > 0.0) & (est > 0.0)
    return ms, me


def _normalize(x):     # image_utils.py:87-91
    lo, hi = torch.min(x).detach(), torch.max(x).detach()
    return (x - lo) / (hi - lo)


def pred_normal(rays_d, rays_o, est):
    """depth_to_normal(camera, depth_est).permute(2, 0, 1), no gradient, in the dtype of the rays."""
    with torch.no_grad():
        return depth_to_normal(rays_d, rays_o, est.to(rays_d.dtype).reshape(1, *est.shape[-2:])).permute(2, 0, 1)


def terms_from_maps(d, rn, sn, rays_d64, rays_o64, sensor, est, w_s, w_e, w_n, ms, me):
    """The weighted total and the four unweighted values from the float64 render maps (surface depth, render_normal,
    surf_normal), given the masks."""
    zero = torch.zeros((), dtype=torch.float64, device=d.device)
    ls = le = ldn = lrn = zero
    if sensor is not None:
        ls = torch.abs(d[ms] - sensor.double().reshape(d.shape)[ms]).mean()
    if est is not None:
        le = torch.abs(_normalize(d[me]) - _normalize(est.double().reshape(d.shape)[me])).mean()
    if est is not None and w_n:
        pn = pred_normal(rays_d64, rays_o64, est)
        ldn = (1 - (sn * pn).sum(dim=0)).mean()
        lrn = (1 - (rn * pn).sum(dim=0)).mean()
    return w_s * ls + w_e * le + w_n * (ldn + lrn), ls, le, ldn, lrn


def terms_from_allmap(allmap64, view, rays_d, rays_o, depth_ratio, sensor, est, w_s, w_e, w_n, ms, me):
    """The same from a float64 allmap (differentiable): the maps as oracle/surfel_maps_ref.py forms them."""
    v64, rd64, ro64 = view.double(), rays_d.double(), rays_o.double()
    _, rn, _, d, sn = surfel_maps_ref(allmap64, v64, rd64, ro64, depth_ratio)
    return terms_from_maps(d, rn, sn, rd64, ro64, sensor, est, w_s, w_e, w_n, ms, me)


def surfel_terms_autograd(allmap, view, rays_d, rays_o, depth_ratio, sensor, est, w_s, w_e, w_n):
    """Values and the gradient with respect to allmap by float64 autograd.  Returns {"Ls", "Le", "Ldn", "Lrn", "total",
    "g_allmap", "Ms", "Me", "d"} (a term without its map: 0, mask None).  Autograd leaves 0 * inf = NaN where alpha == 0 (the
    quotient allmap[0] / alpha); nan_to_num passes no gradient there, so those entries are set to the zeros it stands for -
    any other NaN is kept and fails the caller."""
    d32 = surfel_maps_ref(allmap.detach().float(), view, rays_d, rays_o, depth_ratio)[3]
    ms, me = masks(d32, None if sensor is None else sensor.reshape(d32.shape), None if est is None else est.reshape(d32.shape))
    a64 = allmap.detach().double().requires_grad_(True)
    total, ls, le, ldn, lrn = terms_from_allmap(a64, view, rays_d, rays_o, depth_ratio, sensor, est, w_s, w_e, w_n, ms, me)
    g = torch.autograd.grad(total, a64)[0] if total.requires_grad else torch.zeros_like(a64)
    empty = (allmap[1] == 0).expand_as(g[:2])
    g[:2] = torch.where(empty & torch.isnan(g[:2]), torch.zeros_like(g[:2]), g[:2])
    return {"Ls": ls.detach(), "Le": le.detach(), "Ldn": ldn.detach(), "Lrn": lrn.detach(), "total": total.detach(), "g_allmap": g,
            "Ms": ms, "Me": me, "d": d32}


def isotropic2_autograd(raw_scaling, lam):
    """lam * mean |s - mean_axis s| over [N,2] scales, s = exp(raw) formed in float32 as the model forms it, then float64: the
    unweighted value and the gradient with respect to the raw scales (autograd through s, times ds/draw = s)."""
    s = torch.exp(raw_scaling.detach().float()).double().requires_grad_(True)
    value = torch.abs(s - s.mean(dim=1, keepdim=True)).mean()
    (g_s,) = torch.autograd.grad(lam * value, s)
    return value.detach(), (g_s * s).detach()


def isotropic2_gradient_closed_form(raw_scaling, lam):
    """lam / (2 N) * (sgn_j - (sgn_0 + sgn_1) / 2) * s_j, sgn = sign(s - mean s), float64."""
    s = torch.exp(raw_scaling.detach().float()).double()
    sgn = torch.sign(s - s.mean(dim=1, keepdim=True))
    return lam / (2 * s.shape[0]) * (sgn - sgn.sum(dim=1, keepdim=True) / 2) * s
