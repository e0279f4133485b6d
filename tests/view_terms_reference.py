"""float64 torch yardstick for the loss terms of the late iterations (train_3dgs.py:109-150): the sensor-depth L1
(:112-120), the min-max-normalised L1 against an estimated depth (:125-134 over image_utils.py:87-91) and the isotropic
regulariser (:146-148 over loss_utils.py:75-85), each as the reference's own torch expressions under float64 autograd and
as the closed forms include/scorp_gs.h states (ScorpGs3dViewTerms).  Not a test module: tests/test_view_terms_*.py import it.

Every mask decision is taken on the float32 tensors, as the reference takes it (`r` is the float32 depth render() returns);
the arithmetic after the masks is float64.
"""
import torch


def rendered_depth(depth_raw, alpha):
    """What render() returns for the depth (gaussian_renderer/__init__.py:113-120), in the dtype given."""
    return torch.nan_to_num(depth_raw / alpha, 0, 0)


def masks(r, sensor, est):
    ms = None if sensor is None else (sensor > 0.3) & (sensor < 7) & (r > 0.0)
    me = None if est is None else (r > 0.0) & (est > 0.0)
    return ms, me


def _normalize(x):     # image_utils.py:87-91
    lo, hi = torch.min(x).detach(), torch.max(x).detach()
    return (x - lo) / (hi - lo)


def depth_terms_autograd(r, sensor, est, w_s, w_e):
    """The two terms as train_3dgs.py writes them, on float64 copies of the float32 maps; the gradient with respect to r by
    autograd.  Returns {"Ls", "Le", "total", "g_r", "Ms", "Me"} (a term without its map: value 0, mask None)."""
    r64 = r.detach().double().requires_grad_(True)
    ms, me = masks(r, sensor, est)
    zero = torch.zeros((), dtype=torch.float64, device=r.device)
    ls = le = zero
    if sensor is not None:
        ls = torch.abs(r64[ms] - sensor.double()[ms]).mean()
    if est is not None:
        le = torch.abs(_normalize(r64[me]) - _normalize(est.double()[me])).mean()
    total = w_s * ls + w_e * le
    g_r = torch.autograd.grad(total, r64)[0] if total.requires_grad else torch.zeros_like(r64)
    return {"Ls": ls.detach(), "Le": le.detach(), "total": total.detach(), "g_r": g_r, "Ms": ms, "Me": me}


def depth_gradient_closed_form(r, sensor, est, w_s, w_e):
    """g = w_s sign(r - sensor) / cs [Ms] + w_e sign(rn - pn) / ((rmax - rmin) ce) [Me], float64."""
    r64 = r.detach().double()
    ms, me = masks(r, sensor, est)
    g = torch.zeros_like(r64)
    if sensor is not None:
        g = g + w_s * torch.sign(r64 - sensor.double()) / ms.sum() * ms
    if est is not None:
        e64 = est.double()
        rmin, rmax, pmin, pmax = r64[me].min(), r64[me].max(), e64[me].min(), e64[me].max()
        diff = (r64 - rmin) / (rmax - rmin) - (e64 - pmin) / (pmax - pmin)
        g = g + w_e * torch.sign(diff) / ((rmax - rmin) * me.sum()) * me
    return g


def tail_gradients(g_r, depth_raw, alpha):
    """Through r = nan_to_num(depth_raw / alpha): g_depth_raw = g / alpha, g_alpha = -g depth_raw / alpha^2, zeros where the
    quotient is not finite (what scorp_gs3d_render_tail_backward writes), float64."""
    d, a = depth_raw.detach().double(), alpha.detach().double()
    q = depth_raw / alpha
    ok = (alpha != 0) & torch.isfinite(q)
    safe = torch.where(ok, a, torch.ones_like(a))
    zero = torch.zeros_like(a)
    return torch.where(ok, g_r / safe, zero), torch.where(ok, -g_r * d / (safe * safe), zero)


def isotropic_autograd(raw_scaling, lam):
    """lam * mean |s - mean_axis s|, s = exp(raw) formed in float32 as the model forms it (gaussian_model.py get_scaling), then
    float64: the value and its gradient with respect to s by autograd, times ds/draw = s.  Returns (unweighted value, gradient)."""
    s = torch.exp(raw_scaling.detach().float()).double().requires_grad_(True)
    value = torch.abs(s - s.mean(dim=1, keepdim=True)).mean()
    (g_s,) = torch.autograd.grad(lam * value, s)
    return value.detach(), (g_s * s).detach()


def isotropic_gradient_closed_form(raw_scaling, lam):
    """lam / (3 N) * (sgn_j - (sgn_0 + sgn_1 + sgn_2) / 3) * s_j, sgn = sign(s - mean s), float64."""
    s = torch.exp(raw_scaling.detach().float()).double()
    sgn = torch.sign(s - s.mean(dim=1, keepdim=True))
    return lam / (3 * s.shape[0]) * (sgn - sgn.sum(dim=1, keepdim=True) / 3) * s
