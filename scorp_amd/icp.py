"""Multi-start ICP on the GPU, point-to-point, point-to-plane, generalized or coloured: the alignment scripts'
get_ICP_fitting_transformation_best (align_3dgs_clpe_9dof.py:42-115, align_2dgs_clpe_9dof.py:48-121) without Open3D.

The reference runs Open3D's registration_icp (TransformationEstimationPointToPoint, no scaling, max_iteration=400) once
per initial pose, 67 poses by default.  Here every init runs in one batch through scorp_icp_point_to_point
(csrc/icp.hip): one launch per iteration covers all inits still running.  estimation="point_to_plane" runs the same
batch through scorp_icp_point_to_plane (the same file, the other estimator) on the target's normals:
model_normals(gaussians) for a trained model, estimate_normals(points) for a bare cloud.  estimation="generalized" runs
it through scorp_icp_generalized on a covariance per point of both clouds (Segal et al. 2009; the estimator for two
independent samplings of one surface): model_covariances(gaussians) for a trained model, estimate_covariances(points) for
a bare cloud.  estimation="colored" runs it through scorp_icp_colored (Park, Zhou, Koltun 2017; the estimator for surfaces
that slide or spin at no geometric cost and carry a texture) on an intensity per point of both clouds and the target's
normals and colour gradients: model_colors(gaussians) for a trained model, estimate_color_gradients(points, colors) for the
gradients.  Swap it in with one import:

    from scorp_amd.icp import get_ICP_fitting_transformation_best
"""
from dataclasses import dataclass

import numpy as np
import torch

from . import _C
from ._points import _check_finite, _check_shape, _device, _points


@dataclass
class ICPResult:
    """Per init: the final transform [n_init, 4, 4] float64, its fitness and inlier_rmse, and the updates made."""
    transformation: np.ndarray
    fitness: np.ndarray
    inlier_rmse: np.ndarray
    iterations: np.ndarray


ESTIMATIONS = ("point_to_point", "point_to_plane", "generalized", "colored")


def _check_estimation(estimation):
    if estimation not in ESTIMATIONS:
        raise ValueError(f"unknown estimation {estimation!r}: expected one of {list(ESTIMATIONS)}")


def estimate_normals(points, knn=30, return_neighbors=False):
    """Unit normals [n, 3] fp32 (a device tensor) of a cloud that brings none, such as 3DGS centres: per point the
    eigenvector of the smallest eigenvalue of the float64 covariance of its min(knn, n) exact nearest neighbours (itself
    included), signed so that its largest component is positive (scorp_estimate_normals).  With return_neighbors also
    the neighbour indices [n, knn] int32, sorted by (d^2, index) and padded with -1."""
    if not 3 <= int(knn) <= 32:
        raise ValueError(f"knn must be in [3, 32]; got {knn}")
    _check_shape("points", points)
    _check_finite("points", points)
    dev = _device(points)
    P = _points("points", points, dev)
    n, knn = P.shape[0], int(knn)
    normals = torch.empty(n, 3, dtype=torch.float32, device=dev)
    nb = torch.empty(n, knn, dtype=torch.int32, device=dev) if return_neighbors else None
    _C.call_with_workspace("scorp_estimate_normals", "scorp_estimate_normals_workspace_bytes", (n,), P, n, knn, normals, nb)
    return (normals, nb) if return_neighbors else normals


def model_normals(gaussians):
    """Per-Gaussian normals [N, 3] of a trained model, for target_normals: a GaussianModel2D's surfel normal is the third
    axis of its rotation; a GaussianModel's is the rotation axis of its smallest scale.  Plain torch, once per object."""
    from .gaussian_model import build_rotation
    from .rasterizer3d import _GS2D
    from .segment import _model_kind
    kind = _model_kind(gaussians)
    with torch.no_grad():
        R = build_rotation(gaussians._rotation)
        if kind is _GS2D:
            return R[:, :, 2].contiguous()
        axis = gaussians._scaling.argmin(dim=1)       # (the activation is monotonic: the smallest raw scale)
        return torch.gather(R, 2, axis[:, None, None].expand(-1, 3, 1))[:, :, 0].contiguous()


_TRIU = ([0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2])   # (row, column) of the six packed values


def covariances_from_normals(normals, epsilon=1e-3):
    """Covariances [n, 6] fp32 (xx, xy, xz, yy, yz, zz) from normals [n, 3], Open3D's rule for generalized ICP: unit
    variance in the tangent plane and `epsilon` along the normal, I - (1 - epsilon) n n^T, computed in float64 and then
    rounded.  The normals are used as given; a zero normal gives I.  Plain torch, on the normals' device."""
    n = normals if isinstance(normals, torch.Tensor) else torch.as_tensor(np.array(normals))
    if n.ndim != 2 or n.shape[1] != 3:
        raise ValueError(f"normals must be [n, 3]; got {tuple(n.shape)}")
    n = n.to(torch.float64)
    f = 1.0 - float(epsilon)
    ia, ib = _TRIU
    C = -f * n[:, ia] * n[:, ib]
    C[:, [0, 3, 5]] += 1.0
    return C.to(torch.float32).contiguous()


def estimate_covariances(points, knn=30, epsilon=1e-3):
    """covariances_from_normals(estimate_normals(points, knn), epsilon): the covariances of a bare cloud, [n, 6] fp32 on
    the device."""
    return covariances_from_normals(estimate_normals(points, knn=knn), epsilon)


def model_covariances(gaussians, mode="plane", epsilon=1e-3):
    """Per-Gaussian covariances [N, 6] fp32 of a trained model, for source_covariances / target_covariances.
    mode="plane": covariances_from_normals(model_normals(gaussians), epsilon).  mode="full": the Gaussian's own
    R diag(sigma^2) R^T of its activated scales; a surfel's missing third variance, and any variance below epsilon times
    that Gaussian's largest, is raised to epsilon times the largest, so that no covariance has a condition number above
    1 / epsilon.  Plain torch, once per object."""
    if mode not in ("plane", "full"):
        raise ValueError(f"unknown mode {mode!r}: expected 'plane' or 'full'")
    if mode == "plane":
        return covariances_from_normals(model_normals(gaussians), epsilon)
    from .gaussian_model import build_rotation
    with torch.no_grad():
        R = build_rotation(gaussians._rotation).to(torch.float64)
        var = gaussians.get_scaling.to(torch.float64) ** 2
        if var.shape[1] == 2:
            var = torch.cat([var, torch.zeros_like(var[:, :1])], dim=1)
        var = torch.maximum(var, float(epsilon) * var.max(dim=1, keepdim=True).values)
        C = (R * var[:, None, :]) @ R.transpose(1, 2)
        ia, ib = _TRIU
        return (0.5 * (C[:, ia, ib] + C[:, ib, ia])).to(torch.float32).contiguous()


def intensities(colors):
    """The intensity [n] fp32 (a device tensor) of colours [n, 3] (the mean of the channels) or [n] (passed through),
    numpy or torch."""
    t = colors if isinstance(colors, torch.Tensor) else torch.as_tensor(np.array(colors))
    if not (t.ndim == 1 or (t.ndim == 2 and t.shape[1] == 3)):
        raise ValueError(f"colors must be [n, 3] or [n]; got {tuple(t.shape)}")
    _check_finite("colors", t)
    dev = t.device if t.is_cuda else _device(t)
    if t.ndim == 2:
        t = t.to(torch.float64).mean(dim=1)
    return t.to(device=dev, dtype=torch.float32).contiguous()


def _intensity(name, a, n, device):
    """A colour argument, [n, 3] or [n] (numpy or torch), as the intensity [n] fp32 on the device."""
    shape = tuple(np.shape(a))
    if shape not in ((n, 3), (n,)):
        raise ValueError(f"{name} must be [{n}, 3] or [{n}]; got {shape}")
    try:
        return intensities(a).to(device)
    except ValueError as e:
        raise ValueError(str(e).replace("colors", name, 1)) from None


def color_gradients(points, normals, intensity, neighbors):
    """scorp_color_gradients on device tensors: gradients [n, 3] fp32 of the intensity [n] over the stored neighbour lists
    [n, knn] int32 (estimate_normals' layout), in the tangent planes of `normals`."""
    n, knn = neighbors.shape
    if tuple(points.shape) != (n, 3) or tuple(normals.shape) != (n, 3) or tuple(intensity.shape) != (n,):
        raise ValueError(f"points and normals must be [{n}, 3] and intensity [{n}]; got {tuple(points.shape)}, "
                         f"{tuple(normals.shape)}, {tuple(intensity.shape)}")
    if bool((neighbors >= n).any()):
        raise ValueError(f"neighbors holds an index >= {n}")
    out = torch.empty(n, 3, dtype=torch.float32, device=points.device)
    with torch.cuda.device(points.device):
        _C.call("scorp_color_gradients", points, normals, intensity, neighbors, n, knn, out)
    return out


def estimate_color_gradients(points, colors, normals=None, knn=30):
    """Colour gradients [n, 3] fp32 (a device tensor) of a cloud, for target_gradients: per point the least-squares gradient
    of intensities(colors) over the neighbour list of estimate_normals(points, knn, return_neighbors=True), kept in the
    tangent plane of its normal (scorp_color_gradients; the rule is in include/scorp_gs.h).  normals [n, 3]: the cloud's
    own, when it brings them; None takes the estimated ones."""
    est, nb = estimate_normals(points, knn=knn, return_neighbors=True)
    dev = est.device
    P = _points("points", points, dev)
    if normals is not None:
        if tuple(np.shape(normals)) != tuple(P.shape):
            raise ValueError(f"normals must have the points' shape {tuple(P.shape)}; got {tuple(np.shape(normals))}")
        _check_finite("normals", normals)
        est = _points("normals", normals, dev)
    return color_gradients(P, est, _intensity("colors", colors, P.shape[0], dev), nb)


def model_colors(gaussians):
    """Per-Gaussian colours [N, 3] of a trained model (either kind), for source_colors / target_colors: the view-independent
    part of its spherical harmonics, clamp(0.5 + C0 * _features_dc[:, 0, :], 0, 1).  Plain torch, once per object."""
    from .sh import C0
    with torch.no_grad():
        return (0.5 + C0 * gaussians._features_dc[:, 0, :]).clamp(0.0, 1.0).contiguous()


def _covariances(name, a, n, device):
    """A covariance argument, [n, 6] or [n, 3, 3] (numpy or torch), as [n, 6] fp32 on the device."""
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.array(a))
    shape = tuple(t.shape)
    if shape not in ((n, 6), (n, 3, 3)):
        raise ValueError(f"{name} must be [{n}, 6] or [{n}, 3, 3]; got {shape}")
    _check_finite(name, t)
    if t.ndim == 3:
        big = t.abs().amax(dim=(1, 2))
        if bool(((t - t.transpose(1, 2)).abs().amax(dim=(1, 2)) > 1e-6 * big).any()):
            raise ValueError(f"{name} holds a 3x3 that is not symmetric")
        ia, ib = _TRIU
        t = t[:, ia, ib]
    return t.to(device=device, dtype=torch.float32).contiguous()


def registration_icp(source, target, max_correspondence_distance, inits, max_iteration=30, relative_fitness=1e-6,
                     relative_rmse=1e-6, estimation="point_to_point", target_normals=None, source_covariances=None,
                     target_covariances=None, source_colors=None, target_colors=None, target_gradients=None,
                     lambda_geometric=0.968):
    """Open3D's registration_icp(source, target, r, init, TransformationEstimationPointToPoint(),
    ICPConvergenceCriteria(relative_fitness, relative_rmse, max_iteration)) from every init of `inits` ([4, 4] or
    [n_init, 4, 4]) at once.  source [n, 3] and target [m, 3]: numpy arrays or torch tensors (searched in fp32; pair
    distances, moments and transforms in float64).  estimation="point_to_plane" is TransformationEstimationPointToPlane
    (no robust kernel) on target_normals [m, 3]; without them the normals are estimate_normals(target, knn=30).
    estimation="generalized" is generalized ICP (the rules of include/scorp_gs.h) on source_covariances and
    target_covariances, each [n, 6] (xx, xy, xz, yy, yz, zz) or [n, 3, 3]; one left out is estimate_covariances(cloud).
    estimation="colored" is coloured ICP (the rules of include/scorp_gs.h) on source_colors and target_colors ([n, 3] or
    intensities [n]; both required), target_normals and target_gradients [m, 3], weighing the geometric term by
    lambda_geometric and the colour term by 1 - lambda_geometric; normals left out are estimate_normals(target, knn=30),
    gradients left out estimate_color_gradients(target, target_colors, those normals).
    Returns an ICPResult of numpy arrays."""
    _check_estimation(estimation)
    r = float(max_correspondence_distance)
    if not np.isfinite(r) or r <= 0.0:
        raise ValueError(f"max_correspondence_distance must be positive and finite; got {max_correspondence_distance}")
    if int(max_iteration) < 0:
        raise ValueError(f"max_iteration must be >= 0; got {max_iteration}")
    _check_finite("source", source)
    _check_finite("target", target)
    plane = estimation == "point_to_plane"
    gicp = estimation == "generalized"
    colored = estimation == "colored"
    if colored:
        if source_colors is None or target_colors is None:
            raise ValueError("estimation='colored' needs source_colors and target_colors")
        lam = float(lambda_geometric)
        if not 0.0 <= lam <= 1.0:
            raise ValueError(f"lambda_geometric must be in [0, 1]; got {lambda_geometric}")
        if target_gradients is not None:
            if tuple(np.shape(target_gradients)) != tuple(np.shape(target)):
                raise ValueError(f"target_gradients must have the target's shape {tuple(np.shape(target))}; "
                                 f"got {tuple(np.shape(target_gradients))}")
            _check_finite("target_gradients", target_gradients)
    if (plane or colored) and target_normals is not None:
        if tuple(np.shape(target_normals)) != tuple(np.shape(target)):
            raise ValueError(f"target_normals must have the target's shape {tuple(np.shape(target))}; "
                             f"got {tuple(np.shape(target_normals))}")
        _check_finite("target_normals", target_normals)
    T0 = np.asarray(inits.detach().cpu() if isinstance(inits, torch.Tensor) else inits, dtype=np.float64)
    if T0.shape == (4, 4):
        T0 = T0[None]
    if T0.ndim != 3 or T0.shape[1:] != (4, 4) or not 1 <= T0.shape[0] <= 65535:
        raise ValueError(f"inits must be [4, 4] or [n_init, 4, 4] with 1 <= n_init <= 65535; got {T0.shape}")
    _check_finite("inits", T0)
    dev = _device(source, target)
    P = _points("source", source, dev)
    Q = _points("target", target, dev)
    ni = T0.shape[0]
    if plane:
        Nq = estimate_normals(Q, knn=30) if target_normals is None else _points("target_normals", target_normals, dev)
    if colored:
        Ip = _intensity("source_colors", source_colors, P.shape[0], dev)
        Iq = _intensity("target_colors", target_colors, Q.shape[0], dev)
        nb = None
        if target_normals is None:
            Nq, nb = estimate_normals(Q, knn=30, return_neighbors=True)
        else:
            Nq = _points("target_normals", target_normals, dev)
        if target_gradients is None:
            if nb is None:
                nb = estimate_normals(Q, knn=30, return_neighbors=True)[1]
            Gq = color_gradients(Q, Nq, Iq, nb)
        else:
            Gq = _points("target_gradients", target_gradients, dev)
    if gicp:
        Cp = (estimate_covariances(P) if source_covariances is None
              else _covariances("source_covariances", source_covariances, P.shape[0], dev))
        Cq = (estimate_covariances(Q) if target_covariances is None
              else _covariances("target_covariances", target_covariances, Q.shape[0], dev))
    T_in = torch.as_tensor(np.ascontiguousarray(T0), device=dev)
    T_out = torch.empty_like(T_in)
    fit = torch.empty(ni, dtype=torch.float64, device=dev)
    rmse = torch.empty(ni, dtype=torch.float64, device=dev)
    iters = torch.empty(ni, dtype=torch.int32, device=dev)
    if colored:
        _C.call_with_workspace("scorp_icp_colored", "scorp_icp_colored_workspace_bytes", (P.shape[0], Q.shape[0], ni),
                               P, Ip, P.shape[0], Q, Nq, Iq, Gq, Q.shape[0], T_in, ni, r, int(max_iteration),
                               float(relative_fitness), float(relative_rmse), lam, T_out, fit, rmse, iters)
        return ICPResult(T_out.cpu().numpy(), fit.cpu().numpy(), rmse.cpu().numpy(), iters.cpu().numpy())
    name, size_name = (("scorp_icp_generalized", "scorp_icp_generalized_workspace_bytes") if gicp
                       else ("scorp_icp_point_to_plane", "scorp_icp_point_to_plane_workspace_bytes") if plane
                       else ("scorp_icp_point_to_point", "scorp_icp_workspace_bytes"))
    _C.call_with_workspace(name, size_name, (P.shape[0], Q.shape[0], ni),
                           P, *((Cp,) if gicp else ()), P.shape[0], Q, *((Cq,) if gicp else (Nq,) if plane else ()), Q.shape[0],
                           T_in, ni, r, int(max_iteration), float(relative_fitness), float(relative_rmse), T_out, fit, rmse, iters)
    return ICPResult(T_out.cpu().numpy(), fit.cpu().numpy(), rmse.cpu().numpy(), iters.cpu().numpy())


def downsample_indices(num_original, num_refined):
    """The source indices the reference keeps: Open3D's uniform_down_sample(k) (indices 0, k, 2k, ...) with
    k = int(n_ref / (4 n_orig)) when n_ref > 4 n_orig, else every point."""
    if num_refined > 4 * num_original:
        k = int(num_refined / (4 * num_original))
        return np.arange(0, num_refined, k)
    return np.arange(num_refined)


def icp_inits(rotations, center_original, center_refined):
    """The reference's initial poses: [R | c_orig - R c_ref] per rotation, then the centroid translation twice (the
    reference lists it twice), then the identity."""
    rotations = np.asarray(rotations, dtype=np.float64)
    T = np.tile(np.eye(4), (len(rotations) + 3, 1, 1))
    for i, rot in enumerate(rotations):
        T[i, :3, :3] = rot
        T[i, :3, 3] = center_original - rot @ center_refined
    T[-3, :3, 3] = center_original - center_refined
    T[-2, :3, 3] = center_original - center_refined
    return T


def get_ICP_fitting_transformation_best(pc_xyz_original: np.ndarray, pc_xyz_refined: np.ndarray, rotations: np.ndarray,
                                        threshold: float, *, estimation="point_to_point", target_normals=None,
                                        max_iteration=400, source_covariances=None, target_covariances=None,
                                        source_colors=None, target_colors=None, target_gradients=None,
                                        lambda_geometric=0.968) -> np.ndarray:
    """The reference's function of the same name, statement for statement, with every ICP run on the GPU in one batch:
    the 4x4 float64 transform (refined -> original) of the FIRST init with the highest fitness.  The keyword-only
    arguments are this project's: estimation="point_to_plane" with target_normals [len(pc_xyz_original), 3] (a surfel
    model's come from model_normals; None estimates them from the cloud) normally needs far fewer updates;
    estimation="generalized" with source_covariances for pc_xyz_refined (subsampled here with its points) and
    target_covariances for pc_xyz_original (a trained model's come from model_covariances; None estimates them from the
    cloud that is registered) weighs every pair by both; estimation="colored" with source_colors for pc_xyz_refined
    (subsampled here with its points), target_colors for pc_xyz_original (a trained model's come from model_colors) and
    optionally target_gradients (None: estimate_color_gradients of the cloud that is registered) adds the colour term of
    coloured ICP at the weight 1 - lambda_geometric."""
    _check_estimation(estimation)
    if np.any(np.isnan(pc_xyz_original)) or np.any(np.isnan(pc_xyz_refined)):
        raise ValueError("Point clouds contain NaN values")
    if np.any(np.isinf(pc_xyz_original)) or np.any(np.isinf(pc_xyz_refined)):
        raise ValueError("Point clouds contain Inf values")
    orig = np.asarray(pc_xyz_original)
    ref = np.asarray(pc_xyz_refined)
    center_original = orig.mean(axis=0)   # get_centroid(., method="mean"), in the clouds' own dtype as there
    center_refined = ref.mean(axis=0)
    keep = downsample_indices(len(orig), len(ref))
    src = ref[keep]
    if estimation == "generalized" and source_covariances is not None:
        if len(source_covariances) != len(ref):
            raise ValueError(f"source_covariances must have one entry per point of pc_xyz_refined ({len(ref)}); "
                             f"got {len(source_covariances)}")
        source_covariances = source_covariances[keep]
    if estimation == "colored" and source_colors is not None:
        if len(source_colors) != len(ref):
            raise ValueError(f"source_colors must have one entry per point of pc_xyz_refined ({len(ref)}); "
                             f"got {len(source_colors)}")
        source_colors = source_colors[keep]
    inits = icp_inits(rotations, center_original, center_refined)
    res = registration_icp(src, orig, threshold, inits, max_iteration=max_iteration, estimation=estimation,
                           target_normals=target_normals, source_covariances=source_covariances,
                           target_covariances=target_covariances, source_colors=source_colors, target_colors=target_colors,
                           target_gradients=target_gradients, lambda_geometric=lambda_geometric)
    best = int(np.argmax(res.fitness))   # the first maximum: the reference keeps a pose only on a strictly higher fitness
    return res.transformation[best].copy()
