"""Cleaning a point cloud on the GPU: statistical and radius outlier removal, DBSCAN, voxel-grid downsampling - what a
user of Open3D looks for next to registration_icp (remove_statistical_outlier, remove_radius_outlier, cluster_dbscan,
voxel_down_sample).  The alignment scripts size an object by the bounding box of ALL its Gaussian centres
(align_3dgs_clpe_9dof.py:377-382, align_2dgs_clpe_9dof.py likewise); one floater left by the mask vote or by
truncate_opacity.py moves the initial scale, the RANSAC threshold and the ICP radius at once.  Clean first:

    from scorp_amd import cloud, segment
    mask3d = cloud.clean_gaussians(gaussians, method="dbscan", eps=0.05, min_points=10)
    segment.apply_mask3d(gaussians, mask3d, "gs_seg/object_clean.ply")

The searches are csrc/cloud_filter.hip (scorp_cloud_*): exact, decided in float64 on the float32 coordinates, bit-
reproducible.  The rules R1 - R8 are in include/scorp_gs.h; they are this project's own.  Open3D was never run where
this was written: where a rule follows what Open3D is believed to do, that is believed, unchecked.  Every function takes a
numpy array or a torch tensor [n, 3] and returns device tensors.
"""
import numpy as np
import torch

from . import _C
from ._points import _at_least, _cloud, _positive

MAX_KNN = 32
METHODS = ("dbscan", "statistical", "radius")


def _call(name, P, *args):
    n = P.shape[0]
    _C.call_with_workspace(name, "scorp_cloud_workspace_bytes", (n,), P, n, *args)


def knn_mean_distance(points, nb_neighbors=20, return_neighbors=False):
    """Per point the mean distance [n] float64 to its k = min(nb_neighbors, n) nearest points, ITSELF INCLUDED (distance
    0), in ascending order of (d^2, index) (rule R3).  With return_neighbors also their indices [n, nb_neighbors] int32 in
    that order, padded with -1 when nb_neighbors > n."""
    knn = _at_least("nb_neighbors", nb_neighbors, 1)
    if knn > MAX_KNN:
        raise ValueError(f"nb_neighbors must be in [1, {MAX_KNN}]; got {knn}")
    P = _cloud(points)
    n = P.shape[0]
    mean = torch.empty(n, dtype=torch.float64, device=P.device)
    nb = torch.empty(n, knn, dtype=torch.int32, device=P.device) if return_neighbors else None
    _call("scorp_cloud_knn_distance", P, knn, mean, nb)
    return (mean, nb) if return_neighbors else mean


def radius_neighbor_count(points, radius):
    """Per point the number [n] int32 of points within `radius` of it, inclusive, ITSELF INCLUDED (rule R2)."""
    r = _positive("radius", radius)
    P = _cloud(points)
    count = torch.empty(P.shape[0], dtype=torch.int32, device=P.device)
    _call("scorp_cloud_radius_count", P, r, count)
    return count


def _select(points, keep):
    ind = keep.nonzero().reshape(-1)   # int64, ascending
    P = points if isinstance(points, torch.Tensor) else torch.as_tensor(np.asarray(points))
    return P.to(keep.device)[ind], ind


def remove_statistical_outlier(points, nb_neighbors=20, std_ratio=2.0):
    """(points[ind], ind): the points whose k-nearest mean distance m_i (knn_mean_distance) is at most mu + std_ratio sd,
    mu = sum(m) / n and sd = sqrt(sum((m - mu)^2) / (n - 1)) (0 for n = 1) in float64 on the device; ind int64, ascending.
    Open3D's remove_statistical_outlier is believed (unchecked) to keep m_i < threshold instead and to drop points whose
    mean is 0; here the bound is inclusive and a mean of 0 is an ordinary value, so a cloud of identical points is kept."""
    std_ratio = float(std_ratio)
    if not np.isfinite(std_ratio):
        raise ValueError(f"std_ratio must be finite; got {std_ratio}")
    m = knn_mean_distance(points, nb_neighbors)
    n = m.shape[0]
    mu = m.sum() / n
    sd = torch.sqrt(((m - mu) ** 2).sum() / (n - 1)) if n > 1 else torch.zeros((), dtype=torch.float64, device=m.device)
    return _select(points, m <= mu + std_ratio * sd)


def remove_radius_outlier(points, nb_points, radius):
    """(points[ind], ind): the points with MORE than nb_points points within `radius`, the point itself counted (believed,
    unchecked, to be Open3D's rule); ind int64, ascending."""
    nb_points = _at_least("nb_points", nb_points, 0)
    return _select(points, radius_neighbor_count(points, radius) > nb_points)


def cluster_dbscan(points, eps, min_points, return_core=False):
    """DBSCAN labels [n] int32: clusters numbered from 0 in ascending order of their smallest core index, -1 for noise
    (rules R4 - R6).  A point is core when at least min_points points lie within eps of it, itself counted; a border point
    takes the label of its nearest core point (ties to the lower index), so the labels are a function of the input alone.
    With return_core also the core flags [n] bool."""
    eps = _positive("eps", eps)
    min_points = _at_least("min_points", min_points, 1)
    P = _cloud(points)
    n, dev = P.shape[0], P.device
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    core = torch.empty(n, dtype=torch.uint8, device=dev) if return_core else None
    num = torch.empty(1, dtype=torch.int32, device=dev)
    _call("scorp_cloud_dbscan", P, eps, min(min_points, 2 ** 31 - 1), labels, core, None, num)
    return (labels, core.bool()) if return_core else labels


def keep_largest_clusters(labels, cluster_to_keep=1):
    """bool mask [n] of the points in the `cluster_to_keep` clusters with the most points (ties go to the lower label).
    Noise (-1) is never kept.  Plain torch, on the labels' device."""
    keep_n = _at_least("cluster_to_keep", cluster_to_keep, 1)
    labels = torch.as_tensor(labels)
    if labels.dim() != 1 or labels.dtype.is_floating_point:
        raise ValueError(f"labels must be an integer tensor [n]; got {labels.dtype} {tuple(labels.shape)}")
    labels = labels.to(torch.int64)
    member = labels >= 0
    if not bool(member.any()):
        return torch.zeros_like(member)
    counts = torch.bincount(labels[member])
    order = torch.sort(counts, descending=True, stable=True).indices   # (stable: equal counts stay in label order)
    kept = order[:keep_n][counts[order[:keep_n]] > 0]
    return member & torch.isin(labels, kept)


def voxel_down_sample(points, voxel_size, colors=None, return_inverse=False):
    """One point per occupied cell of a grid of `voxel_size`: the float64 mean of the cell's members, rounded to float32
    (rules 1 - 3 of the vertex-clustering block of include/scorp_gs.h, driven exactly as mesh.simplify does: the grid's
    origin is the cloud's minimum - voxel_size / 2, cells are numbered by their smallest point index).  Returns the points
    [C, 3]; with `colors` [n, 3] a tuple (points, colors [C, 3]) of the means of both; with return_inverse the tuple also
    ends with inverse [n] int64, the output point each input point went to."""
    from .mesh.simplify import check_grid_fits, cluster_cells_gpu
    h = _positive("voxel_size", voxel_size)
    if colors is not None and tuple(np.shape(colors)) != tuple(np.shape(points)):
        raise ValueError(f"colors must have the points' shape {tuple(np.shape(points))}; got {tuple(np.shape(colors))}")
    P = _cloud(points)
    lo, hi = P.amin(0), P.amax(0)
    check_grid_fits(torch.stack([lo, hi]).cpu().numpy().astype(np.float64), h)
    col = P if colors is None else torch.as_tensor(colors).to(device=P.device, dtype=torch.float32).contiguous()
    cell, positions, colours = cluster_cells_gpu(P, col, None, lo.contiguous(), h, 0)
    out = (positions,) + (() if colors is None else (colours,)) + ((cell.to(torch.int64),) if return_inverse else ())
    return out[0] if len(out) == 1 else out


def clean_gaussians(gaussians, method="dbscan", **kw):
    """bool mask3d [N] of the Gaussians of a GaussianModel or a GaussianModel2D to keep, by their centres (get_xyz), ready
    for segment.apply_mask3d:
      "dbscan"       eps, min_points, cluster_to_keep=1: the largest clusters of cluster_dbscan;
      "statistical"  nb_neighbors=20, std_ratio=2.0: remove_statistical_outlier;
      "radius"       nb_points, radius: remove_radius_outlier."""
    from .segment import _model_kind
    if method not in METHODS:
        raise ValueError(f"unknown method {method!r}: expected one of {list(METHODS)}")
    _model_kind(gaussians)
    xyz = gaussians.get_xyz.detach()
    if method == "dbscan":
        keep_n = kw.pop("cluster_to_keep", 1)
        return keep_largest_clusters(cluster_dbscan(xyz, **kw), keep_n)
    _, ind = (remove_statistical_outlier if method == "statistical" else remove_radius_outlier)(xyz, **kw)
    mask = torch.zeros(xyz.shape[0], dtype=torch.bool, device=ind.device)
    mask[ind] = True
    return mask
