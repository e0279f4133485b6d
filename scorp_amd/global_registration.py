"""Global registration from geometry alone on the GPU: the FPFH descriptor, nearest-descriptor matching and RANSAC over the
matched pairs - what a user of Open3D looks for next to registration_icp (compute_fpfh_feature,
registration_ransac_based_on_feature_matching).  One RANSAC pose and one ICP run replace the 67 ICP runs of
get_ICP_fitting_transformation_best's rotation sweep, and the rotation table stops being a dependency:

    from scorp_amd.global_registration import get_FPFH_fitting_transformation
    T = get_FPFH_fitting_transformation(pc_xyz_original, pc_xyz_refined, threshold)

The descriptor and its neighbour search are csrc/cloud_fpfh.hip (scorp_cloud_fpfh), the 33-dimensional brute-force match
is csrc/feature_match.hip (scorp_feature_match); the pose fit is scorp_pose_ransac as it stands and the refinement is
registration_icp.  The rules F1 - F5 and M1 are in include/scorp_gs.h; they are this project's own.  Open3D was never run
where this was written: where a rule follows what Open3D is believed to do, that is believed, unchecked.

The descriptor depends on the sign of every normal.  orient_normals_away_from is the cheap orientation, right on
star-shaped objects; orient_normals_consistent_tangent_plane (csrc/cloud_orient.hip, scorp_cloud_orient_normals, rules
O1 - O6) propagates signs along the minimum spanning forest of the neighbour graph and is the one for cups and shelves:
get_FPFH_fitting_transformation(..., orientation="tangent_plane").
"""
import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _C
from ._points import _at_least, _check_finite, _cloud, _device, _points, _positive
from .cloud import knn_mean_distance, voxel_down_sample
from .icp import downsample_indices, estimate_normals, registration_icp
from .pose_fit import MAX_HYPOTHESES, ransac_fit

FPFH_DIM = 33
MAX_NN = 64
MATCH_TILE = 64   # target rows per LDS tile of scorp_feature_match (scorp_feature_match_tile_rows(); the tests sit on its edges)


@dataclass
class RansacRegistration:
    """What registration_ransac_based_on_feature_matching returns: the 4x4 float64 transform (source -> target, the
    winner's refit over its inliers), the winner's inlier count over the correspondences, fitness = inlier_count /
    #correspondences, the correspondences [c, 2] (source index, target index), the winner's inlier mask [c] and every
    surviving hypothesis's count."""
    transformation: np.ndarray
    inlier_count: int
    fitness: float
    correspondences: np.ndarray
    inlier_mask: np.ndarray
    counts: np.ndarray


def match_split_rows(ns, nt):
    """Target rows per split of a scorp_feature_match call of ns x nt rows (host arithmetic; for the tests' edges)."""
    return int(_C.lib().scorp_feature_match_split_rows(int(ns), int(nt)))


def orient_normals_away_from(points, normals, center=None):
    """normals with every n flipped for which dot(n, p - c) < 0, c the float64 mean of the points unless `center` is
    given; a zero dot leaves n unchanged.  Plain torch, the dot in float64; returns a tensor of the normals' dtype on
    their device.  The cheap orientation the descriptor needs on a star-shaped object: estimate_normals signs by the
    largest component, which is not equivariant under rotation.  Right only for an object that is roughly star-shaped
    about c: the inner wall of a cup points away from the centroid and is signed inwards.  For everything else there is
    orient_normals_consistent_tangent_plane."""
    N = normals if isinstance(normals, torch.Tensor) else torch.as_tensor(np.asarray(normals))
    P = points if isinstance(points, torch.Tensor) else torch.as_tensor(np.asarray(points))
    if P.dim() != 2 or P.shape[1] != 3 or P.shape[0] == 0:
        raise ValueError(f"points must be [n, 3]; got {tuple(P.shape)}")
    if tuple(N.shape) != tuple(P.shape):
        raise ValueError(f"normals must have the points' shape {tuple(P.shape)}; got {tuple(N.shape)}")
    P = P.to(device=N.device, dtype=torch.float64)
    if center is None:
        c = P.sum(0) / P.shape[0]
    else:
        c = torch.as_tensor(np.asarray(center.detach().cpu() if isinstance(center, torch.Tensor) else center, dtype=np.float64),
                            device=N.device)
        if tuple(c.shape) != (3,):
            raise ValueError(f"center must be [3]; got {tuple(c.shape)}")
    d = P - c
    n64 = N.to(torch.float64)
    dot = (n64[:, 0] * d[:, 0] + n64[:, 1] * d[:, 1]) + n64[:, 2] * d[:, 2]
    return torch.where((dot < 0)[:, None], -N, N)


COMPONENT_SIGNS = {"majority_away": _C.ORIENT_MAJORITY_AWAY, "first": _C.ORIENT_FIRST}
ORIENT_MAX_K = 64       # columns of a neighbour list scorp_cloud_orient_normals takes
ORIENT_ROUTE_K = 12     # columns of the estimate_normals list the route orients over


def orient_normals_consistent_tangent_plane(points, normals, k=12, neighbors=None, center=None, component_sign="majority_away",
                                            return_info=False):
    """normals with signs made consistent between neighbouring tangent planes (rules O1 - O6 of include/scorp_gs.h): the
    signs are propagated along the minimum spanning forest of the neighbour graph, edge weight 1 - |n_i . n_j|, and each
    connected component is then signed as a whole - with component_sign="majority_away" so that most of its normals point
    away from `center` (default: the float64 mean of the points), with "first" so that its smallest index keeps its normal.
    One call of scorp_cloud_orient_normals (csrc/cloud_orient.hip), no read-back inside it; every output is a function of
    the input alone.

    Without `neighbors` the graph is cloud.knn_mean_distance(points, min(k + 1, 32), return_neighbors=True)[1]: the exact
    k nearest, the point itself included (and ignored).  With `neighbors` any [n, <= 64] int32 list is taken as it is:
    estimate_normals(..., return_neighbors=True), the FPFH list, or their first columns; entries < 0 are padding, an entry
    >= n raises ValueError.  Returns the normals in their dtype on their device; with return_info a tuple (normals, info),
    info a dict of flip [n] bool, label [n] int32 (the smallest index of the point's component), tree [t, 2] int64 (the
    forest's edges (lo, hi), sorted) and n_components.

    The limit: a wall thinner than the neighbourhood radius joins its two sides by edges of weight near 0 (antiparallel
    normals have |dot| = 1) and is oriented wrongly.  Keep k small (the default 12) on thin-walled objects."""
    if component_sign not in COMPONENT_SIGNS:
        raise ValueError(f"unknown component_sign {component_sign!r}: expected one of {sorted(COMPONENT_SIGNS)}")
    shape = tuple(np.shape(points))
    if len(shape) != 2 or shape[1] != 3 or shape[0] == 0:
        raise ValueError(f"points must be [n, 3] with n >= 1; got {shape}")
    if shape[0] > 2 ** 30:
        raise ValueError("points has more than 2^30 points")
    if tuple(np.shape(normals)) != shape:
        raise ValueError(f"normals must have the points' shape {shape}; got {tuple(np.shape(normals))}")
    n = shape[0]
    if neighbors is None:
        k = _at_least("k", k, 1)
        if k > ORIENT_MAX_K:
            raise ValueError(f"k must be in [1, {ORIENT_MAX_K}]; got {k}")
    else:
        nshape = tuple(np.shape(neighbors))
        if len(nshape) != 2 or nshape[0] != n or not 1 <= nshape[1] <= ORIENT_MAX_K:
            raise ValueError(f"neighbors must be [{n}, 1 .. {ORIENT_MAX_K}]; got {nshape}")
        dt = neighbors.dtype if isinstance(neighbors, torch.Tensor) else np.asarray(neighbors).dtype
        if dt != (torch.int32 if isinstance(neighbors, torch.Tensor) else np.int32):
            raise ValueError(f"neighbors must be int32; got {dt}")
    c = None
    if center is not None:
        c = np.asarray(center.detach().cpu() if isinstance(center, torch.Tensor) else center, dtype=np.float64)
        if tuple(c.shape) != (3,):
            raise ValueError(f"center must be [3]; got {tuple(c.shape)}")
        if not np.isfinite(c).all():
            raise ValueError("center must be finite")
        c = (ctypes.c_double * 3)(*c.tolist())
    _check_finite("points", points)
    _check_finite("normals", normals)
    given = normals.detach() if isinstance(normals, torch.Tensor) else torch.as_tensor(np.asarray(normals))
    dev = _device(points, normals, neighbors)
    P = _points("points", points, dev)
    N = _points("normals", given, dev)
    if neighbors is None:
        nb = knn_mean_distance(P, min(k + 1, 32), return_neighbors=True)[1]
    else:
        nb = (neighbors.detach() if isinstance(neighbors, torch.Tensor) else torch.as_tensor(np.asarray(neighbors))).to(dev).contiguous()
        if int(nb.max()) >= n:
            raise ValueError(f"neighbors holds an index >= n = {n}")
    kk = nb.shape[1]
    out = torch.empty(n, 3, dtype=torch.float32, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    flip = label = tree = None
    if return_info or out.dtype != given.dtype or given.device != dev:
        flip = torch.empty(n, dtype=torch.uint8, device=dev)
    if return_info:
        label = torch.empty(n, dtype=torch.int32, device=dev)
        tree = torch.empty(n, 2, dtype=torch.int32, device=dev)
    _C.call_with_workspace("scorp_cloud_orient_normals", "scorp_cloud_orient_workspace_bytes", (n, kk),
                           P, N, nb, n, kk, c, COMPONENT_SIGNS[component_sign], out, flip, label, tree, counts)
    if given.dtype != torch.float32 or given.device != dev:   # the caller's dtype and device: a negation is exact in every float type
        out = torch.where(flip.to(given.device).bool()[:, None], -given, given)
    if not return_info:
        return out
    edges = tree[tree[:, 0] >= 0].to(torch.int64).cpu().numpy()
    edges = edges[np.lexsort((edges[:, 1], edges[:, 0]))]
    n_components, n_edges = (int(v) for v in counts.cpu())
    if not len(edges) == n_edges == n - n_components:
        raise RuntimeError(f"scorp_cloud_orient_normals: {len(edges)} tree rows, counts {n_components} components / {n_edges} edges of {n} points")
    return out, {"flip": flip.bool(), "label": label, "tree": torch.from_numpy(edges), "n_components": n_components}


def compute_fpfh_feature(points, normals, radius, max_nn=64, return_neighbors=False):
    """The FPFH descriptor [n, 33] float64 (a device tensor) of a cloud with normals (rules F1 - F5): per point the at most
    max_nn nearest other points within `radius` in ascending (d^2, index), the three 11-bin histograms of the Darboux
    angles of its pairs (SPFH), and the 1 / d^2-weighted sum of its neighbours' SPFH, each block scaled to 100, plus its
    own.  The normals are used as given, not normalised.  Open3D's max_nn counts the point itself and is believed,
    unchecked, to be this one + 1.  With return_neighbors a tuple (feature, neighbors [n, max_nn] int32 padded with -1,
    degree [n] int32, spfh_count [n, 33] int32)."""
    r = _positive("radius", radius)
    max_nn = _at_least("max_nn", max_nn, 1)
    if max_nn > MAX_NN:
        raise ValueError(f"max_nn must be in [1, {MAX_NN}]; got {max_nn}")
    if tuple(np.shape(normals)) != tuple(np.shape(points)):
        raise ValueError(f"normals must have the points' shape {tuple(np.shape(points))}; got {tuple(np.shape(normals))}")
    _check_finite("normals", normals)
    P = _cloud(points)
    N = _points("normals", normals, P.device)
    n, dev = P.shape[0], P.device
    feature = torch.empty(n, FPFH_DIM, dtype=torch.float64, device=dev)
    nb = deg = cnt = None
    if return_neighbors:
        nb = torch.empty(n, max_nn, dtype=torch.int32, device=dev)
        deg = torch.empty(n, dtype=torch.int32, device=dev)
        cnt = torch.empty(n, FPFH_DIM, dtype=torch.int32, device=dev)
    _C.call_with_workspace("scorp_cloud_fpfh", "scorp_cloud_fpfh_workspace_bytes", (n, max_nn), P, N, n, r, max_nn, feature, cnt, nb, deg)
    return (feature, nb, deg, cnt) if return_neighbors else feature


def _check_features(name, f):
    shape = tuple(np.shape(f))
    if len(shape) != 2 or shape[1] != FPFH_DIM or shape[0] == 0:
        raise ValueError(f"{name} must be [n, {FPFH_DIM}] with n >= 1; got {shape}")
    if shape[0] > 2 ** 30:
        raise ValueError(f"{name} has more than 2^30 rows")
    _check_finite(name, f)


def _features(f, device):
    t = f.detach() if isinstance(f, torch.Tensor) else torch.as_tensor(np.asarray(f))
    return t.to(device=device, dtype=torch.float32).contiguous()   # the float64 descriptor is rounded ONCE, here


def _match(S, T):
    ns, nt, dev = S.shape[0], T.shape[0], S.device
    index = torch.empty(ns, dtype=torch.int32, device=dev)
    d2 = torch.empty(ns, dtype=torch.float64, device=dev)
    _C.call_with_workspace("scorp_feature_match", "scorp_feature_match_workspace_bytes", (ns, nt), S, ns, T, nt, index, d2)
    return index, d2


def match_features(source_feature, target_feature, mutual_filter=False):
    """(index [ns] int32, d2 [ns] float64): for every source row the target row of smallest (D2, index), D2 the float64
    squared distance of the rows rounded once to float32 (rule M1).  With mutual_filter a third result, the bool mask
    back[index[i]] == i, `back` from a second call with the roles swapped."""
    _check_features("source_feature", source_feature)
    _check_features("target_feature", target_feature)
    dev = _device(source_feature, target_feature)
    S, T = _features(source_feature, dev), _features(target_feature, dev)
    index, d2 = _match(S, T)
    if not mutual_filter:
        return index, d2
    back, _ = _match(T, S)
    mutual = back[index.to(torch.int64)].to(torch.int64) == torch.arange(S.shape[0], device=dev)
    return index, d2, mutual


def edge_length_mask(source_pairs, target_pairs, triples, threshold):
    """bool [H]: the triples that pass Open3D's edge-length check (believed, unchecked: CorrespondenceCheckerBasedOnEdgeLength) -
    for each of the three edges (a, b) of a triple, with ls = |s_a - s_b| and lt = |t_a - t_b| over the matched pairs,
    ls >= threshold lt and lt >= threshold ls, in float64 torch."""
    S = torch.as_tensor(source_pairs).to(torch.float64)
    T = torch.as_tensor(target_pairs).to(device=S.device, dtype=torch.float64)
    tri = torch.as_tensor(triples).to(device=S.device, dtype=torch.int64)
    ok = torch.ones(tri.shape[0], dtype=torch.bool, device=S.device)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        ls = torch.linalg.norm(S[tri[:, a]] - S[tri[:, b]], dim=1)
        lt = torch.linalg.norm(T[tri[:, a]] - T[tri[:, b]], dim=1)
        ok &= (ls >= threshold * lt) & (lt >= threshold * ls)
    return ok


def select_triples(source_pairs, target_pairs, triples, edge_length_threshold):
    """The triples [h, 3] that go to the pose fit: those with a repeated index dropped, then those that fail
    edge_length_mask.  The order of the survivors is the order given."""
    tri = torch.as_tensor(triples).to(torch.int64)
    distinct = (tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])
    tri = tri[distinct]
    return tri[edge_length_mask(source_pairs, target_pairs, tri, edge_length_threshold).to(tri.device)]


def _check_ransac_args(source, target, source_feature, target_feature, max_correspondence_distance, n_hypotheses, edge_length_threshold,
                       samples):
    for name, pts, feat in (("source", source, source_feature), ("target", target, target_feature)):
        shape = tuple(np.shape(pts))
        if len(shape) != 2 or shape[1] != 3 or shape[0] == 0:
            raise ValueError(f"{name} must be [n, 3]; got {shape}")
        if tuple(np.shape(feat)) != (shape[0], FPFH_DIM):
            raise ValueError(f"{name}_feature must be [{shape[0]}, {FPFH_DIM}]; got {tuple(np.shape(feat))}")
        _check_finite(name, pts)
    _positive("max_correspondence_distance", max_correspondence_distance)
    e = float(edge_length_threshold)
    if not 0.0 <= e <= 1.0:
        raise ValueError(f"edge_length_threshold must be in [0, 1]; got {edge_length_threshold}")
    if samples is None:
        n_hypotheses = _at_least("n_hypotheses", n_hypotheses, 1)
        if n_hypotheses > MAX_HYPOTHESES:
            raise ValueError(f"n_hypotheses above {MAX_HYPOTHESES} is not supported")
    else:
        shape = tuple(np.shape(samples))
        if len(shape) != 2 or shape[1] != 3 or not 1 <= shape[0] <= MAX_HYPOTHESES:
            raise ValueError(f"samples must be [H, 3] with 1 <= H <= {MAX_HYPOTHESES}; got {shape}")


def registration_ransac_based_on_feature_matching(source, target, source_feature, target_feature, max_correspondence_distance,
                                                  mutual_filter=True, n_hypotheses=4096, edge_length_threshold=0.9, seed=0,
                                                  samples=None):
    """The rigid transform source -> target by RANSAC over descriptor matches, as a RansacRegistration.

    The correspondences are match_features(source_feature, target_feature): every source point with its nearest target
    descriptor; with mutual_filter only the mutual ones, unless fewer than 3 are mutual, then all.  Triples of
    correspondences are drawn by numpy.random.default_rng(seed).integers(0, c, (n_hypotheses, 3)), or are
    `samples` [H, 3] as given; triples with a repeated index are dropped, then those that fail the edge-length check
    (edge_length_mask); ValueError when none is left.  The rest go to scorp_pose_ransac (Kabsch, float64 pairs, threshold =
    max_correspondence_distance) as it stands: every hypothesis is counted over the CORRESPONDENCE set - believed,
    unchecked, to be the rule of Open3D's current ..._based_on_correspondence; there is no nearest-neighbour fitness pass
    over all points - the first with the highest count wins and is refitted over its inliers.  ValueError("No inliers
    found in RANSAC.") when the winner has fewer than 3 inliers, as pc_align_ransac raises it."""
    _check_ransac_args(source, target, source_feature, target_feature, max_correspondence_distance, n_hypotheses, edge_length_threshold,
                       samples)
    dev = _device(source, target, source_feature, target_feature)
    P = torch.as_tensor(np.asarray(source) if not isinstance(source, torch.Tensor) else source.detach()).to(device=dev, dtype=torch.float64)
    Q = torch.as_tensor(np.asarray(target) if not isinstance(target, torch.Tensor) else target.detach()).to(device=dev, dtype=torch.float64)
    index, _, *mutual = match_features(source_feature, target_feature, mutual_filter=bool(mutual_filter))
    src_idx = torch.arange(P.shape[0], device=dev)
    if mutual_filter and int(mutual[0].sum()) >= 3:
        src_idx = src_idx[mutual[0]]
    corr = torch.stack([src_idx, index.to(torch.int64)[src_idx]], dim=1)
    c = corr.shape[0]
    if c < 3:
        raise ValueError(f"at least 3 correspondences are required; got {c}")
    S, T = P[corr[:, 0]].contiguous(), Q[corr[:, 1]].contiguous()
    if samples is None:
        tri = np.random.default_rng(seed).integers(0, c, (int(n_hypotheses), 3))
    else:
        tri = samples.detach().cpu().numpy() if isinstance(samples, torch.Tensor) else np.asarray(samples)
        if not np.issubdtype(tri.dtype, np.integer) or tri.min() < 0 or tri.max() >= c:
            raise ValueError(f"samples must be integer correspondence indices in [0, {c})")
    tri = select_triples(S, T, torch.as_tensor(tri, device=dev), float(edge_length_threshold))
    if tri.shape[0] == 0:
        raise ValueError("no sample triple passes the distinct-index and edge-length checks")
    fit = ransac_fit(S, T, tri.to(torch.int32), float(max_correspondence_distance), method="kabsch")
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = fit.R, fit.t
    return RansacRegistration(M, fit.count, fit.count / c, corr.cpu().numpy(), fit.mask, fit.counts)


def default_voxel_size(points):
    """The mean edge of the points' bounding box / 32."""
    P = np.asarray(points.detach().cpu() if isinstance(points, torch.Tensor) else points, dtype=np.float64)
    return float((P.max(0) - P.min(0)).mean() / 32.0)


def get_FPFH_fitting_transformation(pc_xyz_original, pc_xyz_refined, threshold, *, voxel_size=None, max_iteration=400,
                                    estimation="point_to_point", seed=0, return_icp=False, orientation="away_from"):
    """The 4x4 float64 transform (refined -> original), the convention of get_ICP_fitting_transformation_best, from one
    global registration and ONE ICP run instead of a sweep over tabulated rotations.

    Both clouds go through voxel_down_sample(voxel_size), by default the mean edge of the original's bounding box / 32;
    their normals are estimate_normals(knn=30) followed by orient_normals_away_from (so the object should be roughly
    star-shaped about its centroid); FPFH with radius 5 voxel_size and max_nn 64; RANSAC with distance 1.5 voxel_size; then
    one registration_icp from that pose at `threshold` on the full clouds, the refined one thinned by downsample_indices
    as the sweep thins it.  The 5 x and 1.5 x ratios are the customary ones of Open3D's global-registration example; they
    are UNMEASURED on real objects.  With return_icp a tuple (transform, ICPResult of the one run).
    estimation="generalized" refines with generalized ICP on estimate_covariances of the two clouds that run registers.
    estimation="colored" is refused: this function takes no colours (refine with registration_icp from the returned pose).

    orientation="tangent_plane": the normals are signed by orient_normals_consistent_tangent_plane over the first 12 columns
    of estimate_normals' own neighbour list instead, for objects that are not star-shaped (cups, shelves).  The default
    stays "away_from": no existing call changes its result."""
    if orientation not in ("away_from", "tangent_plane"):
        raise ValueError(f"unknown orientation {orientation!r}: expected 'away_from' or 'tangent_plane'")
    if estimation == "colored":
        raise ValueError("estimation='colored' needs colours, which this function does not take: refine its pose with "
                         "registration_icp(..., estimation='colored', source_colors=, target_colors=)")
    threshold = _positive("threshold", threshold)
    orig, ref = np.asarray(pc_xyz_original), np.asarray(pc_xyz_refined)
    for name, a in (("pc_xyz_original", orig), ("pc_xyz_refined", ref)):
        if a.ndim != 2 or a.shape[1] != 3 or a.shape[0] < 3:
            raise ValueError(f"{name} must be [n, 3] with n >= 3; got {a.shape}")
        _check_finite(name, a)
    voxel = default_voxel_size(orig) if voxel_size is None else _positive("voxel_size", voxel_size)
    if not voxel > 0.0:
        raise ValueError("the original cloud's bounding box is a point: no default voxel_size")
    down, feat = [], []
    for a in (ref, orig):
        P = voxel_down_sample(a, voxel)
        knn = min(30, max(3, P.shape[0]))
        if orientation == "tangent_plane":
            N, nb = estimate_normals(P, knn=knn, return_neighbors=True)
            N = orient_normals_consistent_tangent_plane(P, N, neighbors=nb[:, :ORIENT_ROUTE_K])
        else:
            N = orient_normals_away_from(P, estimate_normals(P, knn=knn))
        down.append(P)
        feat.append(compute_fpfh_feature(P, N, 5.0 * voxel, MAX_NN))
    reg = registration_ransac_based_on_feature_matching(down[0], down[1], feat[0], feat[1], 1.5 * voxel, seed=seed)
    src = ref[downsample_indices(len(orig), len(ref))]
    res = registration_icp(src, orig, threshold, reg.transformation, max_iteration=max_iteration, estimation=estimation)
    T = res.transformation[0].copy()
    return (T, res) if return_icp else T
