"""Measuring a mesh: the exact distance from points to a triangle mesh, area-weighted surface samples, the nearest point of a
cloud, and the accuracy / completeness / chamfer / Hausdorff / F-score figures built on them (csrc/mesh_distance.hip, or a
numpy form of the same statements for CPU tensors).  The rules are the mesh-distance block of include/scorp_gs.h."""
import ctypes
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np
import torch

from .. import _C
from ._common import check_mesh
from ._topology import _cross3, _dot3

MAX_QUERIES = (1 << 31) - 1      # the C ABI's bound on queries and samples
MAX_CLOUD_POINTS = 1 << 30       # ... and on the points of a cloud to search
PAIR_CAP_FACTOR, PAIR_CAP_FLOOR = 8, 4096   # rule 3: at most 8 F + 4096 (cell, triangle) pairs
_CHUNK_PAIRS = 1 << 21           # (query, triangle) pairs per trip of the numpy forms
_U64 = np.uint64


class PointMeshDistance(NamedTuple):
    """squared_distance [Q] float64, face [Q] int32 (-1: nothing within max_distance), closest [Q, 3] float32"""
    squared_distance: torch.Tensor
    face: torch.Tensor
    closest: torch.Tensor

    @property
    def distance(self):
        return self.squared_distance.sqrt()


class NearestPoint(NamedTuple):
    """squared_distance [Q] float64, index [Q] int32 (-1: no point within max_distance)"""
    squared_distance: torch.Tensor
    index: torch.Tensor

    @property
    def distance(self):
        return self.squared_distance.sqrt()


@dataclass
class SurfaceSamples:
    """points [n, 3] float32, faces [n] int32, barycentric [n, 3] float32 (the weights of the face's three corners)"""
    points: torch.Tensor
    faces: torch.Tensor
    barycentric: torch.Tensor


@dataclass
class MeshDistance:
    """accuracy: the mean distance from the samples of a to b; completeness: from those of b to a; chamfer: their mean;
    hausdorff_ab / hausdorff_ba: the maxima; precision / recall / f_score: one value per threshold (the share of a's samples
    within the threshold of b, of b's within it of a, and their harmonic mean); samples_a / samples_b: the counts."""
    accuracy: float
    completeness: float
    chamfer: float
    hausdorff_ab: float
    hausdorff_ba: float
    thresholds: tuple
    precision: tuple
    recall: tuple
    f_score: tuple
    samples_a: int
    samples_b: int


# ---- the numpy forms ----

def _along(a, t, e):
    return a + t[..., None] * e


def _closest_on_segment(a, e, ap):
    t, den = _dot3(ap, e), _dot3(e, e)
    on = _along(a, t / den, e)
    return np.where((~(t > 0.0))[..., None], a, np.where((t >= den)[..., None], a + e, on))


def _closest_on_triangle(P, A, ab, ac, bc):
    """rules 4 and 5 of include/scorp_gs.h, statement for statement, over broadcast arrays [..., 3]"""
    n = _cross3(ab, ac)
    ap = P - A
    B, C = A + ab, A + ac
    # rule 5
    c0, c1, c2 = _closest_on_segment(A, ab, ap), _closest_on_segment(B, bc, P - B), _closest_on_segment(C, -ac, P - C)
    e0, e1, e2 = (_dot3(P - c, P - c) for c in (c0, c1, c2))
    seg, eb = c0, e0
    seg, eb = np.where((e1 < eb)[..., None], c1, seg), np.where(e1 < eb, e1, eb)
    seg = np.where((e2 < eb)[..., None], c2, seg)
    # rule 4
    d1, d2 = _dot3(ab, ap), _dot3(ac, ap)
    bp = ap - ab
    d3, d4 = _dot3(ab, bp), _dot3(ac, bp)
    vc = d1 * d4 - d3 * d2
    cp = ap - ac
    d5, d6 = _dot3(ab, cp), _dot3(ac, cp)
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    s = _dot3(n, ap) / _dot3(n, n)
    out = P - s[..., None] * n
    cases = [                                        # last to first, so that the first true condition wins
        ((va <= 0.0) & (d4 - d3 >= 0.0) & (d5 - d6 >= 0.0), _along(B, (d4 - d3) / ((d4 - d3) + (d5 - d6)), bc)),
        ((vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0), _along(A, d2 / (d2 - d6), ac)),
        ((d6 >= 0.0) & (d5 <= d6), C),
        ((vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0), _along(A, d1 / (d1 - d3), ab)),
        ((d3 >= 0.0) & (d4 <= d3), B),
        ((d1 <= 0.0) & (d2 <= 0.0), A),
    ]
    for cond, point in cases:
        out = np.where(cond[..., None], point, out)
    flat = (n[..., 0] == 0.0) & (n[..., 1] == 0.0) & (n[..., 2] == 0.0)
    return np.where(flat[..., None], seg, out)


def _grid_centre(verts):
    """rule 1: the centre of the bounding box of all vertices, as icp_grid_setup_kernel takes it"""
    v = verts.astype(np.float64)
    return 0.5 * (v.min(0) + v.max(0))


def _point_mesh_numpy(points, verts, faces, max_distance):
    """Rules 4 - 7 by brute force over all (query, triangle) pairs: the grid only decides which pairs the kernel looks at,
    never a value, so the minimum of (d^2, face) over all of them is the same statement."""
    Q, F = points.shape[0], faces.shape[0]
    d2_out, face_out = np.full(Q, np.inf), np.full(Q, -1, np.int32)
    closest = np.full((Q, 3), np.nan, np.float32)
    if Q == 0 or F == 0:
        return d2_out, face_out, closest
    ct = _grid_centre(verts)
    v64 = verts.astype(np.float64)
    a, b, c = (v64[faces[:, k]] for k in range(3))
    A, ab, ac, bc = (a - ct)[None], (b - a)[None], (c - a)[None], (c - b)[None]
    lo, hi = v64.min(0) - ct, v64.max(0) - ct
    max_d2 = float(max_distance) * float(max_distance)
    step = max(1, _CHUNK_PAIRS // F)
    with np.errstate(all="ignore"):
        for s in range(0, Q, step):
            q = points[s:s + step]
            P = q.astype(np.float64) - ct
            cl = _closest_on_triangle(P[:, None, :], A, ab, ac, bc)
            u = P[:, None, :] - cl
            d2 = _dot3(u, u)
            f = np.argmin(d2, 1)                       # (the first of equal minima: the lower face index)
            rows = np.arange(len(q))
            best = d2[rows, f]
            e = np.maximum(np.maximum(lo - P, P - hi), 0.0)
            ok = np.isfinite(q).all(1) & ((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2] <= max_d2) & (best <= max_d2)
            d2_out[s:s + step] = np.where(ok, best, np.inf)
            face_out[s:s + step] = np.where(ok, f, -1)
            closest[s:s + step] = np.where(ok[:, None], (cl[rows, f] + ct).astype(np.float32), np.float32(np.nan))
    return d2_out, face_out, closest


def _mix(z):
    z = z + _U64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> _U64(27))) * _U64(0x94D049BB133111EB)
    return z ^ (z >> _U64(31))


def _variate(seed, i, k):
    """u(i, k) of include/scorp_gs.h for an array of sample numbers (uint64)"""
    with np.errstate(over="ignore"):
        z = _mix(_mix(_mix(np.array([seed], _U64)) ^ i) ^ _U64(k))
    return (z >> _U64(11)).astype(np.float64) * 2.0 ** -53


def _sample_numpy(verts, faces, prefix, n, seed):
    i = np.arange(n, dtype=_U64)
    total = prefix[-1]
    t = ((np.arange(n, dtype=np.float64) + _variate(seed, i, 0)) / float(n)) * total
    t = np.where(t < total, t, np.nextafter(total, 0.0))
    f = np.searchsorted(prefix, t, side="right").astype(np.int32)
    s, r = np.sqrt(_variate(seed, i, 1)), _variate(seed, i, 2)
    w = np.stack([1.0 - s, s * (1.0 - r), s * r], 1)
    A, B, C = (verts.astype(np.float64)[faces[f, k]] for k in range(3))
    p = (w[:, 0:1] * A + w[:, 1:2] * B) + w[:, 2:3] * C
    return p.astype(np.float32), f, w.astype(np.float32)


def _nearest_numpy(points, cloud, max_distance):
    """the rule of icp_nearest by brute force: fp32 d^2 on centre-relative coordinates, the first (lowest) index of the
    minimum, searched to r^2 (1 + 1e-5); then the pair's d^2 in float64"""
    Q = points.shape[0]
    d2_out, idx = np.full(Q, np.inf), np.full(Q, -1, np.int32)
    if Q == 0:
        return d2_out, idx
    ct = _grid_centre(cloud)
    t64 = cloud.astype(np.float64) - ct
    tq = t64.astype(np.float32).astype(np.float64)
    r2 = float(max_distance) * float(max_distance)
    with np.errstate(all="ignore"):
        r2f = np.float32(r2) * (np.float32(1.0) + np.float32(1e-5))
        step = max(1, _CHUNK_PAIRS // cloud.shape[0])
        for s in range(0, Q, step):
            q = points[s:s + step]
            x64 = q.astype(np.float64) - ct
            x = x64.astype(np.float32).astype(np.float64)
            u = (tq[None] - x[:, None]).astype(np.float32).astype(np.float64)
            zz = (u[..., 2] * u[..., 2]).astype(np.float32).astype(np.float64)      # fmaf(ux, ux, fmaf(uy, uy, uz uz))
            yz = (u[..., 1] * u[..., 1] + zz).astype(np.float32).astype(np.float64)
            d2f = (u[..., 0] * u[..., 0] + yz).astype(np.float32)
            j = np.argmin(d2f, 1)
            rows = np.arange(len(q))
            w = x64 - t64[j]
            d2 = w[:, 0] * w[:, 0] + (w[:, 1] * w[:, 1] + w[:, 2] * w[:, 2])
            ok = np.isfinite(q).all(1) & (d2f[rows, j] <= r2f) & (d2 <= r2)
            d2_out[s:s + step] = np.where(ok, d2, np.inf)
            idx[s:s + step] = np.where(ok, j, -1)
    return d2_out, idx


# ---- the public functions ----

def _check_points(points, what, dev):
    if not isinstance(points, torch.Tensor):
        points = torch.as_tensor(np.asarray(points))
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"{what} must be [N, 3]; got {tuple(points.shape)}")
    if points.shape[0] > MAX_QUERIES:
        raise ValueError(f"more than 2^31 - 1 {what}: {points.shape[0]}")
    return points.to(device=dev, dtype=torch.float32).contiguous()


def _check_max_distance(max_distance):
    r = float(max_distance)
    if not r >= 0.0:
        raise ValueError(f"max_distance must not be negative or NaN; got {max_distance}")
    return r


class _MeshGrid:
    """The workspace of csrc/mesh_distance.hip for one mesh on a CUDA device: build once, query any number of times with up
    to `max_queries` points a call (scripts/time_mesh_distance.py times the two apart).  header: the eight numbers scorp_mesh_distance_build returns."""

    def __init__(self, verts, faces, max_queries):
        self.verts, self.faces, self.max_queries = verts, faces, max(1, int(max_queries))
        Nv, F = verts.shape[0], faces.shape[0]
        size = _C.lib().scorp_mesh_distance_workspace_bytes(F, self.max_queries)
        self.workspace = torch.empty(size, dtype=torch.uint8, device=verts.device)
        head = (ctypes.c_int64 * 8)()
        _C.call("scorp_mesh_distance_build", verts, Nv, faces, F, self.workspace, size, head)
        self.header = dict(zip(("pairs", "pair_cap", "cells", "cell_cap", "dim_x", "dim_y", "dim_z", "grow"), (int(x) for x in head)))

    def query(self, points, max_distance):
        Q, dev = points.shape[0], points.device
        d2 = torch.empty(Q, dtype=torch.float64, device=dev)
        face = torch.empty(Q, dtype=torch.int32, device=dev)
        closest = torch.empty(Q, 3, dtype=torch.float32, device=dev)
        if Q > self.max_queries:
            raise ValueError(f"{Q} queries for a workspace of {self.max_queries}")
        _C.call("scorp_mesh_distance_query", self.verts, self.verts.shape[0], self.faces, self.faces.shape[0], points, Q, max_distance,
                d2, face, closest, self.workspace, self.workspace.numel())
        return PointMeshDistance(d2, face, closest)


def point_mesh_distance(points, mesh, max_distance=float("inf"), header=None):
    """The unsigned distance from every point [Q, 3] to the nearest triangle of `mesh` (the nearest TRIANGLE, not the nearest
    vertex; the use of Open3D's RaycastingScene.compute_closest_points).  Returns a PointMeshDistance on the mesh's device:
    squared_distance [Q] float64, face [Q] int32, closest [Q, 3] float32, and .distance = sqrt of the first.  Where nothing
    lies within `max_distance`, and for a query with a NaN or an infinity, face is -1, squared_distance +inf and closest NaN;
    an empty mesh gives that for every query.  Every (query, triangle) value is float64 arithmetic on the float32 inputs, the
    result is the least (d^2, face index) and a function of the inputs alone: the same call twice, the queries in another
    order, or split over two calls, give the same bits.  A face with collinear or repeated vertices counts as its three
    segments.  `header`, a list, receives the grid's figures (pairs, pair_cap, cells, ...) on a CUDA device.
    CUDA tensors run csrc/mesh_distance.hip (a uniform grid of (cell, triangle) pairs, the queries in Morton order, an
    outward ring walk per query); CPU tensors run the same statements in numpy over ALL pairs, meant for small inputs."""
    r = _check_max_distance(max_distance)
    checked = check_mesh(mesh)
    dev = mesh.vertices.device
    pts = _check_points(points, "points", dev)
    Q = pts.shape[0]
    if checked is None or Q == 0:
        return PointMeshDistance(torch.full((Q,), float("inf"), dtype=torch.float64, device=dev),
                                 torch.full((Q,), -1, dtype=torch.int32, device=dev),
                                 torch.full((Q, 3), float("nan"), dtype=torch.float32, device=dev))
    verts, faces, _, _ = checked
    if dev.type != "cuda":
        d2, face, closest = _point_mesh_numpy(pts.numpy(), verts.numpy(), faces.numpy(), r)
        return PointMeshDistance(torch.from_numpy(d2), torch.from_numpy(face), torch.from_numpy(closest))
    with torch.cuda.device(dev):
        grid = _MeshGrid(verts, faces, Q)
        if header is not None:
            header.append(grid.header)
        return grid.query(pts, r)


def triangle_area_prefix(mesh):
    """The inclusive float64 prefix sum of the triangle areas [F] (0.5 |(B - A) x (C - A)| in float64 on the float32 vertices):
    the array sample_points_uniformly searches."""
    v = mesh.vertices.to(torch.float64)
    f = mesh.faces.long()
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    return torch.cumsum(0.5 * torch.linalg.cross(b - a, c - a).norm(dim=1), 0)


def sample_points_uniformly(mesh, number_of_points, seed=0, area_prefix=None):
    """`number_of_points` points on the surface of `mesh`, area-weighted, stratified and deterministic (the use of Open3D's
    sample_points_uniformly): sample i takes its area coordinate from the i-th of n equal slices of the total area, so the
    face index never falls as i rises and a face of area a receives n a / A_total samples to within one; the three variates
    of a sample are a counter-based hash of (seed, i, k).  Faces of zero area are never chosen; a mesh of zero area raises.
    `area_prefix` [F] float64 replaces triangle_area_prefix(mesh).  Returns SurfaceSamples on the mesh's device; the same
    arguments give the same bits, and CPU and CUDA tensors the same faces."""
    n = int(number_of_points)
    if n < 0 or n > MAX_QUERIES:
        raise ValueError(f"number_of_points must be in [0, 2^31 - 1]; got {number_of_points}")
    checked = check_mesh(mesh)
    if checked is None:
        raise ValueError("cannot sample an empty mesh")
    verts, faces, _, _ = checked
    dev = verts.device
    prefix = triangle_area_prefix(mesh) if area_prefix is None else area_prefix
    prefix = prefix.to(device=dev, dtype=torch.float64).contiguous()
    if tuple(prefix.shape) != (faces.shape[0],):
        raise ValueError(f"area_prefix must be [{faces.shape[0]}]; got {tuple(prefix.shape)}")
    total = float(prefix[-1])
    if not (total > 0.0 and np.isfinite(total)):
        raise ValueError(f"the mesh has no area to sample (total {total})")
    seed = int(seed) & ((1 << 64) - 1)
    if dev.type != "cuda":
        p, f, w = _sample_numpy(verts.numpy(), faces.numpy(), prefix.numpy(), n, seed)
        return SurfaceSamples(torch.from_numpy(p), torch.from_numpy(f), torch.from_numpy(w))
    points = torch.empty(n, 3, dtype=torch.float32, device=dev)
    chosen = torch.empty(n, dtype=torch.int32, device=dev)
    bary = torch.empty(n, 3, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _C.call("scorp_mesh_sample_points", verts, verts.shape[0], faces, faces.shape[0], prefix, n, seed, points, chosen, bary)
    return SurfaceSamples(points, chosen, bary)


def nearest_point_distance(points, cloud, max_distance=float("inf")):
    """The nearest point of `cloud` [N, 3] to every point [Q, 3]: the ICP's grid search for plain point clouds (the use of
    Open3D's compute_point_cloud_distance; DTU-style ground truth is a scan).  The nearest point is chosen by fp32 d^2 on
    coordinates relative to the cloud's centre, ties to the lower index; returns NearestPoint(squared_distance [Q] float64
    of the chosen pair, index [Q] int32), -1 and +inf where nothing lies within `max_distance` or the query is not finite.
    The cloud must be finite and not empty."""
    r = _check_max_distance(max_distance)
    if not isinstance(cloud, torch.Tensor):
        cloud = torch.as_tensor(np.asarray(cloud))
    dev = cloud.device
    cloud = _check_points(cloud, "cloud", dev)
    pts = _check_points(points, "points", dev)
    N, Q = cloud.shape[0], pts.shape[0]
    if N < 1 or N > MAX_CLOUD_POINTS:
        raise ValueError(f"the cloud must have between 1 and 2^30 points; got {N}")
    if not bool(torch.isfinite(cloud).all()):
        raise ValueError("the cloud's points are not all finite")
    if dev.type != "cuda":
        d2, idx = _nearest_numpy(pts.numpy(), cloud.numpy(), r)
        return NearestPoint(torch.from_numpy(d2), torch.from_numpy(idx))
    d2 = torch.empty(Q, dtype=torch.float64, device=dev)
    idx = torch.empty(Q, dtype=torch.int32, device=dev)
    if Q:
        _C.call_with_workspace("scorp_nearest_point_distance", "scorp_nearest_point_workspace_bytes", (Q, N), pts, Q, cloud, N, r, d2, idx)
    return NearestPoint(d2, idx)


def _metrics(d_ab, d_ba, thresholds):
    """The figures of MeshDistance from the two distance vectors: one stacked tensor crosses to the host."""
    th = tuple(float(t) for t in thresholds)
    parts = [d_ab.mean(), d_ba.mean(), d_ab.max(), d_ba.max()]
    for t in th:
        parts += [(d_ab <= t).to(torch.float64).mean(), (d_ba <= t).to(torch.float64).mean()]
    vals = torch.stack(parts).cpu().tolist()
    acc, comp, hab, hba = vals[:4]
    prec, rec = tuple(vals[4::2]), tuple(vals[5::2])
    f = tuple(2.0 * p * r / (p + r) if p + r > 0.0 else 0.0 for p, r in zip(prec, rec))
    return MeshDistance(acc, comp, 0.5 * (acc + comp), hab, hba, th, prec, rec, f, d_ab.shape[0], d_ba.shape[0])


def mesh_distance(a, b, samples=100_000, thresholds=(), seed=0):
    """How far apart two meshes are: `samples` surface samples of each (sample_points_uniformly, seeds `seed` and `seed` + 1)
    are measured against the other's surface by point_mesh_distance.  Returns a MeshDistance: accuracy (a to b), completeness
    (b to a), chamfer, the two one-sided Hausdorff distances over the samples, and precision, recall and F-score per
    threshold (the DTU / Tanks-and-Temples figures when b is the ground truth).  All distances are unsigned and in the
    meshes' units; only the final scalars leave the device.  Both meshes must be on one device and have area."""
    sa = sample_points_uniformly(a, samples, seed).points
    sb = sample_points_uniformly(b, samples, seed + 1).points
    if sa.shape[0] == 0:
        raise ValueError("samples must be positive")
    return _metrics(point_mesh_distance(sa, b).distance, point_mesh_distance(sb, a).distance, thresholds)


def mesh_cloud_distance(mesh, cloud, samples=100_000, thresholds=(), seed=0):
    """mesh_distance with a point cloud, a scan, as the other side: accuracy is the mean distance from `samples` surface
    samples of the mesh to their nearest cloud points (nearest_point_distance), completeness the mean distance from the
    cloud's points to the mesh's surface (point_mesh_distance); hausdorff_ab is mesh to cloud.  samples_b is the cloud's size."""
    sa = sample_points_uniformly(mesh, samples, seed).points
    if sa.shape[0] == 0:
        raise ValueError("samples must be positive")
    cloud = _check_points(cloud, "cloud", mesh.vertices.device)
    return _metrics(nearest_point_distance(sa, cloud).distance, point_mesh_distance(cloud, mesh).distance, thresholds)
