"""Smoothing a mesh, and its normals: the per-vertex adjacency of a triangle mesh in CSR form, face and vertex normals,
Laplacian and Taubin smoothing, the normal map of a rendered mesh and its comparison with another normal map
(csrc/mesh_smooth.hip, or a numpy form of the same statements for CPU tensors).  The rules are the mesh-smooth block of
include/scorp_gs.h and they are this project's own: every sum runs in float64 in a fixed order (a vertex's neighbours
ascending, its faces ascending) with contraction off, so every result is a function of the inputs alone - which a float32
index_add_ over an edge list is not.  Nothing was compared with Open3D's filter_smooth_laplacian, filter_smooth_taubin or
compute_vertex_normals; the inverse-distance weights are what Open3D's Laplacian filter is believed to use, unchecked."""
import ctypes
import math
from dataclasses import dataclass

import numpy as np
import torch

from .. import _C
from ._common import Mesh, check_mesh
from ._topology import _face_cross, _unit, edge_keys, vertex_face_csr
from .render import MAX_RENDER_VIEWS

WEIGHTINGS = {"area": _C.MESH_NORMALS_AREA, "uniform": _C.MESH_NORMALS_UNIFORM}                         # rule 6
SMOOTH_WEIGHTS = {"uniform": _C.MESH_SMOOTH_UNIFORM, "inverse_distance": _C.MESH_SMOOTH_INVERSE_DISTANCE}   # rule 7
DISTANCE_EPS = 1e-12             # rule 7: added to the distance before it is inverted
MAX_SMOOTH_STEPS = 1 << 20       # the C ABI's bound on the half-steps of one call


@dataclass
class MeshAdjacency:
    """Rules 2 - 4 for one mesh, on its device: neighbor_offsets [Nv + 1] int32 and neighbors int32 (vertex v's neighbours
    are neighbors[neighbor_offsets[v]:neighbor_offsets[v + 1]], ascending, each once), corner_offsets [Nv + 1] int32 and
    corner_faces [3 F] int32 (the faces whose corners name v, ascending, one entry per corner), boundary [Nv] bool (v is an
    end of a side that occurs exactly once over all faces)."""
    num_vertices: int
    num_faces: int
    neighbor_offsets: torch.Tensor
    neighbors: torch.Tensor
    corner_offsets: torch.Tensor
    corner_faces: torch.Tensor
    boundary: torch.Tensor


@dataclass
class NormalDifference:
    """Per view, [V] float64: mean_deg and median_deg of the angle between the two normals, in degrees, over the pixels where
    both have a non-zero length (NaN where there is none; the median of an even count is the lower of the middle two),
    reference_covered = the share of the reference's pixels where the mesh has a normal too, mesh_covered the share of the
    mesh's where the reference has.  overall: the same four figures over all views' pixels together."""
    mean_deg: torch.Tensor
    median_deg: torch.Tensor
    reference_covered: torch.Tensor
    mesh_covered: torch.Tensor
    overall: dict


# ---- the adjacency (integers: torch on either device) ----

def _offsets(counts):
    return torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)]).to(torch.int32)


def _shapes(mesh):
    """(checked or None, Nv, F, device) after check_mesh"""
    checked = check_mesh(mesh)
    return checked, int(mesh.vertices.shape[0]), int(mesh.faces.shape[0]), mesh.vertices.device


def mesh_adjacency(mesh):
    """The MeshAdjacency of `mesh` (rules 2 - 4 of the mesh-smooth block of include/scorp_gs.h), built on the edge keys and
    the vertex -> face CSR of _topology.py: 64-bit keys, a sort, unique_consecutive, counts into offsets.  Duplicate faces and non-manifold edges add
    no neighbour; a side with equal ends is ignored; an unreferenced vertex has empty slices.  Pass it as `adjacency=` to
    vertex_normals and the filters to build it once for many calls on meshes of the same faces."""
    checked, Nv, F, dev = _shapes(mesh)
    if checked is None:   # no vertices or no faces: every slice is empty
        zeros, none = torch.zeros(Nv + 1, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
        return MeshAdjacency(Nv, F, zeros, none, zeros.clone(), none.clone(), torch.zeros(Nv, dtype=torch.bool, device=dev))
    f = checked[1].long()
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)               # rule 1: the sides (a, b), (b, c), (c, a)
    proper = a != b
    a, b = a[proper], b[proper]
    directed = torch.unique_consecutive(torch.sort(torch.cat([a << 32 | b, b << 32 | a]))[0])   # rule 2: (v, neighbour) ascending, each once
    neighbors = (directed & 0xFFFFFFFF).to(torch.int32)
    neighbor_offsets = _offsets(torch.bincount(directed >> 32, minlength=Nv))
    corner_offsets, corner_faces = vertex_face_csr(f, Nv)            # rule 3 (every corner, proper side or not)
    sides, counts = torch.unique_consecutive(torch.sort(edge_keys(f).reshape(-1)[proper])[0], return_counts=True)
    once = sides[counts == 1]                                        # rule 4
    boundary = torch.zeros(Nv, dtype=torch.bool, device=dev)
    boundary[once >> 32] = True
    boundary[once & 0xFFFFFFFF] = True
    return MeshAdjacency(Nv, F, neighbor_offsets.contiguous(), neighbors.contiguous(), corner_offsets.contiguous(), corner_faces.contiguous(),
                         boundary)


def _adjacency_for(mesh, adjacency, Nv, F, dev, needed=True):
    if adjacency is None:
        return mesh_adjacency(mesh) if needed else None
    if adjacency.num_vertices != Nv or adjacency.num_faces != F:
        raise ValueError(f"the adjacency is of a mesh with {adjacency.num_vertices} vertices and {adjacency.num_faces} faces; "
                         f"this one has {Nv} and {F}")
    if adjacency.neighbors.device != dev:
        raise ValueError(f"the adjacency is on {adjacency.neighbors.device}, the mesh on {dev}")
    return adjacency


# ---- the numpy form ----

# (rule 5 is _topology.py's _face_cross and _unit)

def _ranked(offsets):
    """The slices of a CSR walked in step: yields (rows, positions) for entry 0 of every row that has one, then entry 1,
    ...: a sum that adds them in this order adds each row's entries in the CSR's order."""
    offsets = offsets.astype(np.int64)
    counts = np.diff(offsets)
    for k in range(int(counts.max()) if len(counts) else 0):
        rows = np.nonzero(counts > k)[0]
        yield rows, offsets[rows] + k


def _vertex_normals_numpy(verts, faces, corner_offsets, corner_faces, weighting):
    """rule 6"""
    n = _face_cross(verts, faces)
    if weighting == _C.MESH_NORMALS_UNIFORM:
        n = _unit(n)
    s = np.zeros((verts.shape[0], 3), np.float64)
    for rows, at in _ranked(corner_offsets):
        s[rows] = s[rows] + n[corner_faces[at]]
    return _unit(s).astype(np.float32)


def _smooth_step_numpy(src, offsets, neighbors, fixed, factor, weights):
    """rule 7: one half-step of float32 positions [Nv, 3]; a new array"""
    p = src.astype(np.float64)
    s, W = np.zeros_like(p), np.zeros(len(p), np.float64)
    with np.errstate(all="ignore"):
        for rows, at in _ranked(offsets):
            q = p[neighbors[at]]
            if weights == _C.MESH_SMOOTH_INVERSE_DISTANCE:
                d = p[rows] - q
                w = 1.0 / (np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) + DISTANCE_EPS)
            else:
                w = np.ones(len(rows), np.float64)
            s[rows] = s[rows] + w[:, None] * q
            W[rows] = W[rows] + w
        moves = np.diff(offsets.astype(np.int64)) > 0
        if fixed is not None:
            moves &= ~fixed
        out = src.copy()
        out[moves] = (p[moves] + np.float64(factor) * (s[moves] / W[moves][:, None] - p[moves])).astype(np.float32)
    return out


def _normal_map_numpy(verts, faces, normals, face_map, bary):
    """the statements of mesh_normal_map_kernel over every pixel that has a face"""
    V, H, W = face_map.shape
    out = np.zeros((V, 3, H, W), np.float32)
    vi, jj, ii = np.nonzero(face_map >= 0)
    f = face_map[vi, jj, ii].astype(np.int64)
    if normals is None:
        n = _unit(_face_cross(verts, faces))[f]
    else:
        N = normals.astype(np.float64)[faces.astype(np.int64)[f]]                 # [n, 3 corners, 3]
        b = [bary[vi, k, jj, ii].astype(np.float64)[:, None] for k in range(3)]
        n = _unit((b[0] * N[:, 0] + b[1] * N[:, 1]) + b[2] * N[:, 2])
    for ch in range(3):
        out[vi, ch, jj, ii] = n[:, ch].astype(np.float32)
    return out


# ---- the public functions ----

def face_normals(mesh, normalized=True):
    """float32 [F, 3]: rule 5 of the mesh-smooth block of include/scorp_gs.h - (b - a) x (c - a) of every face (a, b, c) in
    float64, over its length when `normalized` (a face of no area gives +0), else as it is: twice the face's area long."""
    checked, Nv, F, dev = _shapes(mesh)
    if checked is None:
        return torch.zeros(F, 3, dtype=torch.float32, device=dev)
    verts, faces = checked[0], checked[1]
    if dev.type != "cuda":
        n = _face_cross(verts.numpy(), faces.numpy())
        return torch.from_numpy((_unit(n) if normalized else n).astype(np.float32))
    out = torch.empty(F, 3, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _C.call("scorp_mesh_face_normals", verts, Nv, faces, F, 1 if normalized else 0, out)
    return out


def vertex_normals(mesh, weighting="area", adjacency=None):
    """float32 [Nv, 3], unit or +0: rule 6 - the sum of the normals of the faces at each vertex, in ascending face index, in
    float64.  weighting="area" sums (b - a) x (c - a), so a face counts by its area; "uniform" sums the unit normals.  A
    vertex with no face, and a sum of length zero, give +0.  There is no angle weighting.  The same bits on every run."""
    if weighting not in WEIGHTINGS:
        raise ValueError(f"weighting must be one of {tuple(WEIGHTINGS)}; got {weighting!r}")
    checked, Nv, F, dev = _shapes(mesh)
    adj = _adjacency_for(mesh, adjacency, Nv, F, dev, needed=checked is not None)
    if checked is None:
        return torch.zeros(Nv, 3, dtype=torch.float32, device=dev)
    verts, faces = checked[0], checked[1]
    if dev.type != "cuda":
        return torch.from_numpy(_vertex_normals_numpy(verts.numpy(), faces.numpy(), adj.corner_offsets.numpy(), adj.corner_faces.numpy(),
                                                      WEIGHTINGS[weighting]))
    out = torch.empty(Nv, 3, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _C.call("scorp_mesh_vertex_normals", verts, Nv, faces, F, adj.corner_offsets, adj.corner_faces, WEIGHTINGS[weighting], out)
    return out


def _smooth(mesh, factors, weights, fix_boundary, adjacency):
    """rule 8's driver: the half-steps `factors` in turn; a new Mesh with the faces and colours of `mesh` themselves"""
    if weights not in SMOOTH_WEIGHTS:
        raise ValueError(f"weights must be one of {tuple(SMOOTH_WEIGHTS)}; got {weights!r}")
    if len(factors) > MAX_SMOOTH_STEPS:
        raise ValueError(f"more than {MAX_SMOOTH_STEPS} half-steps: {len(factors)}")
    checked, Nv, F, dev = _shapes(mesh)
    adj = _adjacency_for(mesh, adjacency, Nv, F, dev, needed=checked is not None and bool(factors))
    if checked is None or not factors:
        return Mesh(mesh.vertices.clone(), mesh.faces, mesh.colors)
    verts = checked[0]
    fixed = adj.boundary if fix_boundary else None
    if dev.type != "cuda":
        cur, offsets, neighbors = verts.numpy(), adj.neighbor_offsets.numpy(), adj.neighbors.numpy()
        for f in factors:
            cur = _smooth_step_numpy(cur, offsets, neighbors, None if fixed is None else fixed.numpy(), f, SMOOTH_WEIGHTS[weights])
        return Mesh(torch.from_numpy(cur), mesh.faces, mesh.colors)
    out = torch.empty(Nv, 3, dtype=torch.float32, device=dev)
    scratch = torch.empty(Nv, 3, dtype=torch.float32, device=dev) if len(factors) > 1 else None
    with torch.cuda.device(dev):
        _C.call("scorp_mesh_smooth", verts, Nv, adj.neighbor_offsets, adj.neighbors, fixed, (ctypes.c_double * len(factors))(*factors),
                len(factors), SMOOTH_WEIGHTS[weights], scratch, out)
    return Mesh(out, mesh.faces, mesh.colors)


def _count(number_of_iterations):
    n = int(number_of_iterations)
    if n != number_of_iterations or n < 0:
        raise ValueError(f"number_of_iterations must be a whole number that is not negative; got {number_of_iterations}")
    return n


def _factor(name, value):
    value = float(value)
    if not math.isfinite(value):
        raise ValueError(f"{name} must be finite; got {value}")
    return value


def filter_smooth_laplacian(mesh, number_of_iterations=1, lambda_filter=0.5, weights="uniform", fix_boundary=False, adjacency=None):
    """A new Mesh whose vertices went through `number_of_iterations` half-steps of rule 7 (include/scorp_gs.h) with factor
    lambda_filter: each moves by that share towards the weighted mean of its neighbours, all from the positions of the step
    before (Jacobi).  weights: "uniform" (w = 1) or "inverse_distance" (w = 1 / (distance + 1e-12)).  fix_boundary keeps the
    vertices on an edge that only one face has where they are.  Faces and colours are the input's own tensors; zero
    iterations return the positions bit for bit.  The surface shrinks (filter_smooth_taubin's does not).  The sums are
    float64 in ascending neighbour order: the same bits on every run, unlike an index_add_ over an edge list.  The name and
    the arguments are Open3D's; the result was not compared with Open3D's."""
    n, lam = _count(number_of_iterations), _factor("lambda_filter", lambda_filter)
    return _smooth(mesh, [lam] * n, weights, fix_boundary, adjacency)


def filter_smooth_taubin(mesh, number_of_iterations=1, lambda_filter=0.5, mu=-0.53, weights="uniform", fix_boundary=False, adjacency=None):
    """filter_smooth_laplacian with each iteration a pair of half-steps, factor lambda_filter and then mu (negative, a little
    larger in size): the second undoes the shrinking of the first and leaves the smoothing (Taubin 1995)."""
    n, lam, mu = _count(number_of_iterations), _factor("lambda_filter", lambda_filter), _factor("mu", mu)
    return _smooth(mesh, [lam, mu] * n, weights, fix_boundary, adjacency)


def normal_map(render, mesh, normals=None):
    """float32 [V, 3, H, W], world space: the normal of `mesh` at every pixel of `render`, a MeshRender of that mesh.  With
    `normals` [Nv, 3] (say vertex_normals(mesh)) the three corners' normals are weighted by render.barycentric - which
    render_mesh(..., barycentric=True) fills - and normalised; with None it is the unit normal of the face (flat).  A pixel
    with no face gives +0."""
    checked, Nv, F, dev = _shapes(mesh)
    face_map = render.face
    if face_map.dim() != 3 or face_map.dtype != torch.int32:
        raise ValueError(f"render.face must be int32 [V, H, W]; got {face_map.dtype} {tuple(face_map.shape)}")
    V, H, W = (int(s) for s in face_map.shape)
    if not 1 <= V <= MAX_RENDER_VIEWS:
        raise ValueError(f"the render must have between 1 and {MAX_RENDER_VIEWS} views; got {V}")
    bary = None
    if normals is not None:
        if tuple(normals.shape) != (Nv, 3):
            raise ValueError(f"normals must be [{Nv}, 3]; got {tuple(normals.shape)}")
        if render.barycentric is None or tuple(render.barycentric.shape) != (V, 3, H, W):
            raise ValueError("normals need render.barycentric [V, 3, H, W]: render_mesh(..., barycentric=True)")
        bary = render.barycentric.to(device=dev, dtype=torch.float32).contiguous()
        normals = normals.to(device=dev, dtype=torch.float32).contiguous()
    face_map = face_map.to(dev).contiguous()
    if checked is None or H == 0 or W == 0:
        return torch.zeros(V, 3, H, W, dtype=torch.float32, device=dev)
    if int(face_map.max()) >= F:
        raise ValueError(f"render.face names face {int(face_map.max())} of {F}: the render is of another mesh")
    verts, faces = checked[0], checked[1]
    if dev.type != "cuda":
        return torch.from_numpy(_normal_map_numpy(verts.numpy(), faces.numpy(), None if normals is None else normals.numpy(), face_map.numpy(),
                                                  None if bary is None else bary.numpy()))
    out = torch.empty(V, 3, H, W, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _C.call("scorp_mesh_normal_map", verts, Nv, faces, F, normals, face_map, bary, V, H, W, out)
    return out


def normal_difference(mesh_normals, reference_normals):
    """How a mesh's normal maps [V, 3, H, W] (normal_map) differ from reference maps of the same shape (the surfel render's
    render_normal): a NormalDifference over the pixels where both have a non-zero length.  Both are normalised first - the
    surfel render_normal is alpha-weighted, so shorter than 1 where the render is not opaque - and the angle is
    acos of their clamped dot product, float64.  Plain torch; nothing leaves the device but the overall figures."""
    if mesh_normals.shape != reference_normals.shape or mesh_normals.dim() != 4 or mesh_normals.shape[1] != 3:
        raise ValueError(f"two normal stacks [V, 3, H, W] of one shape are needed; got {tuple(mesh_normals.shape)} and "
                         f"{tuple(reference_normals.shape)}")
    m, r = mesh_normals.to(torch.float64), reference_normals.to(device=mesh_normals.device, dtype=torch.float64)
    lm, lr = torch.linalg.vector_norm(m, dim=1), torch.linalg.vector_norm(r, dim=1)
    has_m, has_r = lm > 0, lr > 0
    both = has_m & has_r
    one = torch.ones((), dtype=torch.float64, device=m.device)
    cos = ((m * r).sum(1) / (torch.where(both, lm, one) * torch.where(both, lr, one))).clamp(-1.0, 1.0)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=m.device)
    angle = torch.where(both, torch.rad2deg(torch.acos(cos)), nan).flatten(1)      # [V, H W], NaN where not compared
    n_both, n_m, n_r = (t.flatten(1).sum(1).to(torch.float64) for t in (both, has_m, has_r))
    sums = torch.nan_to_num(angle, nan=0.0).sum(1)
    median = torch.nanmedian(angle, dim=1)[0]
    total = torch.stack([sums.sum(), torch.nanmedian(angle.reshape(-1)), n_both.sum(), n_m.sum(), n_r.sum()]).cpu().tolist()
    share = lambda a, b: a / b if b > 0 else float("nan")
    overall = dict(mean_deg=share(total[0], total[2]), median_deg=total[1], reference_covered=share(total[2], total[4]),
                   mesh_covered=share(total[2], total[3]))
    return NormalDifference(sums / n_both, median, n_both / n_r, n_both / n_m, overall)
