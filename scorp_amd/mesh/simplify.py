"""Simplification by vertex clustering (csrc/mesh_simplify.hip, with a numpy form for CPU tensors).  The rules are in
include/scorp_gs.h."""
from functools import partial

import numpy as np
import torch

from .. import _C
from ._common import Mesh, check_mesh, empty_mesh
from ._common import drop_unreferenced as _drop_unreferenced   # (simplify_vertex_clustering has an argument of that name)
from ._topology import _dot3, _face_cross, proper_faces, table_slots

CONTRACTIONS = ("average", "quadric")
CELL_SIDE = 1 << 21             # cell indices per axis: three pack into one 63-bit key
QUADRIC_TRUNCATE = 1e-3         # eigenvalues of a cell's quadric below this fraction of the largest do not move the point


def _simplify_numpy(v32, col, f, h, quadric):
    """Rules 1 - 5 of include/scorp_gs.h (vertex clustering) in vectorised numpy float64: (vertex_cell [Nv] int32,
    positions [C, 3] float32, colours [C, 3] float32, faces [K, 3] int32)."""
    v = v32.astype(np.float64)
    origin = v32.min(0).astype(np.float64) - 0.5 * h
    ijk = np.floor((v - origin) / h).astype(np.int64)
    _, first, inverse = np.unique(ijk[:, 0] << 42 | ijk[:, 1] << 21 | ijk[:, 2], return_index=True, return_inverse=True)
    order = np.argsort(first)                        # the cells by their smallest vertex index
    number = np.empty_like(order)
    number[order] = np.arange(order.size)
    cell = number[inverse.reshape(-1)]
    C = order.size
    count = np.bincount(cell, minlength=C).astype(np.float64)
    total = lambda w: np.stack([np.bincount(cell, weights=w[:, k], minlength=C) for k in range(3)], 1)
    mean = total(v) / count[:, None]
    colours = (total(col.astype(np.float64)) / count[:, None]).astype(np.float32)
    positions = mean.astype(np.float32)
    if quadric:
        centre = origin + (ijk[first[order]] + 0.5) * h
        f64 = f.astype(np.int64)
        p0, N = v[f64[:, 0]], _face_cross(v32, f)
        length = np.sqrt(_dot3(N, N))
        live = length > 0.0
        f64, p0, N, length = f64[live], p0[live], N[live], length[live]
        a = 0.5 * length
        n = N / length[:, None]
        an = a[:, None] * n
        corner_cell = cell[f64]                                                  # [T, 3]
        rel = p0[:, None, :] - centre[corner_cell]                               # v0 - p_c per corner
        d = -((n[:, None, 0] * rel[..., 0] + n[:, None, 1] * rel[..., 1]) + n[:, None, 2] * rel[..., 2])
        ad = a[:, None] * d                                                      # [T, 3]
        where = corner_cell.reshape(-1)
        A = np.zeros((C, 3, 3))
        b = np.zeros((C, 3))
        for j in range(3):
            for k in range(j, 3):
                A[:, j, k] = A[:, k, j] = np.bincount(where, weights=np.repeat(an[:, j] * n[:, k], 3), minlength=C)
            b[:, j] = np.bincount(where, weights=(ad * n[:, None, j]).reshape(-1), minlength=C)
        m = mean - centre
        sigma, vec = np.linalg.eigh(A)
        sigma, vec = sigma[:, ::-1], vec[:, :, ::-1]
        r = -b - ((A[:, :, 0] * m[:, None, 0] + A[:, :, 1] * m[:, None, 1]) + A[:, :, 2] * m[:, None, 2])
        x = m.copy()
        with np.errstate(all="ignore"):
            for i in range(3):   # the eigenpairs in descending order, each term as the header writes it
                t = ((vec[:, 0, i] * r[:, 0] + vec[:, 1, i] * r[:, 1]) + vec[:, 2, i] * r[:, 2]) / sigma[:, i]
                x += np.where((sigma[:, i] > QUADRIC_TRUNCATE * sigma[:, 0])[:, None], vec[:, :, i] * t[:, None], 0.0)
        moved = (count > 1) & (sigma[:, 0] > 0.0) & (np.abs(x) <= h).all(1)
        positions = np.where(moved[:, None], (centre + x).astype(np.float32), positions)
    t = cell[f.astype(np.int64)]
    t = t[proper_faces(t)]
    t = np.take_along_axis(t, (np.argmin(t, 1)[:, None] + np.arange(3)[None]) % 3, 1)
    if t.shape[0]:
        _, keep = np.unique(t, axis=0, return_index=True)   # the first (smallest-index) face of every ordered triple
        t = t[np.sort(keep)]
    return cell.astype(np.int32), positions, colours, t.astype(np.int32).reshape(-1, 3)


def check_grid_fits(ends, h):
    """The host-side extent check of rule 1: `ends` [2, 3] float64, the bounding box; every cell index must be < 2^21."""
    origin = ends[0] - 0.5 * h
    if not (np.floor((ends[1] - origin) / h) < CELL_SIDE).all():
        raise ValueError(f"an extent of {tuple((ends[1] - ends[0]).tolist())} at voxel_size {h} needs more than 2^21 cells on an axis")


def cluster_cells_gpu(verts, colors, faces, lo, h, quadric):
    """Rules 1 - 4 on the GPU: (vertex_cell [Nv] int32, positions [C, 3], colours [C, 3]) of the points `verts` with their
    `colors`, lo their minimum per axis (a device tensor).  faces may be None with quadric = 0: a bare cloud
    (cloud.voxel_down_sample)."""
    dev = verts.device
    Nv, F = verts.shape[0], 0 if faces is None else faces.shape[0]
    i32 = partial(torch.empty, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        slots = table_slots(Nv, 2)
        keys = torch.empty(slots, dtype=torch.int64, device=dev)
        owner, slot, overflow = i32(slots), i32(Nv), i32(1)
        _C.call("scorp_mesh_simplify_cells", verts, Nv, lo, h, keys, owner, slots, slot, overflow)
        rep = i32(Nv)
        is_root = torch.empty(Nv, dtype=torch.uint8, device=dev)
        _C.call("scorp_mesh_simplify_roots", owner, slots, slot, Nv, rep, is_root)
        del keys, owner, slot
        rep_scan = torch.cumsum(is_root, 0, dtype=torch.int32)
        C = int(rep_scan[-1])
        if int(overflow):   # (the extent was checked on the host: this does not happen)
            raise ValueError("a vertex lies outside the grid of 2^21 cells per axis")
        vertex_cell, cell_ijk = i32(Nv), i32(C, 3)
        acc = torch.empty(C, 16, dtype=torch.float64, device=dev)
        _C.call("scorp_mesh_simplify_accumulate", verts, colors, Nv, faces, F, lo, h, rep, rep_scan, C, quadric, vertex_cell, cell_ijk, acc)
        positions = torch.empty(C, 3, dtype=torch.float32, device=dev)
        colours = torch.empty(C, 3, dtype=torch.float32, device=dev)
        _C.call("scorp_mesh_simplify_place", acc, cell_ijk, C, lo, h, quadric, positions, colours)
    return vertex_cell, positions, colours


def _simplify_gpu(verts, colors, faces, lo, h, quadric):
    dev = verts.device
    Nv, F = verts.shape[0], faces.shape[0]
    vertex_cell, positions, colours = cluster_cells_gpu(verts, colors, faces, lo, h, quadric)
    with torch.cuda.device(dev):
        slots = table_slots(F, 2)
        table, rotated = torch.empty(slots, dtype=torch.int32, device=dev), torch.empty(F, 3, dtype=torch.int32, device=dev)
        keep = torch.empty(F, dtype=torch.uint8, device=dev)
        _C.call("scorp_mesh_simplify_faces", faces, F, vertex_cell, Nv, table, slots, rotated, keep)
        return vertex_cell, positions, colours, rotated[keep.bool()]


def cluster_vertices(mesh, voxel_size, contraction="average"):
    """The clustering behind simplify_vertex_clustering with its vertex map: (vertex_cell [Nv] int32, Mesh) - vertex_cell[v] is
    the output vertex that input vertex v went to, and the Mesh keeps every cell's vertex, referenced or not.  An empty mesh
    (no vertices or no faces) gives an empty map and an empty Mesh."""
    if contraction not in CONTRACTIONS:
        raise ValueError(f"contraction must be one of {CONTRACTIONS}; got {contraction!r}")
    h = float(voxel_size)
    if not (h > 0.0 and np.isfinite(h)):
        raise ValueError(f"voxel_size must be positive and finite; got {voxel_size}")

    checked = check_mesh(mesh, extent=partial(check_grid_fits, h=h))
    dev = mesh.vertices.device
    if checked is None:
        return torch.empty(0, dtype=torch.int32, device=dev), empty_mesh(dev)
    verts, faces, colors, lo = checked
    quadric = 1 if contraction == "quadric" else 0
    if dev.type != "cuda":
        out = [torch.from_numpy(a) for a in _simplify_numpy(verts.numpy(), colors.numpy(), faces.numpy(), h, quadric)]
    else:
        out = _simplify_gpu(verts, colors, faces, lo.contiguous(), h, quadric)
    return out[0], Mesh(out[1], out[3].contiguous(), out[2])


def simplify_vertex_clustering(mesh, voxel_size, contraction="average", drop_unreferenced=True):
    """Reduce a Mesh by vertex clustering (Open3D's simplify_vertex_clustering; the rules are this project's own, written
    down in include/scorp_gs.h, and were never compared with Open3D's output): the vertices in one cell of a grid of
    `voxel_size` become one vertex with their mean colour, placed at their mean (contraction="average") or at the minimiser
    of the cell's plane quadrics, which keeps creases and corners ("quadric"); faces are mapped through the cells, those with
    two equal cells and repeated ordered triples are dropped.  Cells are numbered by their smallest vertex index.  With
    `drop_unreferenced` the output vertices no surviving face references are removed (survivors keep their order, faces are
    re-indexed).  Returns a new Mesh on the mesh's device.  CUDA tensors run csrc/mesh_simplify.hip, CPU tensors a numpy form
    of the same rules.  For a target triangle count, and a reduction that follows the detail instead of a grid, see
    simplify_quadric_decimation.

        mesh = simplify_vertex_clustering(post_process_mesh(ex.extract_mesh_unbounded(resolution=1024)), voxel_size=0.02)
    """
    _, out = cluster_vertices(mesh, voxel_size, contraction)
    if not drop_unreferenced or out.faces.shape[0] == 0 and out.vertices.shape[0] == 0:
        return out
    return Mesh(*_drop_unreferenced(out.vertices, out.faces, out.colors))
