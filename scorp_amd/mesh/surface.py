"""The surface of a dense grid: surface nets (csrc/isosurface.hip) and marching cubes (csrc/marching_cubes.hip), each with a
numpy form for CPU tensors."""
import numpy as np
import torch

from .. import _C, mc_table
from ._common import _check_method


def _surface_nets_numpy(f, coords, level):
    """The rules of include/scorp_gs.h (surface extraction) in vectorised numpy float32: the CPU form of extract_surface."""
    f = np.ascontiguousarray(f, np.float32)
    X, Y, Z = f.shape
    level = np.float32(level)
    inside = f < level

    def corner(a, n):   # the values at corner n (4 di + 2 dj + dk) of every cell
        di, dj, dk = n >> 2, (n >> 1) & 1, n & 1
        return a[di:X - 1 + di, dj:Y - 1 + dj, dk:Z - 1 + dk]
    s = [np.zeros((X - 1, Y - 1, Z - 1), np.float32) for _ in range(3)]
    cnt = np.zeros((X - 1, Y - 1, Z - 1), np.int32)
    with np.errstate(all="ignore"):
        for axis in range(3):
            step = 4 >> axis
            for n0 in range(8):
                if n0 & step:
                    continue
                v0, v1 = corner(f, n0), corner(f, n0 + step)
                cross = corner(inside, n0) != corner(inside, n0 + step)
                t = (level - v0) / (v1 - v0)
                fixed = (np.float32(n0 >> 2), np.float32((n0 >> 1) & 1), np.float32(n0 & 1))
                for d in range(3):
                    s[d] += np.where(cross, t if d == axis else fixed[d], np.float32(0)).astype(np.float32)
                cnt += cross
    active = cnt > 0
    ids = (np.cumsum(active.ravel(), dtype=np.int64) - 1).reshape(active.shape)
    ci, cj, ck = np.nonzero(active)
    n = cnt[active].astype(np.float32)
    verts = np.empty((ci.size, 3), np.float32)
    for d, (c, idx) in enumerate(zip(coords, (ci, cj, ck))):
        c = np.asarray(c, np.float32)
        verts[:, d] = c[idx] + (s[d][active] / n) * (c[idx + 1] - c[idx])
    # quads: lattice edges q -> q + e_a, in the order (q, a)
    E = np.zeros((X, Y, Z, 3), bool)
    mid = [np.zeros(m, bool) for m in (X, Y, Z)]
    for m in mid:
        m[1:-1] = True
    mi, mj, mk = mid[0][:, None, None], mid[1][None, :, None], mid[2][None, None, :]
    E[:-1, :, :, 0] = (inside[:-1] != inside[1:]) & (mj & mk)
    E[:, :-1, :, 1] = (inside[:, :-1] != inside[:, 1:]) & (mk & mi)
    E[:, :, :-1, 2] = (inside[:, :, :-1] != inside[:, :, 1:]) & (mi & mj)
    qi, qj, qk, qa = np.nonzero(E)
    q = np.stack([qi, qj, qk], 1)
    b = np.eye(3, dtype=np.int64)[(qa + 1) % 3]
    c = np.eye(3, dtype=np.int64)[(qa + 2) % 3]
    cell = lambda p: ids[p[:, 0], p[:, 1], p[:, 2]]
    c00, c10, c11, c01 = cell(q), cell(q - b), cell(q - b - c), cell(q - c)
    qin = inside[qi, qj, qk]
    faces = np.stack([c00, np.where(qin, c10, c11), np.where(qin, c11, c10),
                      c00, np.where(qin, c11, c01), np.where(qin, c01, c11)], 1).reshape(-1, 3).astype(np.int32)
    return verts, faces


def _mc_faces_numpy(case, emit, vid, table):
    """The triangles of the cells case [..., X, Y, Z] (emit: which cells may emit) through the per-edge vertex ids
    vid [..., X + 1, Y + 1, Z + 1, 3], in ascending cell index, then table order."""
    n = np.where(emit, table[case, 15], 0)
    cells = np.nonzero(n > 0)
    rows = table[case[cells]]                                   # [m, 16]
    e = rows[:, :15].reshape(-1, 5, 3).astype(np.int64)
    live = np.arange(5)[None, :] < rows[:, 15:16]               # [m, 5]
    e = np.where(live[..., None], e, 0)
    n0, axis = mc_table.EDGE_N0[e], mc_table.EDGE_AXIS[e]
    at = tuple(c[:, None, None] for c in cells[:-3]) + tuple(
        cells[-3 + d][:, None, None] + ((n0 >> (2 - d)) & 1) for d in range(3)) + (axis,)
    return vid[at][live].astype(np.int32).reshape(-1, 3)


def _marching_cubes_numpy(f, coords, level):
    """The marching-cubes rules of include/scorp_gs.h in vectorised numpy float32: the CPU form of extract_surface."""
    f = np.ascontiguousarray(f, np.float32)
    X, Y, Z = f.shape
    level = np.float32(level)
    inside = f < level
    E = np.zeros((X, Y, Z, 3), bool)
    E[:-1, :, :, 0] = inside[:-1] != inside[1:]
    E[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    E[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    vid = (np.cumsum(E.ravel(), dtype=np.int64) - 1).reshape(E.shape)   # C order of [X, Y, Z, 3]: ascending (q, axis)
    q = np.stack(np.nonzero(E), 1)
    qa = q[:, 3]
    q1 = q[:, :3] + np.eye(3, dtype=np.int64)[qa]
    f0, f1 = f[q[:, 0], q[:, 1], q[:, 2]], f[q1[:, 0], q1[:, 1], q1[:, 2]]
    with np.errstate(all="ignore"):
        t = (level - f0) / (f1 - f0)
    verts = np.empty((q.shape[0], 3), np.float32)
    for d, c in enumerate(coords):
        c = np.asarray(c, np.float32)
        c0, c1 = c[q[:, d]], c[q1[:, d]]
        verts[:, d] = np.where(qa == d, c0 + t * (c1 - c0), c0)
    case = np.zeros((X - 1, Y - 1, Z - 1), np.int64)
    for n in range(8):
        di, dj, dk = n >> 2, (n >> 1) & 1, n & 1
        case |= inside[di:X - 1 + di, dj:Y - 1 + dj, dk:Z - 1 + dk].astype(np.int64) << n
    return verts, _mc_faces_numpy(case, np.ones(case.shape, bool), vid, mc_table.cached_table())


def _scan_counts(counts, limit, what):
    """The inclusive prefix sums of the count bytes a count kernel wrote, and their total n (one host read): (n, the scan as
    int32, or None when n == 0).  n >= limit does not fit the mesh's int32 indices."""
    scan = torch.cumsum(counts, 0, dtype=torch.int64)
    n = int(scan[-1])
    if n >= limit:
        raise ValueError(f"the surface has more than 2^31 - 1 {what}")
    return n, (scan.to(torch.int32) if n else None)


def _marching_cubes_gpu(f, xyz, level):
    dev = f.device
    X, Y, Z = f.shape
    verts = torch.empty(0, 3, dtype=torch.float32, device=dev)
    faces = torch.empty(0, 3, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        masks = torch.empty(X * Y * Z, dtype=torch.uint8, device=dev)
        counts = torch.empty(X * Y * Z, dtype=torch.uint8, device=dev)
        _C.call("scorp_marching_cubes_count_edges", f, X, Y, Z, level, masks, counts)
        nv, edge_scan = _scan_counts(counts, 2 ** 31, "vertices")
        if nv == 0:
            return verts, faces
        verts = torch.empty(nv, 3, dtype=torch.float32, device=dev)
        _C.call("scorp_marching_cubes_emit_vertices", f, *xyz, X, Y, Z, level, masks, edge_scan, nv, verts)
        counts = torch.empty((X - 1) * (Y - 1) * (Z - 1), dtype=torch.uint8, device=dev)
        _C.call("scorp_marching_cubes_count_faces", f, X, Y, Z, level, counts)
        nf, face_scan = _scan_counts(counts, 2 ** 31, "triangles")
        if nf == 0:
            return verts, faces
        faces = torch.empty(nf, 3, dtype=torch.int32, device=dev)
        _C.call("scorp_marching_cubes_emit_faces", f, X, Y, Z, level, masks, edge_scan, face_scan, nf, faces)
    return verts, faces


def _surface_nets_gpu(f, xyz, level):
    dev = f.device
    X, Y, Z = f.shape
    verts = torch.empty(0, 3, dtype=torch.float32, device=dev)
    faces = torch.empty(0, 3, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        flags = torch.empty((X - 1) * (Y - 1) * (Z - 1), dtype=torch.uint8, device=dev)
        _C.call("scorp_isosurface_count_cells", f, X, Y, Z, level, flags)
        nv, cell_scan = _scan_counts(flags, 2 ** 31, "vertices")
        if nv == 0:
            return verts, faces
        verts = torch.empty(nv, 3, dtype=torch.float32, device=dev)
        _C.call("scorp_isosurface_emit_vertices", f, *xyz, X, Y, Z, level, cell_scan, nv, verts)
        counts = torch.empty(X * Y * Z, dtype=torch.uint8, device=dev)
        _C.call("scorp_isosurface_count_faces", f, X, Y, Z, level, counts)
        nq, edge_scan = _scan_counts(counts, 2 ** 30, "triangles")   # (two triangles per quad)
        if nq == 0:
            return verts, faces
        faces = torch.empty(2 * nq, 3, dtype=torch.int32, device=dev)
        _C.call("scorp_isosurface_emit_faces", f, X, Y, Z, level, cell_scan, edge_scan, nq, faces)
    return verts, faces


def extract_surface(grid, coords, level=0.0, method="surface_nets"):
    """The surface f = level of the dense grid [X, Y, Z] (inside: f < level) over the lattice coords = (x, y, z):
    (vertices [Nv, 3] float32, faces [Nf, 3] int32) on the grid's device, in the fixed order of include/scorp_gs.h.
    method "surface_nets" puts one vertex in every cell the surface crosses; "marching_cubes" one on every lattice edge it
    crosses, with the triangles of the case table of scorp_amd/mc_table.py.  The triangles' normals point from inside to
    outside."""
    _check_method(method)
    if not isinstance(grid, torch.Tensor) or grid.dim() != 3:
        raise ValueError("grid must be a [X, Y, Z] tensor")
    if len(coords) != 3 or any(c.dim() != 1 or c.numel() != n for c, n in zip(coords, grid.shape)):
        raise ValueError("coords must be three 1-D tensors matching the grid's shape")
    if min(grid.shape) < 2:
        raise ValueError(f"every grid dimension must be at least 2; got {tuple(grid.shape)}")
    dev = grid.device
    f = grid.to(torch.float32).contiguous()
    xyz = [c.to(device=dev, dtype=torch.float32).contiguous() for c in coords]
    if dev.type != "cuda":
        form = _marching_cubes_numpy if method == "marching_cubes" else _surface_nets_numpy
        v, t = form(f.numpy(), [c.numpy() for c in xyz], level)
        return torch.from_numpy(v), torch.from_numpy(t)
    form = _marching_cubes_gpu if method == "marching_cubes" else _surface_nets_gpu
    return form(f, xyz, float(level))
