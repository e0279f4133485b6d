"""From a trained surfel model to a coloured triangle mesh: gs2dgs/utils/mesh_utils.py's GaussianExtractor
(reconstruction, estimate_bounding_sphere, extract_mesh_unbounded / compute_unbounded_tsdf) and the lattice of
gs2dgs/utils/mcube_utils.py, on the GPU.

    ex = GaussianExtractor(gaussians, render, pipe)
    ex.reconstruction(cameras)
    write_mesh_ply("mesh.ply", post_process_mesh(ex.extract_mesh_unbounded(resolution=512), cluster_to_keep=50))

The depth and colour maps stay on the device as two stacked tensors.  The TSDF of every sample is fused over all views by
one launch (csrc/tsdf.hip: scorp_tsdf_fuse), the volume is ONE dense grid (no 512^3 crops, so no crop seams and no
restriction of `resolution` to multiples of 512), and the surface is extracted by surface nets (csrc/isosurface.hip: one
vertex per cell the surface crosses, which lies in the same cell as the marching-cubes vertices of that cell) or, with
method="marching_cubes", by marching cubes (csrc/marching_cubes.hip: one vertex per crossed lattice edge, the triangles
from the case table that scorp_amd/mc_table.py generates).  `post_process_mesh` (mesh_utils.py:22-43) drops the floaters: the triangles are clustered over shared edges
by a lock-free union-find on the device (csrc/mesh_cluster.hip, Open3D's cluster_connected_triangles), the largest
clusters are kept and the mesh is compacted with torch ops, without a mesh-sized array visiting the host.
`extract_mesh_bounded`, the route the 2DGS paper reports its meshes with, fuses the same maps into a SPARSE volume instead:
16^3-voxel blocks that exist only within sdf_trunc of an observed depth point (csrc/tsdf_blocks.hip: a hashed block set, one
workgroup per block with the view loop inside), meshed by surface nets whose corner fetch goes through a block-neighbour table
(csrc/isosurface_blocks.hip) or by marching cubes that does (csrc/marching_cubes_blocks.hip).  The reference hands this to
Open3D's ScalableTSDFVolume and its marching cubes; the volume here
follows the rules written down in include/scorp_gs.h and was never compared with Open3D's own output, which was not
available.  `simplify_vertex_clustering` reduces the mesh: the vertices in one cell of a grid become one vertex, at their mean
or at the minimiser of the cell's plane quadrics (csrc/mesh_simplify.hip; the rules are this project's own, in
include/scorp_gs.h, uncompared with Open3D's simplify_vertex_clustering).  `simplify_quadric_decimation` reduces it to a
target triangle count by edge collapses, an independent set of edges per round (csrc/mesh_decimate.hip; again this
project's own rules, in include/scorp_gs.h).

CUDA tensors run the HIP kernels; CPU tensors run a torch / numpy form of the same statements.
"""
import ctypes
import os
from dataclasses import dataclass
from functools import partial

import numpy as np
import torch

from . import _C, mc_table

MAX_RANGE = 32.0            # mcube_utils.py:26,93: the un-contracted vertices are clipped to +-max_range
LAUNCH_SAMPLES = 1 << 30    # samples per scorp_tsdf_fuse call (the C ABI takes up to (2^31 - 1) * 256)


@dataclass
class Mesh:
    """vertices [Nv, 3] float32, faces [Nf, 3] int32 (vertex indices), colors [Nv, 3] float32 in [0, 1]."""
    vertices: torch.Tensor
    faces: torch.Tensor
    colors: torch.Tensor


def uncontract(y):
    """Contracted space back to the normalised one: a point of norm n >= 1 goes to norm 1 / (2 - n) on its ray, the unit
    ball stays (the inverse of the contraction n -> 2 - 1 / n that the reference's unbounded route works in)."""
    n = torch.linalg.vector_norm(y, dim=-1, keepdim=True)
    return y * torch.where(n < 1, torch.ones_like(n), 1 / ((2 - n) * n))


# ---- TSDF fusion ----

def _maps(depth, rgb, full_proj):
    if not isinstance(depth, torch.Tensor) or not isinstance(full_proj, torch.Tensor):
        raise ValueError("depth and full_proj must be torch tensors")
    if depth.dim() == 4 and depth.shape[1] == 1:
        depth = depth[:, 0]
    if depth.dim() != 3:
        raise ValueError(f"depth must be [V, H, W] or [V, 1, H, W]; got {tuple(depth.shape)}")
    V, H, W = depth.shape
    if V < 1:
        raise ValueError("no views")
    if H < 2 or W < 2:
        raise ValueError(f"the maps must be at least 2 x 2; got {H} x {W}")
    dev = depth.device
    depth = depth.to(torch.float32).contiguous()
    if rgb is not None:
        if tuple(rgb.shape) != (V, 3, H, W):
            raise ValueError(f"rgb must be [{V}, 3, {H}, {W}] like depth; got {tuple(rgb.shape)}")
        rgb = rgb.to(device=dev, dtype=torch.float32).contiguous()
    if tuple(full_proj.shape) not in ((V, 4, 4), (V, 16)):
        raise ValueError(f"full_proj must be [{V}, 4, 4] or [{V}, 16]; got {tuple(full_proj.shape)}")
    return depth, rgb, full_proj.to(device=dev, dtype=torch.float32).reshape(V, 16).contiguous()


def _bilinear(img, fx, fy, x0, y0):
    """img [C, H, W] at (fx, fy) with (x0, y0) = floor: grid_sample's four corners in its order; a corner past the last
    row / column has weight 0 and is not read."""
    H, W = img.shape[-2:]
    x1, y1 = x0 + 1, y0 + 1
    ex, ey, dx, dy = (x0 + 1).to(fx.dtype) - fx, (y0 + 1).to(fx.dtype) - fy, fx - x0.to(fx.dtype), fy - y0.to(fx.dtype)
    zero = torch.zeros((), dtype=img.dtype)

    def at(x, y):
        ok = (x < W) & (y < H)
        return torch.where(ok, img[:, y.clamp(max=H - 1), x.clamp(max=W - 1)], zero)
    return at(x0, y0) * (ex * ey) + at(x1, y0) * (dx * ey) + at(x0, y1) * (ex * dy) + at(x1, y1) * (dx * dy)


def _tsdf_fuse_torch(depth, rgb, full_proj, pts, voxel_size, contracted, center, radius):
    """scorp_tsdf_fuse's statements on CPU tensors (include/scorp_gs.h), every view over all samples at once."""
    V, H, W = depth.shape
    trunc = torch.full((pts.shape[0],), float(np.float32(5.0 * voxel_size)), dtype=torch.float32)
    if contracted:
        n = torch.sqrt((pts * pts).sum(-1))
        trunc = torch.where(n > 1, trunc * (1.0 / (2.0 - n.clamp(max=1.9))), trunc)
        k = (1.0 / (2.0 - n))[:, None]
        pts = torch.where((n < 1)[:, None], pts, k * (pts / n[:, None]))
        pts = pts * float(radius) + center
    tsdf = torch.ones(pts.shape[0])
    w = torch.ones(pts.shape[0])
    col = torch.zeros(pts.shape[0], 3)
    M = full_proj.reshape(V, 4, 4)
    for v in range(V):
        m = M[v]
        p = [pts[:, 2] * m[2, j] + (pts[:, 1] * m[1, j] + pts[:, 0] * m[0, j]) + m[3, j] for j in (0, 1, 3)]
        zc = p[2]
        u, t = p[0] / zc, p[1] / zc
        inside = (u > -1) & (u < 1) & (t > -1) & (t < 1) & (zc > 0)
        idx = torch.nonzero(inside)[:, 0]
        if idx.numel() == 0:
            continue
        fx = ((u[idx] + 1) / 2 * (W - 1)).clamp(0, W - 1)
        fy = ((t[idx] + 1) / 2 * (H - 1)).clamp(0, H - 1)
        x0, y0 = fx.floor().long(), fy.floor().long()
        sdf = _bilinear(depth[v][None], fx, fy, x0, y0)[0] - zc[idx]
        hit = sdf > -trunc[idx]
        idx, s = idx[hit], (sdf[hit] / trunc[idx[hit]]).clamp(-1.0, 1.0)
        wp = w[idx] + 1
        tsdf[idx] = (tsdf[idx] * w[idx] + s) / wp
        if rgb is not None:
            c = _bilinear(rgb[v], fx[hit], fy[hit], x0[hit], y0[hit]).T
            col[idx] = (col[idx] * w[idx][:, None] + c) / wp[:, None]
        w[idx] = wp
    return tsdf, (col if rgb is not None else None)


def tsdf_fuse(depth, rgb, full_proj, samples, voxel_size, contracted=False, center=None, radius=None):
    """compute_unbounded_tsdf (mesh_utils.py:209-247) over the views depth [V, H, W] (or [V, 1, H, W]), rgb [V, 3, H, W]
    or None, full_proj [V, 4, 4] (each camera's full_proj_transform as stored).  `samples` is [M, 3], or a tuple (x, y, z)
    of 1-D coordinate tensors: the lattice of their product in C order, never materialised on the GPU path.  With
    `contracted` the samples lie in the contracted space of the sphere (center [3], radius).  Returns the TSDF - [M], or
    [X, Y, Z] for a lattice - and, when rgb is given, (tsdf, colours [..., 3])."""
    depth, rgb, full_proj = _maps(depth, rgb, full_proj)
    dev = depth.device
    voxel_size = float(voxel_size)
    if not voxel_size > 0.0:
        raise ValueError(f"voxel_size must be positive; got {voxel_size}")
    if contracted:
        if center is None or radius is None:
            raise ValueError("contracted samples need center and radius")
        if not float(radius) > 0.0:
            raise ValueError(f"radius must be positive; got {radius}")
        center = torch.as_tensor(center, dtype=torch.float32, device="cpu").reshape(3)
    lattice = isinstance(samples, (tuple, list))
    if lattice:
        if len(samples) != 3 or any(not isinstance(c, torch.Tensor) or c.dim() != 1 or c.numel() < 1 for c in samples):
            raise ValueError("a lattice is a tuple of three non-empty 1-D coordinate tensors")
        coords = [c.to(device=dev, dtype=torch.float32).contiguous() for c in samples]
        shape = tuple(c.numel() for c in coords)
        M = shape[0] * shape[1] * shape[2]
        if max(shape) >= 2 ** 31:
            raise ValueError("a lattice axis has more than 2^31 - 1 points")
    else:
        if not isinstance(samples, torch.Tensor) or samples.dim() != 2 or samples.shape[1] != 3:
            raise ValueError("samples must be [M, 3] or a tuple (x, y, z)")
        pts = samples.to(device=dev, dtype=torch.float32).contiguous()
        M, shape = pts.shape[0], (pts.shape[0],)
    if M < 1:
        raise ValueError("no samples")
    V, H, W = depth.shape
    if not dev.type == "cuda":
        if lattice:
            pts = torch.stack(torch.meshgrid(*coords, indexing="ij"), dim=-1).reshape(-1, 3)
        tsdf, col = _tsdf_fuse_torch(depth, rgb, full_proj, pts, voxel_size, contracted, center, radius)
    else:
        L = _C.lib()
        tsdf = torch.empty(M, dtype=torch.float32, device=dev)
        col = torch.empty(M, 3, dtype=torch.float32, device=dev) if rgb is not None else None
        views = _C.ScorpTsdfViews(depth=depth.data_ptr(), rgb=rgb.data_ptr() if rgb is not None else None,
                                  full_proj=full_proj.data_ptr(), num_views=V, width=W, height=H)
        params = _C.ScorpTsdfParams(voxel_size=voxel_size, contracted=1 if contracted else 0, radius=float(radius or 0.0))
        if contracted:
            params.center[:] = center.tolist()
        smp = _C.ScorpTsdfSamples()
        if lattice:
            smp.x, smp.y, smp.z = (c.data_ptr() for c in coords)
            smp.nx, smp.ny, smp.nz = shape
        else:
            smp.xyz = pts.data_ptr()
        with torch.cuda.device(dev):
            stream = _C.current_stream_ptr()
            for first in range(0, M, LAUNCH_SAMPLES):
                smp.first, smp.count = first, min(LAUNCH_SAMPLES, M - first)
                _C.check(L.scorp_tsdf_fuse(ctypes.byref(views), ctypes.byref(smp), ctypes.byref(params), tsdf.data_ptr(),
                                           col.data_ptr() if col is not None else None, stream), "scorp_tsdf_fuse")
    tsdf = tsdf.reshape(shape)
    return (tsdf, col.reshape(*shape, 3)) if rgb is not None else tsdf


# ---- surface extraction ----

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


METHODS = ("surface_nets", "marching_cubes")


def _check_method(method):
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}; got {method!r}")


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
    L = _C.lib()
    dev = f.device
    X, Y, Z = f.shape
    verts = torch.empty(0, 3, dtype=torch.float32, device=dev)
    faces = torch.empty(0, 3, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = _C.current_stream_ptr()
        masks = torch.empty(X * Y * Z, dtype=torch.uint8, device=dev)
        counts = torch.empty(X * Y * Z, dtype=torch.uint8, device=dev)
        _C.check(L.scorp_marching_cubes_count_edges(f.data_ptr(), X, Y, Z, level, masks.data_ptr(), counts.data_ptr(), stream),
                 "scorp_marching_cubes_count_edges")
        nv, edge_scan = _scan_counts(counts, 2 ** 31, "vertices")
        if nv == 0:
            return verts, faces
        verts = torch.empty(nv, 3, dtype=torch.float32, device=dev)
        _C.check(L.scorp_marching_cubes_emit_vertices(f.data_ptr(), xyz[0].data_ptr(), xyz[1].data_ptr(), xyz[2].data_ptr(), X, Y, Z,
                                                      level, masks.data_ptr(), edge_scan.data_ptr(), nv, verts.data_ptr(), stream),
                 "scorp_marching_cubes_emit_vertices")
        counts = torch.empty((X - 1) * (Y - 1) * (Z - 1), dtype=torch.uint8, device=dev)
        _C.check(L.scorp_marching_cubes_count_faces(f.data_ptr(), X, Y, Z, level, counts.data_ptr(), stream), "scorp_marching_cubes_count_faces")
        nf, face_scan = _scan_counts(counts, 2 ** 31, "triangles")
        if nf == 0:
            return verts, faces
        faces = torch.empty(nf, 3, dtype=torch.int32, device=dev)
        _C.check(L.scorp_marching_cubes_emit_faces(f.data_ptr(), X, Y, Z, level, masks.data_ptr(), edge_scan.data_ptr(),
                                                   face_scan.data_ptr(), nf, faces.data_ptr(), stream), "scorp_marching_cubes_emit_faces")
    return verts, faces


def _surface_nets_gpu(f, xyz, level):
    L = _C.lib()
    dev = f.device
    X, Y, Z = f.shape
    verts = torch.empty(0, 3, dtype=torch.float32, device=dev)
    faces = torch.empty(0, 3, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = _C.current_stream_ptr()
        flags = torch.empty((X - 1) * (Y - 1) * (Z - 1), dtype=torch.uint8, device=dev)
        _C.check(L.scorp_isosurface_count_cells(f.data_ptr(), X, Y, Z, level, flags.data_ptr(), stream), "scorp_isosurface_count_cells")
        nv, cell_scan = _scan_counts(flags, 2 ** 31, "vertices")
        if nv == 0:
            return verts, faces
        verts = torch.empty(nv, 3, dtype=torch.float32, device=dev)
        _C.check(L.scorp_isosurface_emit_vertices(f.data_ptr(), xyz[0].data_ptr(), xyz[1].data_ptr(), xyz[2].data_ptr(), X, Y, Z,
                                                  level, cell_scan.data_ptr(), nv, verts.data_ptr(), stream),
                 "scorp_isosurface_emit_vertices")
        counts = torch.empty(X * Y * Z, dtype=torch.uint8, device=dev)
        _C.check(L.scorp_isosurface_count_faces(f.data_ptr(), X, Y, Z, level, counts.data_ptr(), stream), "scorp_isosurface_count_faces")
        nq, edge_scan = _scan_counts(counts, 2 ** 30, "triangles")   # (two triangles per quad)
        if nq == 0:
            return verts, faces
        faces = torch.empty(2 * nq, 3, dtype=torch.int32, device=dev)
        _C.check(L.scorp_isosurface_emit_faces(f.data_ptr(), X, Y, Z, level, cell_scan.data_ptr(), edge_scan.data_ptr(), nq,
                                               faces.data_ptr(), stream), "scorp_isosurface_emit_faces")
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


# ---- bounded TSDF volume: sparse 16^3-voxel blocks (the rules are in include/scorp_gs.h) ----

BLOCK_SIDE, BLOCK_VOXELS = 16, 4096
KEY_BIAS = 1 << 20          # block coordinates lie in [-2^20, 2^20)
MAX_TABLE_SLOTS = 1 << 32   # the C ABI's bound on the touch table


@dataclass
class BlockVolume:
    """A fused sparse volume.  keys [B] int64 ascending (the block keys; they are below 2^63), coords [B, 3] int32 (bx, by, bz),
    view_mask [B, ceil(V / 32)] int32 (the bits of uint32 words), tsdf / weight [B, 4096] float32, colour [B, 4096, 3] float32
    in [0, 255] or None, voxel_length."""
    keys: torch.Tensor
    coords: torch.Tensor
    view_mask: torch.Tensor
    tsdf: torch.Tensor
    weight: torch.Tensor
    colour: object
    voxel_length: float


def block_coords(keys):
    """[B] int64 keys -> [B, 3] int32 block coordinates."""
    return torch.stack([((keys >> s) & 0x1FFFFF) - KEY_BIAS for s in (42, 21, 0)], -1).to(torch.int32)


def _block_views(depth, rgb, world_to_cam, intrinsics):
    if not isinstance(depth, torch.Tensor) or not isinstance(world_to_cam, torch.Tensor):
        raise ValueError("depth and world_to_cam must be torch tensors")
    if depth.dim() == 4 and depth.shape[1] == 1:
        depth = depth[:, 0]
    if depth.dim() != 3:
        raise ValueError(f"depth must be [V, H, W] or [V, 1, H, W]; got {tuple(depth.shape)}")
    V, H, W = depth.shape
    if V < 1:
        raise ValueError("no views")
    if V > 65535:
        raise ValueError(f"more than 65535 views: {V}")
    if H < 1 or W < 1:
        raise ValueError(f"empty maps: {H} x {W}")
    dev = depth.device
    depth = depth.to(torch.float32).contiguous()
    if rgb is not None:
        if tuple(rgb.shape) != (V, H, W, 3) or rgb.dtype != torch.uint8:
            raise ValueError(f"rgb must be uint8 [{V}, {H}, {W}, 3]; got {rgb.dtype} {tuple(rgb.shape)}")
        rgb = rgb.to(dev).contiguous()
    if tuple(world_to_cam.shape) not in ((V, 3, 4), (V, 4, 4)):
        raise ValueError(f"world_to_cam must be [{V}, 3, 4] or [{V}, 4, 4]; got {tuple(world_to_cam.shape)}")
    intrinsics = torch.as_tensor(intrinsics, dtype=torch.float32)   # (a device tensor stays where it is)
    if tuple(intrinsics.shape) == (4,):
        intrinsics = intrinsics[None].expand(V, 4)
    if tuple(intrinsics.shape) != (V, 4):
        raise ValueError(f"intrinsics must be (fx, fy, cx, cy) as [4] or [{V}, 4]; got {tuple(intrinsics.shape)}")
    cam = torch.cat([world_to_cam[:, :3].to(device=dev, dtype=torch.float32).reshape(V, 12), intrinsics.to(dev)], 1).contiguous()
    return depth, rgb, cam


def _check_lengths(voxel_length, sdf_trunc, stride):
    voxel_length, sdf_trunc, stride = float(np.float32(voxel_length)), float(np.float32(sdf_trunc)), int(stride)
    if not voxel_length > 0.0:
        raise ValueError(f"voxel_length must be positive; got {voxel_length}")
    if not sdf_trunc > 0.0 or not np.float32(sdf_trunc) <= np.float32(16) * np.float32(voxel_length):
        raise ValueError(f"sdf_trunc must be in (0, 16 voxel_length]; got {sdf_trunc} with voxel_length {voxel_length}")
    if stride < 1:
        raise ValueError(f"stride must be at least 1; got {stride}")
    return voxel_length, sdf_trunc, stride


def _block_coords_numpy(keys):
    """block_coords on a numpy array of keys, in int64."""
    return np.stack([((keys >> s) & 0x1FFFFF) - KEY_BIAS for s in (42, 21, 0)], -1)


def _pack_keys_numpy(b):
    b = b.astype(np.int64) + KEY_BIAS
    return b[..., 0] << 42 | b[..., 1] << 21 | b[..., 2]


def _blocks_touch_numpy(depth, cam, voxel_length, sdf_trunc, stride):
    """The touch rule in vectorised numpy float32: (keys [B] int64 ascending, view_mask [B, words] uint32)."""
    f = np.float32
    V, H, W = depth.shape
    words = (V + 31) // 32
    block_len, trunc = f(16) * f(voxel_length), f(sdf_trunc)
    uu, vv = np.meshgrid(np.arange(0, W, stride), np.arange(0, H, stride))
    per_view = []
    with np.errstate(all="ignore"):
        for i in range(V):
            C = cam[i]
            d = depth[i][::stride, ::stride]
            ok = d > 0
            d, u, v = d[ok], uu[ok].astype(f), vv[ok].astype(f)
            q = ((u - C[14]) * d / C[12] - C[3], (v - C[15]) * d / C[13] - C[7], d - C[11])
            pw = np.stack([(C[k] * q[0] + C[4 + k] * q[1]) + C[8 + k] * q[2] for k in range(3)], -1)
            lo, hi = np.floor((pw - trunc) / block_len), np.floor((pw + trunc) / block_len)
            if not bool(((lo >= -KEY_BIAS) & (hi < KEY_BIAS)).all()):
                raise ValueError("a depth point lies outside the volume's range of 2^20 blocks per axis (or is not finite)")
            lo, hi = lo.astype(np.int64), hi.astype(np.int64)
            keys = [np.empty(0, np.int64)]
            for o in np.ndindex(3, 3, 3):
                b = lo + np.asarray(o)
                keys.append(_pack_keys_numpy(b[(b <= hi).all(-1)]))
            per_view.append(np.unique(np.concatenate(keys)))
    keys = np.unique(np.concatenate(per_view))
    mask = np.zeros((keys.size, words), np.uint32)
    for i, k in enumerate(per_view):
        mask[np.searchsorted(keys, k), i >> 5] |= np.uint32(1 << (i & 31))
    return keys, mask


def _blocks_integrate_numpy(depth, rgb, cam, keys, mask, voxel_length, sdf_trunc):
    """The integrate rule in vectorised numpy float32, one view at a time over the blocks that carry its bit."""
    f = np.float32
    V, H, W = depth.shape
    B = keys.size
    vl, trunc = f(voxel_length), f(sdf_trunc)
    coords = _block_coords_numpy(keys)
    local = np.stack(np.unravel_index(np.arange(BLOCK_VOXELS), (16, 16, 16)), -1)
    tsdf, w = np.zeros(B * BLOCK_VOXELS, f), np.zeros(B * BLOCK_VOXELS, f)
    col = np.zeros((B * BLOCK_VOXELS, 3), f) if rgb is not None else None
    u_max, v_max = f(W) - f(1e-4), f(H) - f(1e-4)
    with np.errstate(all="ignore"):
        for i in range(V):
            blocks = np.flatnonzero((mask[:, i >> 5] >> np.uint32(i & 31)) & np.uint32(1))
            if blocks.size == 0:
                continue
            C = cam[i]
            g = coords[blocks][:, None, :] * 16 + local[None]
            c = vl * (g.astype(f) + f(0.5))
            x, y, z = c[..., 0].ravel(), c[..., 1].ravel(), c[..., 2].ravel()
            at = (blocks[:, None] * BLOCK_VOXELS + np.arange(BLOCK_VOXELS)[None]).ravel()
            px, py, pz = (((C[4 * r] * x + C[4 * r + 1] * y) + C[4 * r + 2] * z) + C[4 * r + 3] for r in range(3))
            uf, vf = (px * C[12] / pz + C[14]) + f(0.5), (py * C[13] / pz + C[15]) + f(0.5)
            ok = (pz > 0) & (uf >= f(1e-4)) & (uf < u_max) & (vf >= f(1e-4)) & (vf < v_max)
            at, pz, u, v = at[ok], pz[ok], uf[ok].astype(np.int64), vf[ok].astype(np.int64)
            d = depth[i][v, u]
            rx, ry = (u.astype(f) - C[14]) / C[12], (v.astype(f) - C[15]) / C[13]
            sdf = (d - pz) * np.sqrt((rx * rx + ry * ry) + f(1))
            hit = (d > 0) & (sdf > -trunc)
            at, s, u, v = at[hit], np.minimum(f(1), sdf[hit] / trunc), u[hit], v[hit]
            wo = w[at]
            wp = wo + f(1)
            tsdf[at] = (tsdf[at] * wo + s) / wp
            if col is not None:
                col[at] = (col[at] * wo[:, None] + rgb[i][v, u].astype(f)) / wp[:, None]
            w[at] = wp
    return (tsdf.reshape(B, BLOCK_VOXELS), w.reshape(B, BLOCK_VOXELS), col.reshape(B, BLOCK_VOXELS, 3) if col is not None else None)


def _blocks_touch(views, depth, voxel_length, sdf_trunc, stride, num_slots):
    """One scorp_tsdf_blocks_touch call on a table of num_slots: (keys [B] int64 ascending, view_mask [B, words] int32,
    overflow word).  With an overflow bit set the blocks are incomplete."""
    dev = depth.device
    words = (views.num_views + 31) // 32
    keys = torch.empty(num_slots, dtype=torch.int64, device=dev)
    mask = torch.empty(num_slots, words, dtype=torch.int32, device=dev)
    overflow = torch.empty(1, dtype=torch.int32, device=dev)
    _C.check(_C.lib().scorp_tsdf_blocks_touch(ctypes.byref(views), voxel_length, sdf_trunc, stride, keys.data_ptr(), mask.data_ptr(),
                                             num_slots, overflow.data_ptr(), _C.current_stream_ptr()), "scorp_tsdf_blocks_touch")
    taken = keys != -1   # the empty key is all ones
    keys, order = torch.sort(keys[taken])
    return keys, mask[taken][order].contiguous(), int(overflow)


def tsdf_blocks_fuse(depth, rgb, world_to_cam, intrinsics, voxel_length, sdf_trunc, stride=4, num_slots=None):
    """Fuse the views depth [V, H, W] (0 = no measurement), rgb uint8 [V, H, W, 3] or None, world_to_cam [V, 3, 4] (p_cam =
    R p_w + t; [V, 4, 4] is cut), intrinsics (fx, fy, cx, cy) as [4] or [V, 4] into a BlockVolume by the rules of
    include/scorp_gs.h: every `stride`-th pixel of a view touches the blocks within sdf_trunc of its point, then every voxel of a
    touched block runs over the views that touched it.  sdf_trunc <= 16 voxel_length.  `num_slots` (a power of two) is the
    first size of the touch table; a table that turns out too small is doubled and the call repeated."""
    depth, rgb, cam = _block_views(depth, rgb, world_to_cam, intrinsics)
    voxel_length, sdf_trunc, stride = _check_lengths(voxel_length, sdf_trunc, stride)
    dev = depth.device
    V, H, W = depth.shape
    words = (V + 31) // 32
    if dev.type != "cuda":
        d, c = depth.numpy(), cam.numpy()
        keys, mask = _blocks_touch_numpy(d, c, voxel_length, sdf_trunc, stride)
        tsdf, weight, col = _blocks_integrate_numpy(d, rgb.numpy() if rgb is not None else None, c, keys, mask, voxel_length, sdf_trunc)
        keys = torch.from_numpy(keys)
        return BlockVolume(keys, block_coords(keys), torch.from_numpy(mask.view(np.int32)), torch.from_numpy(tsdf), torch.from_numpy(weight),
                           torch.from_numpy(col) if col is not None else None, voxel_length)
    L = _C.lib()
    views = _C.ScorpTsdfBlockViews(depth=depth.data_ptr(), rgb=rgb.data_ptr() if rgb is not None else None, cam=cam.data_ptr(),
                                   num_views=V, width=W, height=H)
    if num_slots is None:   # a first guess: a block per 16 sampled pixels, at load 1/2
        pixels = V * -(-W // stride) * -(-H // stride)
        num_slots = 1 << max(10, (pixels // 8).bit_length())
    num_slots = int(num_slots)
    if num_slots < 1 or num_slots & (num_slots - 1):
        raise ValueError(f"num_slots must be a power of two; got {num_slots}")
    with torch.cuda.device(dev):
        while True:
            keys, mask, overflow = _blocks_touch(views, depth, voxel_length, sdf_trunc, stride, num_slots)
            if overflow & 2:
                raise ValueError("a depth point lies outside the volume's range of 2^20 blocks per axis (or is not finite)")
            if not overflow:
                break
            if num_slots >= MAX_TABLE_SLOTS:
                raise ValueError("the touch table overflows at 2^32 slots")
            num_slots *= 2
        B = keys.numel()
        tsdf = torch.empty(B, BLOCK_VOXELS, dtype=torch.float32, device=dev)
        weight = torch.empty(B, BLOCK_VOXELS, dtype=torch.float32, device=dev)
        col = torch.empty(B, BLOCK_VOXELS, 3, dtype=torch.float32, device=dev) if rgb is not None else None
        if B:
            _C.check(L.scorp_tsdf_blocks_integrate(ctypes.byref(views), voxel_length, sdf_trunc, keys.data_ptr(), mask.data_ptr(), B,
                                                   tsdf.data_ptr(), weight.data_ptr(), col.data_ptr() if col is not None else None,
                                                   _C.current_stream_ptr()), "scorp_tsdf_blocks_integrate")
    return BlockVolume(keys, block_coords(keys), mask, tsdf, weight, col, voxel_length)


def block_neighbors(keys):
    """nbr [B, 27] int32 for the ascending keys [B] int64: entry (dx + 1) 9 + (dy + 1) 3 + (dz + 1) is the rank of block
    b + (dx, dy, dz), or -1."""
    B = keys.numel()
    if keys.device.type == "cuda":
        nbr = torch.empty(B, 27, dtype=torch.int32, device=keys.device)
        if B:
            with torch.cuda.device(keys.device):
                _C.check(_C.lib().scorp_tsdf_blocks_neighbors(keys.data_ptr(), B, nbr.data_ptr(), _C.current_stream_ptr()),
                         "scorp_tsdf_blocks_neighbors")
        return nbr
    k = keys.numpy()
    coords = _block_coords_numpy(k)
    nbr = np.full((B, 27), -1, np.int32)
    for n, o in enumerate(np.ndindex(3, 3, 3)):
        c = coords + (np.asarray(o) - 1)
        ok = ((c >= -KEY_BIAS) & (c < KEY_BIAS)).all(-1)
        want = _pack_keys_numpy(np.where(ok[:, None], c, 0))
        pos = np.minimum(np.searchsorted(k, want), max(B - 1, 0))
        nbr[:, n] = np.where(ok & (k[pos] == want), pos, -1)
    return torch.from_numpy(nbr)


def _pad_blocks(a, nbr, lo, hi, fill):
    """a [B, 16, 16, 16, ...] -> [B, n, n, n, ...] over the local range lo .. hi - 1 per axis (lo in (-1, 0), hi in (16, 17)),
    the entries outside 0 .. 15 fetched from the neighbouring blocks, `fill` where there is none."""
    B, n = a.shape[0], hi - lo
    out = np.full((B, n, n, n) + a.shape[4:], fill, a.dtype)
    segs = [(1, slice(0, 16), slice(-lo, 16 - lo))]
    if lo < 0:
        segs.append((0, slice(15, 16), slice(0, 1)))
    if hi > 16:
        segs.append((2, slice(0, 1), slice(16 - lo, 17 - lo)))
    for ox, sx, dx in segs:
        for oy, sy, dy in segs:
            for oz, sz, dz in segs:
                r = nbr[:, ox * 9 + oy * 3 + oz]
                have = np.flatnonzero(r >= 0)
                out[have[:, None, None, None], np.arange(n)[dx][None, :, None, None], np.arange(n)[dy][None, None, :, None],
                    np.arange(n)[dz][None, None, None, :]] = a[r[have]][:, sx, sy, sz]
    return out


def _surface_blocks_numpy(keys, nbr, tsdf, weight, colour, voxel_length):
    """The surface rule of include/scorp_gs.h in vectorised numpy float32: (vertices, faces, colours or None)."""
    f = np.float32
    B = keys.size
    coords = _block_coords_numpy(keys)
    nbr = nbr.copy()
    nbr[:, 13] = np.arange(B)
    shape = (B, 16, 16, 16)
    T = _pad_blocks(tsdf.reshape(shape), nbr, -1, 17, f(0))
    valid = _pad_blocks(weight.reshape(shape), nbr, -1, 17, f(0)) > 0
    inside = T < 0
    Cc = _pad_blocks(colour.reshape(shape + (3,)), nbr, 0, 17, f(0)) if colour is not None else None

    def corner(a, n, base=1):   # the values at corner n of the block's own cells (a padded from local -1: base 1)
        di, dj, dk = base + (n >> 2), base + ((n >> 1) & 1), base + (n & 1)
        return a[:, di:di + 16, dj:dj + 16, dk:dk + 16]
    cell_valid = np.ones((B, 17, 17, 17), bool)   # cells -1 .. 15 at index 0 .. 16
    for n in range(8):
        di, dj, dk = n >> 2, (n >> 1) & 1, n & 1
        cell_valid &= valid[:, di:di + 17, dj:dj + 17, dk:dk + 17]
    s = [np.zeros(shape, f) for _ in range(3)]
    csum = np.zeros(shape + (3,), f) if Cc is not None else None
    cnt = np.zeros(shape, np.int32)
    with np.errstate(all="ignore"):
        for axis in range(3):
            step = 4 >> axis
            for n0 in range(8):
                if n0 & step:
                    continue
                v0, v1 = corner(T, n0), corner(T, n0 + step)
                cross = corner(inside, n0) != corner(inside, n0 + step)
                t = (f(0) - v0) / (v1 - v0)
                fixed = (f(n0 >> 2), f((n0 >> 1) & 1), f(n0 & 1))
                for d in range(3):
                    s[d] += np.where(cross, t if d == axis else fixed[d], f(0)).astype(f)
                if csum is not None:
                    c0, c1 = corner(Cc, n0, 0), corner(Cc, n0 + step, 0)
                    csum += np.where(cross[..., None], c0 + t[..., None] * (c1 - c0), f(0)).astype(f)
                cnt += cross
    active = (cnt > 0) & cell_valid[:, 1:, 1:, 1:]
    ids = (np.cumsum(active.ravel(), dtype=np.int64) - 1).reshape(shape)
    bi, ci, cj, ck = np.nonzero(active)
    n = cnt[active].astype(f)
    verts = np.empty((bi.size, 3), f)
    for d, l in enumerate((ci, cj, ck)):
        g = coords[bi, d] * 16 + l
        verts[:, d] = f(voxel_length) * ((g.astype(f) + f(0.5)) + s[d][active] / n)
    cols = (csum[active] / n[:, None] / f(255)).astype(f) if csum is not None else None
    ids = _pad_blocks(np.where(active, ids, -1), nbr, -1, 16, -1)   # cells -1 .. 15 at index 0 .. 16
    E = np.zeros(shape + (3,), bool)
    own = lambda a, off=(0, 0, 0): a[:, 1 + off[0]:17 + off[0], 1 + off[1]:17 + off[1], 1 + off[2]:17 + off[2]]
    eye = np.eye(3, dtype=np.int64)
    for a in range(3):
        b, c = eye[(a + 1) % 3], eye[(a + 2) % 3]
        ok = own(inside) != own(inside, eye[a])
        for off in (0 * b, -b, -b - c, -c):
            ok = ok & own(cell_valid, off)
        E[..., a] = ok
    qb, qi, qj, qk, qa = np.nonzero(E)
    q = np.stack([qi, qj, qk], 1) + 1   # into the arrays padded from -1
    b, c = eye[(qa + 1) % 3], eye[(qa + 2) % 3]
    cell = lambda p: ids[qb, p[:, 0], p[:, 1], p[:, 2]]
    c00, c10, c11, c01 = cell(q), cell(q - b), cell(q - b - c), cell(q - c)
    qin = inside[qb, q[:, 0], q[:, 1], q[:, 2]]
    faces = np.stack([c00, np.where(qin, c10, c11), np.where(qin, c11, c10),
                      c00, np.where(qin, c11, c01), np.where(qin, c01, c11)], 1).reshape(-1, 3).astype(np.int32)
    return verts, faces, cols


def _marching_cubes_blocks_numpy(keys, nbr, tsdf, weight, colour, voxel_length):
    """The marching-cubes surface rule of include/scorp_gs.h in vectorised numpy float32: (vertices, faces, colours or None)."""
    f = np.float32
    B = keys.size
    coords = _block_coords_numpy(keys)
    nbr = nbr.copy()
    nbr[:, 13] = np.arange(B)
    shape = (B, 16, 16, 16)
    T = _pad_blocks(tsdf.reshape(shape), nbr, -1, 17, f(0))          # local -1 .. 16 at index 0 .. 17
    valid = _pad_blocks(weight.reshape(shape), nbr, -1, 17, f(0)) > 0
    inside = (T < 0) & valid
    cell_valid = np.ones((B, 17, 17, 17), bool)                      # cells -1 .. 15 at index 0 .. 16
    for n in range(8):
        di, dj, dk = n >> 2, (n >> 1) & 1, n & 1
        cell_valid &= valid[:, di:di + 17, dj:dj + 17, dk:dk + 17]
    own = lambda a, off=(0, 0, 0): a[:, 1 + off[0]:17 + off[0], 1 + off[1]:17 + off[1], 1 + off[2]:17 + off[2]]
    eye = np.eye(3, dtype=np.int64)
    E = np.zeros(shape + (3,), bool)
    for a in range(3):
        b, c = eye[(a + 1) % 3], eye[(a + 2) % 3]
        some = np.zeros(shape, bool)
        for off in (0 * b, -b, -b - c, -c):
            some |= own(cell_valid, off)
        E[..., a] = (own(inside) != own(inside, eye[a])) & some
    vid = (np.cumsum(E.ravel(), dtype=np.int64) - 1).reshape(E.shape)   # ascending (block rank, local q, axis)
    qb, qi, qj, qk, qa = np.nonzero(E)
    q = np.stack([qi, qj, qk], 1)
    q1 = q + eye[qa]
    f0, f1 = T[qb, q[:, 0] + 1, q[:, 1] + 1, q[:, 2] + 1], T[qb, q1[:, 0] + 1, q1[:, 1] + 1, q1[:, 2] + 1]
    with np.errstate(all="ignore"):
        t = (f(0) - f0) / (f1 - f0)
    verts = np.empty((qb.size, 3), f)
    for d in range(3):
        g = (coords[qb, d] * 16 + q[:, d]).astype(f) + f(0.5)
        verts[:, d] = f(voxel_length) * np.where(qa == d, g + t, g)
    cols = None
    if colour is not None:
        Cc = _pad_blocks(colour.reshape(shape + (3,)), nbr, 0, 17, f(0))
        c0, c1 = Cc[qb, q[:, 0], q[:, 1], q[:, 2]], Cc[qb, q1[:, 0], q1[:, 1], q1[:, 2]]
        cols = ((c0 + t[:, None] * (c1 - c0)) / f(255)).astype(f)
    case = np.zeros(shape, np.int64)
    for n in range(8):
        case |= own(inside, (n >> 2, (n >> 1) & 1, n & 1)).astype(np.int64) << n
    vid = _pad_blocks(np.where(E, vid, -1), nbr, 0, 17, -1)          # local 0 .. 16: the edges of the cells' far corners
    return verts, _mc_faces_numpy(case, cell_valid[:, 1:, 1:, 1:], vid, mc_table.cached_table()), cols


def _marching_cubes_blocks_gpu(keys, nbr, tsdf, weight, colour, voxel_length, empty):
    L = _C.lib()
    dev = tsdf.device
    B = keys.numel()
    with torch.cuda.device(dev):
        stream = _C.current_stream_ptr()
        masks = torch.empty(B * BLOCK_VOXELS, dtype=torch.uint8, device=dev)
        counts = torch.empty(B * BLOCK_VOXELS, dtype=torch.uint8, device=dev)
        _C.check(L.scorp_marching_cubes_blocks_count_edges(tsdf.data_ptr(), weight.data_ptr(), nbr.data_ptr(), B, masks.data_ptr(),
                                                           counts.data_ptr(), stream), "scorp_marching_cubes_blocks_count_edges")
        nv, edge_scan = _scan_counts(counts, 2 ** 31, "vertices")
        if nv == 0:
            return empty
        verts = torch.empty(nv, 3, dtype=torch.float32, device=dev)
        cols = torch.empty(nv, 3, dtype=torch.float32, device=dev) if colour is not None else None
        _C.check(L.scorp_marching_cubes_blocks_emit_vertices(tsdf.data_ptr(), weight.data_ptr(),
                                                             colour.data_ptr() if colour is not None else None, keys.data_ptr(),
                                                             nbr.data_ptr(), B, voxel_length, masks.data_ptr(), edge_scan.data_ptr(), nv,
                                                             verts.data_ptr(), cols.data_ptr() if cols is not None else None, stream),
                 "scorp_marching_cubes_blocks_emit_vertices")
        if cols is None:
            cols = torch.zeros(nv, 3, dtype=torch.float32, device=dev)
        _C.check(L.scorp_marching_cubes_blocks_count_faces(tsdf.data_ptr(), weight.data_ptr(), nbr.data_ptr(), B, counts.data_ptr(), stream),
                 "scorp_marching_cubes_blocks_count_faces")
        nf, face_scan = _scan_counts(counts, 2 ** 31, "triangles")
        faces = torch.empty(nf, 3, dtype=torch.int32, device=dev)
        if nf:
            _C.check(L.scorp_marching_cubes_blocks_emit_faces(tsdf.data_ptr(), weight.data_ptr(), nbr.data_ptr(), B, masks.data_ptr(),
                                                              edge_scan.data_ptr(), face_scan.data_ptr(), nf, faces.data_ptr(), stream),
                     "scorp_marching_cubes_blocks_emit_faces")
    return Mesh(verts, faces, cols)


def _surface_nets_blocks_gpu(keys, nbr, tsdf, weight, colour, voxel_length, empty):
    L = _C.lib()
    dev = tsdf.device
    B = keys.numel()
    with torch.cuda.device(dev):
        stream = _C.current_stream_ptr()
        flags = torch.empty(B * BLOCK_VOXELS, dtype=torch.uint8, device=dev)
        _C.check(L.scorp_isosurface_blocks_count_cells(tsdf.data_ptr(), weight.data_ptr(), nbr.data_ptr(), B, flags.data_ptr(), stream),
                 "scorp_isosurface_blocks_count_cells")
        nv, cell_scan = _scan_counts(flags, 2 ** 31, "vertices")
        if nv == 0:
            return empty
        verts = torch.empty(nv, 3, dtype=torch.float32, device=dev)
        cols = torch.empty(nv, 3, dtype=torch.float32, device=dev) if colour is not None else None
        _C.check(L.scorp_isosurface_blocks_emit_vertices(tsdf.data_ptr(), weight.data_ptr(), colour.data_ptr() if colour is not None else None,
                                                         keys.data_ptr(), nbr.data_ptr(), B, voxel_length, cell_scan.data_ptr(), nv,
                                                         verts.data_ptr(), cols.data_ptr() if cols is not None else None, stream),
                 "scorp_isosurface_blocks_emit_vertices")
        if cols is None:
            cols = torch.zeros(nv, 3, dtype=torch.float32, device=dev)
        counts = torch.empty(B * BLOCK_VOXELS, dtype=torch.uint8, device=dev)
        _C.check(L.scorp_isosurface_blocks_count_faces(tsdf.data_ptr(), weight.data_ptr(), nbr.data_ptr(), B, counts.data_ptr(), stream),
                 "scorp_isosurface_blocks_count_faces")
        nq, edge_scan = _scan_counts(counts, 2 ** 30, "triangles")   # (two triangles per quad)
        faces = torch.empty(2 * nq, 3, dtype=torch.int32, device=dev)
        if nq:
            _C.check(L.scorp_isosurface_blocks_emit_faces(tsdf.data_ptr(), weight.data_ptr(), nbr.data_ptr(), B, cell_scan.data_ptr(),
                                                          edge_scan.data_ptr(), nq, faces.data_ptr(), stream),
                     "scorp_isosurface_blocks_emit_faces")
    return Mesh(verts, faces, cols)


def extract_surface_blocks(volume, method="surface_nets"):
    """The zero surface of a BlockVolume through the block borders (include/scorp_gs.h): a Mesh on the volume's device, colours
    in [0, 1] (zeros for a volume without colour).  method "surface_nets": vertices in ascending (block, local cell index);
    cells with a corner no view has written, or in a block that does not exist, carry no vertex and no face.
    "marching_cubes": one vertex per crossed lattice edge that has a valid cell round it, in ascending (block, local index of
    the edge's first point, axis); only valid cells emit triangles."""
    _check_method(method)
    keys, tsdf, weight, colour = volume.keys, volume.tsdf, volume.weight, volume.colour
    dev = tsdf.device
    B = keys.numel()
    empty = Mesh(torch.empty(0, 3, dtype=torch.float32, device=dev), torch.empty(0, 3, dtype=torch.int32, device=dev),
                 torch.empty(0, 3, dtype=torch.float32, device=dev))
    if B == 0:
        return empty
    if tuple(tsdf.shape) != (B, BLOCK_VOXELS) or tuple(weight.shape) != (B, BLOCK_VOXELS) or \
            (colour is not None and tuple(colour.shape) != (B, BLOCK_VOXELS, 3)):
        raise ValueError(f"tsdf and weight must be [{B}, 4096] and colour [{B}, 4096, 3]")
    keys = keys.to(torch.int64).contiguous()
    tsdf, weight = tsdf.to(torch.float32).contiguous(), weight.to(torch.float32).contiguous()
    colour = colour.to(torch.float32).contiguous() if colour is not None else None
    voxel_length = float(np.float32(volume.voxel_length))
    nbr = block_neighbors(keys)
    if dev.type != "cuda":
        form = _marching_cubes_blocks_numpy if method == "marching_cubes" else _surface_blocks_numpy
        v, t, c = form(keys.numpy(), nbr.numpy(), tsdf.numpy(), weight.numpy(), colour.numpy() if colour is not None else None, voxel_length)
        return Mesh(torch.from_numpy(v), torch.from_numpy(t), torch.from_numpy(c) if c is not None else torch.zeros(v.shape[0], 3))
    form = _marching_cubes_blocks_gpu if method == "marching_cubes" else _surface_nets_blocks_gpu
    return form(keys, nbr, tsdf, weight, colour, voxel_length, empty)


# ---- triangle clustering and floater removal ----

MAX_CLUSTER_FACES = 1 << 28   # the C ABI's bound (include/scorp_gs.h)
MIN_CLUSTER_TRIANGLES = 50    # mesh_utils.py:36: no cluster below it is ever kept


def _triangle_areas_numpy(f, v):
    """0.5 |(v1 - v0) x (v2 - v0)| in float64 from the float32 vertices, every product and sum rounded on its own."""
    v = np.asarray(v, np.float32).astype(np.float64)
    u, w = v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]
    nx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
    ny = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
    nz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    return 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)


def _cluster_numpy(f, verts):
    """The rules of include/scorp_gs.h (connected triangles) in numpy: the 3F edge keys grouped by np.unique, then every
    triangle takes the smallest label on its edges and the labels are pointer-jumped, until nothing changes.  A label is
    always a triangle of the same component, so the fixed point is the component's smallest triangle index."""
    F = f.shape[0]
    f = f.astype(np.int64)
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)                     # edge e of triangle t at 3 t + e
    _, edge = np.unique(np.minimum(a, b) << 32 | np.maximum(a, b), return_inverse=True)
    edge = edge.reshape(-1)
    order = np.argsort(edge, kind="stable")
    tri = order // 3                                                        # the triangles edge by edge
    starts = np.flatnonzero(np.diff(edge[order], prepend=-1))
    label = np.arange(F, dtype=np.int64)
    while True:
        edge_min = np.minimum.reduceat(label[tri], starts)
        new = np.minimum(label, edge_min[edge].reshape(F, 3).min(1))
        while True:
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, label):
            break
        label = new
    is_root = label == np.arange(F)
    cluster = (np.cumsum(is_root) - 1)[label].astype(np.int32)
    C = int(is_root.sum())
    counts = np.bincount(cluster, minlength=C).astype(np.int32)
    area = np.bincount(cluster, weights=_triangle_areas_numpy(f, verts), minlength=C) if verts is not None else None
    return cluster, counts, area


def cluster_connected_triangles(faces, vertices=None):
    """Open3D's TriangleMesh.cluster_connected_triangles on faces [F, 3] (integer vertex indices): (triangle_clusters [F]
    int32, cluster_n_triangles [C] int32, cluster_area [C] float64 - None without `vertices` [Nv, 3]) on faces' device.
    Triangles are adjacent when they share an edge (a pair of vertex indices); clusters are numbered by their smallest
    triangle index (include/scorp_gs.h).  CUDA tensors run csrc/mesh_cluster.hip, CPU tensors a numpy form of the same rules."""
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype.is_floating_point \
            or faces.dtype.is_complex or faces.dtype == torch.bool:
        raise ValueError("faces must be an integer tensor [F, 3]")
    dev = faces.device
    F = faces.shape[0]
    if F > MAX_CLUSTER_FACES:
        raise ValueError(f"more than 2^28 triangles: {F}")
    if vertices is not None:
        if not isinstance(vertices, torch.Tensor) or vertices.dim() != 2 or vertices.shape[1] != 3:
            raise ValueError("vertices must be [Nv, 3]")
        vertices = vertices.to(device=dev, dtype=torch.float32).contiguous()
    if F == 0:
        return (torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                torch.empty(0, dtype=torch.float64, device=dev) if vertices is not None else None)
    lo, hi = int(faces.min()), int(faces.max())
    if lo < 0:
        raise ValueError(f"negative vertex index {lo}")
    if hi > 2 ** 31 - 1:
        raise ValueError(f"vertex index {hi} above 2^31 - 1")
    if vertices is not None and hi >= vertices.shape[0]:
        raise ValueError(f"vertex index {hi} with {vertices.shape[0]} vertices")
    faces = faces.to(torch.int32).contiguous()
    if dev.type != "cuda":
        cluster, counts, area = _cluster_numpy(faces.numpy(), vertices.numpy() if vertices is not None else None)
        return torch.from_numpy(cluster), torch.from_numpy(counts), torch.from_numpy(area) if area is not None else None
    L = _C.lib()
    slots = 1 << (6 * F - 1).bit_length()   # the power of two >= 6 F
    with torch.cuda.device(dev):
        stream = _C.current_stream_ptr()
        keys = torch.empty(slots, dtype=torch.int64, device=dev)
        owner = torch.empty(slots, dtype=torch.int32, device=dev)
        parent = torch.empty(F, dtype=torch.int32, device=dev)
        _C.check(L.scorp_mesh_cluster_link(faces.data_ptr(), F, keys.data_ptr(), owner.data_ptr(), slots, parent.data_ptr(), stream),
                 "scorp_mesh_cluster_link")
        del keys, owner
        root = torch.empty(F, dtype=torch.int32, device=dev)
        is_root = torch.empty(F, dtype=torch.uint8, device=dev)
        _C.check(L.scorp_mesh_cluster_roots(parent.data_ptr(), F, root.data_ptr(), is_root.data_ptr(), stream), "scorp_mesh_cluster_roots")
        root_scan = torch.cumsum(is_root, 0, dtype=torch.int32)
        C = int(root_scan[-1])
        cluster = torch.empty(F, dtype=torch.int32, device=dev)
        counts = torch.empty(C, dtype=torch.int32, device=dev)
        area = torch.empty(C, dtype=torch.float64, device=dev) if vertices is not None else None
        _C.check(L.scorp_mesh_cluster_stats(faces.data_ptr(), vertices.data_ptr() if vertices is not None else None,
                                            vertices.shape[0] if vertices is not None else 0, root.data_ptr(), root_scan.data_ptr(),
                                            F, C, cluster.data_ptr(), counts.data_ptr(),
                                            area.data_ptr() if area is not None else None, stream), "scorp_mesh_cluster_stats")
    return cluster, counts, area


def post_process_mesh(mesh, cluster_to_keep=1000):
    """mesh_utils.py:22-43, statement for statement, on the mesh's device: cluster the triangles, n = the size of the
    `cluster_to_keep`-th largest cluster (ties keep every cluster of that size) and at least 50, drop the triangles of
    smaller clusters, drop the vertices no remaining triangle references (survivors keep their order, colours travel with
    them, faces are re-indexed), last drop the triangles with two equal indices.  Returns a new Mesh.

    Departure from the reference: with fewer than `cluster_to_keep` clusters its negative index raises IndexError; here the
    smallest cluster's size stands in, so every cluster of at least 50 triangles is kept."""
    cluster_to_keep = int(cluster_to_keep)
    if cluster_to_keep < 1:
        raise ValueError(f"cluster_to_keep must be at least 1; got {cluster_to_keep}")
    verts, faces, colors = mesh.vertices, mesh.faces, mesh.colors
    dev = faces.device
    Nv = verts.shape[0]
    if colors.shape[0] != Nv:
        raise ValueError(f"{colors.shape[0]} colours for {Nv} vertices")
    if faces.shape[0] == 0:
        return Mesh(torch.empty(0, 3, dtype=torch.float32, device=dev), torch.empty(0, 3, dtype=torch.int32, device=dev),
                    torch.empty(0, 3, dtype=torch.float32, device=dev))
    if int(faces.max()) >= Nv:
        raise ValueError(f"vertex index {int(faces.max())} with {Nv} vertices")
    triangle_clusters, cluster_n_triangles, _ = cluster_connected_triangles(faces)
    C = cluster_n_triangles.numel()
    n = torch.sort(cluster_n_triangles)[0][C - min(cluster_to_keep, C)].clamp(min=MIN_CLUSTER_TRIANGLES)
    faces = faces[cluster_n_triangles[triangle_clusters.long()] >= n].long()
    used = torch.zeros(Nv, dtype=torch.bool, device=dev)
    used[faces.reshape(-1)] = True
    new_index = torch.cumsum(used, 0, dtype=torch.int32) - 1
    faces = new_index[faces]
    faces = faces[(faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 2] != faces[:, 0])]
    return Mesh(verts[used].to(torch.float32), faces.to(torch.int32).contiguous(), colors[used].to(torch.float32))


# ---- simplification by vertex clustering (the rules are in include/scorp_gs.h) ----

CONTRACTIONS = ("average", "quadric")
CELL_SIDE = 1 << 21             # cell indices per axis: three pack into one 63-bit key
MAX_SIMPLIFY_VERTICES = 1 << 30   # the C ABI's bound
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
        p0 = v[f64[:, 0]]
        u, w = v[f64[:, 1]] - p0, v[f64[:, 2]] - p0
        N = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], 1)
        length = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
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
    t = t[(t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 2] != t[:, 0])]
    t = np.take_along_axis(t, (np.argmin(t, 1)[:, None] + np.arange(3)[None]) % 3, 1)
    if t.shape[0]:
        _, keep = np.unique(t, axis=0, return_index=True)   # the first (smallest-index) face of every ordered triple
        t = t[np.sort(keep)]
    return cell.astype(np.int32), positions, colours, t.astype(np.int32).reshape(-1, 3)


def _simplify_gpu(verts, colors, faces, lo, h, quadric):
    L = _C.lib()
    dev = verts.device
    Nv, F = verts.shape[0], faces.shape[0]
    i32 = partial(torch.empty, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = _C.current_stream_ptr()
        slots = 1 << (2 * Nv - 1).bit_length()   # the power of two >= 2 Nv
        keys = torch.empty(slots, dtype=torch.int64, device=dev)
        owner, slot, overflow = i32(slots), i32(Nv), i32(1)
        _C.check(L.scorp_mesh_simplify_cells(verts.data_ptr(), Nv, lo.data_ptr(), h, keys.data_ptr(), owner.data_ptr(), slots,
                                             slot.data_ptr(), overflow.data_ptr(), stream), "scorp_mesh_simplify_cells")
        rep = i32(Nv)
        is_root = torch.empty(Nv, dtype=torch.uint8, device=dev)
        _C.check(L.scorp_mesh_simplify_roots(owner.data_ptr(), slots, slot.data_ptr(), Nv, rep.data_ptr(), is_root.data_ptr(), stream),
                 "scorp_mesh_simplify_roots")
        del keys, owner, slot
        rep_scan = torch.cumsum(is_root, 0, dtype=torch.int32)
        C = int(rep_scan[-1])
        if int(overflow):   # (the extent was checked on the host: this does not happen)
            raise ValueError("a vertex lies outside the grid of 2^21 cells per axis")
        vertex_cell, cell_ijk = i32(Nv), i32(C, 3)
        acc = torch.empty(C, 16, dtype=torch.float64, device=dev)
        _C.check(L.scorp_mesh_simplify_accumulate(verts.data_ptr(), colors.data_ptr(), Nv, faces.data_ptr(), F, lo.data_ptr(), h,
                                                  rep.data_ptr(), rep_scan.data_ptr(), C, quadric, vertex_cell.data_ptr(),
                                                  cell_ijk.data_ptr(), acc.data_ptr(), stream), "scorp_mesh_simplify_accumulate")
        positions = torch.empty(C, 3, dtype=torch.float32, device=dev)
        colours = torch.empty(C, 3, dtype=torch.float32, device=dev)
        _C.check(L.scorp_mesh_simplify_place(acc.data_ptr(), cell_ijk.data_ptr(), C, lo.data_ptr(), h, quadric, positions.data_ptr(),
                                             colours.data_ptr(), stream), "scorp_mesh_simplify_place")
        slots = 1 << (2 * F - 1).bit_length()
        table, rotated = i32(slots), i32(F, 3)
        keep = torch.empty(F, dtype=torch.uint8, device=dev)
        _C.check(L.scorp_mesh_simplify_faces(faces.data_ptr(), F, vertex_cell.data_ptr(), Nv, table.data_ptr(), slots, rotated.data_ptr(),
                                             keep.data_ptr(), stream), "scorp_mesh_simplify_faces")
        return vertex_cell, positions, colours, rotated[keep.bool()]


def _empty_mesh(dev):
    return Mesh(torch.empty(0, 3, dtype=torch.float32, device=dev), torch.empty(0, 3, dtype=torch.int32, device=dev),
                torch.empty(0, 3, dtype=torch.float32, device=dev))


def cluster_vertices(mesh, voxel_size, contraction="average"):
    """The clustering behind simplify_vertex_clustering with its vertex map: (vertex_cell [Nv] int32, Mesh) - vertex_cell[v] is
    the output vertex that input vertex v went to, and the Mesh keeps every cell's vertex, referenced or not.  An empty mesh
    (no vertices or no faces) gives an empty map and an empty Mesh."""
    verts, faces, colors = mesh.vertices, mesh.faces, mesh.colors
    if contraction not in CONTRACTIONS:
        raise ValueError(f"contraction must be one of {CONTRACTIONS}; got {contraction!r}")
    h = float(voxel_size)
    if not (h > 0.0 and np.isfinite(h)):
        raise ValueError(f"voxel_size must be positive and finite; got {voxel_size}")
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype.is_floating_point:
        raise ValueError("vertices must be [Nv, 3] and faces an integer tensor [F, 3]")
    dev = verts.device
    Nv, F = verts.shape[0], faces.shape[0]
    if colors.dim() != 2 or tuple(colors.shape) != (Nv, 3):
        raise ValueError(f"{colors.shape[0]} colours for {Nv} vertices")
    if Nv > MAX_SIMPLIFY_VERTICES or F > MAX_CLUSTER_FACES:
        raise ValueError(f"more than 2^30 vertices or 2^28 triangles: {Nv}, {F}")
    if F == 0 or Nv == 0:
        return torch.empty(0, dtype=torch.int32, device=dev), _empty_mesh(dev)
    verts = verts.to(torch.float32).contiguous()
    colors = colors.to(device=dev, dtype=torch.float32).contiguous()
    lo, hi = verts.amin(0), verts.amax(0)
    ends = torch.stack([lo, hi]).cpu().numpy().astype(np.float64)
    if not np.isfinite(ends).all():   # (a NaN or an infinity anywhere reaches the minimum or the maximum)
        raise ValueError("the vertices are not all finite")
    origin = ends[0] - 0.5 * h
    if not (np.floor((ends[1] - origin) / h) < CELL_SIDE).all():
        raise ValueError(f"an extent of {tuple((ends[1] - ends[0]).tolist())} at voxel_size {h} needs more than 2^21 cells on an axis")
    fmin, fmax = int(faces.min()), int(faces.max())
    if fmin < 0 or fmax >= Nv:
        raise ValueError(f"vertex index {fmin if fmin < 0 else fmax} with {Nv} vertices")
    faces = faces.to(device=dev, dtype=torch.int32).contiguous()
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
    used = torch.zeros(out.vertices.shape[0], dtype=torch.bool, device=out.vertices.device)
    used[out.faces.reshape(-1).long()] = True
    faces = (torch.cumsum(used, 0, dtype=torch.int32) - 1)[out.faces.long()]
    return Mesh(out.vertices[used], faces.contiguous(), out.colors[used])


# ---- edge-collapse decimation to a target triangle count (the rules are in include/scorp_gs.h) ----

DECIMATE_DET_FLOOR = 1e-9    # rule 4: the 3x3 solve is taken iff det > this ((t t) t), t the trace
DECIMATE_REACH = 4.0         # ... and |x - mid|^2 <= this |P[hi] - P[lo]|^2
_M64 = (1 << 64) - 1


def _splitmix(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def _dot3(u, w):
    return (u[..., 0] * w[..., 0] + u[..., 1] * w[..., 1]) + u[..., 2] * w[..., 2]


def _cross3(u, w):
    return np.stack([u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1], u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2],
                     u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]], -1)


def _plane_quadric(n, d, w):
    wn, wd = w * n, w * d
    return np.array([wn[0] * n[0], wn[0] * n[1], wn[0] * n[2], wn[1] * n[1], wn[1] * n[2], wn[2] * n[2], wd * n[0], wd * n[1], wd * n[2], wd * d])


def _quadric_cost(q, x):
    s2 = (q[..., 0] * (x[..., 0] * x[..., 0]) + q[..., 3] * (x[..., 1] * x[..., 1])) + q[..., 5] * (x[..., 2] * x[..., 2])
    s1 = (q[..., 1] * (x[..., 0] * x[..., 1]) + q[..., 2] * (x[..., 0] * x[..., 2])) + q[..., 4] * (x[..., 1] * x[..., 2])
    s0 = (q[..., 6] * x[..., 0] + q[..., 7] * x[..., 1]) + q[..., 8] * x[..., 2]
    c = ((s2 + 2.0 * s1) + 2.0 * s0) + q[..., 9]
    return np.where(c > 0.0, c, 0.0)


def _quadric_place(q, plo, phi):
    """rule 4 for rows of summed quadrics [E, 10] and their ends' positions [E, 3]: (x [E, 3], cost [E])"""
    a00, a01, a02, a11, a12, a22, b0, b1, b2 = (q[:, k] for k in range(9))
    c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
    c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
    det = (a00 * c00 + a01 * c01) + a02 * c02
    t = (a00 + a11) + a22
    mid = 0.5 * (plo + phi)
    x = np.stack([-((c00 * b0 + c01 * b1) + c02 * b2) / det, -((c01 * b0 + c11 * b1) + c12 * b2) / det,
                  -((c02 * b0 + c12 * b1) + c22 * b2) / det], 1)
    dx, de = x - mid, phi - plo
    solved = (det > DECIMATE_DET_FLOOR * ((t * t) * t)) & (_dot3(dx, dx) <= DECIMATE_REACH * _dot3(de, de))   # (false for NaN)
    best, best_cost = plo, _quadric_cost(q, plo)
    for p in (phi, mid):                                          # ties stay with the earlier of lo, hi, mid
        c = _quadric_cost(q, p)
        better = c < best_cost
        best, best_cost = np.where(better[:, None], p, best), np.where(better, c, best_cost)
    return np.where(solved[:, None], x, best), np.where(solved, _quadric_cost(q, x), best_cost)


class _DecimateNumpy:
    """The seven calls of csrc/mesh_decimate.hip in Python over numpy views of CPU tensors, loop for thread: the same
    arrays go in and come out, so _decimate runs either.  For small meshes; correctness is its only duty."""

    def quadrics(self, P, faces, face_edge, edge_faces, vf_start, vf_face, bw, Q):
        P, f, fe, ef, start, vf, Q = (a.numpy() for a in (P, faces, face_edge, edge_faces, vf_start, vf_face, Q))
        with np.errstate(all="ignore"):
            for v in range(P.shape[0]):
                q = np.zeros(10)
                for t in vf[start[v]:start[v + 1]]:
                    i = f[t]
                    p = P[i]
                    N = _cross3(p[1] - p[0], p[2] - p[0])
                    length = np.sqrt(_dot3(N, N))
                    if not length > 0.0:
                        continue
                    n = N / length
                    q += _plane_quadric(n, -_dot3(n, p[0]), 0.5 * length)
                    for k in range(3):
                        a, b = k, (k + 1) % 3
                        if (i[a] != v and i[b] != v) or ef[fe[t, k]] != 1:
                            continue
                        e = p[b] - p[a]
                        M = _cross3(e, n)
                        ml = np.sqrt(_dot3(M, M))
                        if not ml > 0.0:
                            continue
                        m = M / ml
                        q += _plane_quadric(m, -_dot3(m, p[a]), bw * _dot3(e, e))
                Q[v] = q

    def flags(self, keys, edge_faces, flags):
        k, ef, fl = keys.numpy(), edge_faces.numpy(), flags.numpy()
        fl[:] = 0
        bits = (ef == 1) * 1 + (ef >= 3) * 2
        for ends in (k >> 32, k & 0xFFFFFFFF):
            np.bitwise_or.at(fl, ends, bits.astype(np.int32))

    def candidates(self, P, Q, faces, keys, edge_faces, vf_start, vf_face, flags, max_err, cost, x):
        P, Q, f, k, ef, start, vf, fl, cost, x = (a.numpy() for a in (P, Q, faces, keys, edge_faces, vf_start, vf_face, flags, cost, x))
        cost[:] = np.inf
        with np.errstate(all="ignore"):
            los, his = k >> 32, k & 0xFFFFFFFF
            x[:], costs = _quadric_place(Q[los] + Q[his], P[los], P[his])
            for e in range(k.shape[0]):
                lo, hi, n, xe, c = int(los[e]), int(his[e]), int(ef[e]), x[e], costs[e]
                if n > 2 or (fl[lo] | fl[hi]) & 2 or (n == 2 and fl[lo] & 1 and fl[hi] & 1) or not c <= max_err:
                    continue
                of_lo, of_hi = f[vf[start[lo]:start[lo + 1]]], f[vf[start[hi]:start[hi + 1]]]
                both = (of_lo == hi).any(1)
                apexes = of_lo[both][(of_lo[both] != lo) & (of_lo[both] != hi)]
                if len(apexes) != n or len(set(apexes.tolist())) != n:
                    continue
                ring = of_lo[~both]                                   # the faces with lo alone: no vertex next to hi but an apex
                among = lambda a, b: (a[..., None] == b.reshape(-1)).any(-1)
                if (among(ring, of_hi) & (ring != lo) & ~among(ring, apexes)).any():
                    continue
                tri = np.concatenate([ring, of_hi[~(of_hi == lo).any(1)]])   # rule 5 over the faces with one end
                moved = np.concatenate([np.full(len(ring), lo), np.full(len(tri) - len(ring), hi)])
                p = P[tri]
                q = np.where((tri == moved[:, None])[..., None], xe, p)
                if (_dot3(_cross3(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), _cross3(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0])) > 0.0).all():
                    cost[e] = c

    def hash(self, keys, window, rnd, out):
        k, mr = keys.numpy(), _splitmix(rnd)
        out.numpy()[:] = [_splitmix(int(k[e]) ^ mr) >> 1 for e in window.numpy()]

    def select(self, keys, ranked, vmin, vmin2, selected):
        k, rk, vmin, vmin2, sel = (a.numpy() for a in (keys, ranked, vmin, vmin2, selected))
        lo, hi = k >> 32, k & 0xFFFFFFFF
        vmin[:] = 2 ** 31 - 1
        rank = np.arange(rk.shape[0], dtype=np.int32)
        np.minimum.at(vmin, lo[rk], rank)
        np.minimum.at(vmin, hi[rk], rank)
        vmin2[:] = vmin
        np.minimum.at(vmin2, lo, vmin[hi])
        np.minimum.at(vmin2, hi, vmin[lo])
        sel[:] = (vmin2[lo[rk]] == rank) & (vmin2[hi[rk]] == rank)

    def apply(self, keys, ranked, applied, x, P, Q, C, count, vmap):
        k, rk, ap, x, P, Q, C, count, vmap = (a.numpy() for a in (keys, ranked, applied, x, P, Q, C, count, vmap))
        vmap[:] = np.arange(vmap.shape[0])
        for r in np.flatnonzero(ap):
            e = rk[r]
            lo, hi = int(k[e] >> 32), int(k[e] & 0xFFFFFFFF)
            P[lo] = x[e]
            Q[lo] = Q[lo] + Q[hi]
            nl, nh = float(count[lo]), float(count[hi])
            C[lo] = (nl * C[lo] + nh * C[hi]) / (nl + nh)
            count[lo] += count[hi]
            vmap[hi] = lo

    def faces(self, faces, vmap, out_faces, keep):
        m = vmap.numpy()[faces.numpy()]
        out_faces.numpy()[:] = m
        keep.numpy()[:] = (m[:, 0] != m[:, 1]) & (m[:, 1] != m[:, 2]) & (m[:, 2] != m[:, 0])


class _DecimateHip:
    """The seven entry points of csrc/mesh_decimate.hip on the current stream"""

    def __init__(self):
        self.L = _C.lib()
        self.stream = _C.current_stream_ptr()

    def _call(self, name, *args):
        _C.check(getattr(self.L, name)(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args], self.stream), name)

    def quadrics(self, P, faces, face_edge, edge_faces, vf_start, vf_face, bw, Q):
        self._call("scorp_mesh_decimate_quadrics", P, P.shape[0], faces, faces.shape[0], face_edge, edge_faces, edge_faces.shape[0],
                   vf_start, vf_face, bw, Q)

    def flags(self, keys, edge_faces, flags):
        self._call("scorp_mesh_decimate_flags", keys, edge_faces, keys.shape[0], flags.shape[0], flags)

    def candidates(self, P, Q, faces, keys, edge_faces, vf_start, vf_face, flags, max_err, cost, x):
        self._call("scorp_mesh_decimate_candidates", P, Q, P.shape[0], faces, faces.shape[0], keys, edge_faces, keys.shape[0], vf_start,
                   vf_face, flags, max_err, cost, x)

    def hash(self, keys, window, rnd, out):
        self._call("scorp_mesh_decimate_hash", keys, keys.shape[0], window, window.shape[0], rnd, out)

    def select(self, keys, ranked, vmin, vmin2, selected):
        self._call("scorp_mesh_decimate_select", keys, keys.shape[0], ranked, ranked.shape[0], vmin.shape[0], vmin, vmin2, selected)

    def apply(self, keys, ranked, applied, x, P, Q, C, count, vmap):
        self._call("scorp_mesh_decimate_apply", keys, keys.shape[0], ranked, applied, ranked.shape[0], x, P.shape[0], P, Q, C, count, vmap)

    def faces(self, faces, vmap, out_faces, keep):
        self._call("scorp_mesh_decimate_faces", faces, faces.shape[0], vmap, vmap.shape[0], out_faces, keep)


def _decimate_tables(faces, Nv):
    """One `unique` and one stable sort over the current faces: (edge_keys [E] int64 ascending, face_edge [F, 3] int32,
    edge_faces [E] int32, vf_start [Nv + 1] int32, vf_face [3 F] int32)."""
    f = faces.long()
    a, b = f, f.roll(-1, 1)
    keys, inverse, counts = torch.unique((torch.minimum(a, b) << 32 | torch.maximum(a, b)).reshape(-1), return_inverse=True, return_counts=True)
    order = torch.sort(f.reshape(-1), stable=True)[1]          # (stable: a vertex's faces in ascending index)
    start = torch.zeros(Nv + 1, dtype=torch.int32, device=faces.device)
    start[1:] = torch.cumsum(torch.bincount(f.reshape(-1), minlength=Nv), 0)
    return keys, inverse.reshape(-1, 3).to(torch.int32).contiguous(), counts.to(torch.int32), start, (order // 3).to(torch.int32)


def _decimate(verts, colors, faces, target, max_err, bw, ops, rounds=None):
    """Rules 0 - 11 on tensors of one device; `ops` runs the seven calls.  rounds (a list) receives (faces, edges, window,
    applied faces) of every round."""
    dev, Nv = verts.device, verts.shape[0]
    new = partial(torch.empty, device=dev)
    origin = verts.amin(0).double()
    P = (verts.double() - origin).contiguous()
    C = colors.double().contiguous()
    count = torch.ones(Nv, dtype=torch.int32, device=dev)
    faces = faces[(faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 2] != faces[:, 0])].contiguous()
    Q = new(Nv, 10, dtype=torch.float64)
    flags, vmin, vmin2, vmap = (new(Nv, dtype=torch.int32) for _ in range(4))
    rnd = 0
    while faces.shape[0] > target:
        rnd += 1
        F = faces.shape[0]
        K = F - target
        keys, face_edge, edge_faces, vf_start, vf_face = _decimate_tables(faces, Nv)
        if rnd == 1:
            ops.quadrics(P, faces, face_edge, edge_faces, vf_start, vf_face, bw, Q)
        E = keys.shape[0]
        ops.flags(keys, edge_faces, flags)
        cost, x = new(E, dtype=torch.float64), new(E, 3, dtype=torch.float64)
        ops.candidates(P, Q, faces, keys, edge_faces, vf_start, vf_face, flags, max_err, cost, x)
        by_cost = torch.sort(cost, stable=True)[1]                # (cost, edge number) ascending: +inf, no candidate, last
        candidates = int((cost < float("inf")).sum())             # the one count the host reads per round
        if candidates == 0:
            break
        W = min(max(1, K // 2), candidates)
        window = torch.sort(by_cost[:W])[0].to(torch.int32)
        h = new(W, dtype=torch.int64)
        ops.hash(keys, window, rnd, h)
        ranked = window[torch.sort(h, stable=True)[1]].contiguous()   # (h, edge number) ascending
        selected = new(W, dtype=torch.uint8)
        ops.select(keys, ranked, vmin, vmin2, selected)
        taken = edge_faces[ranked.long()].long() * selected
        applied = (selected.bool() & (torch.cumsum(taken, 0) - taken < K)).to(torch.uint8)
        ops.apply(keys, ranked, applied, x, P, Q, C, count, vmap)
        mapped, keep = new(F, 3, dtype=torch.int32), new(F, dtype=torch.uint8)
        ops.faces(faces, vmap, mapped, keep)
        faces = mapped[keep.bool()].contiguous()
        if rounds is not None:
            rounds.append((F, E, W, F - faces.shape[0]))
    used = torch.zeros(Nv, dtype=torch.bool, device=dev)
    used[faces.reshape(-1).long()] = True
    faces = (torch.cumsum(used, 0, dtype=torch.int32) - 1)[faces.long()].reshape(-1, 3)
    return Mesh((origin + P[used]).float(), faces.contiguous(), C[used].float())


def simplify_quadric_decimation(mesh, target_number_of_triangles, maximum_error=float("inf"), boundary_weight=1.0, rounds=None):
    """Reduce a Mesh to `target_number_of_triangles` by edge collapses placed by quadric error (the use of Open3D's
    simplify_quadric_decimation and of the simplify step of TRELLIS post-processing; the rules are this project's own, rules
    0 - 11 of the decimation block of include/scorp_gs.h, and were never compared with Open3D's output).  Every vertex
    carries the quadric of its faces' planes, and `boundary_weight` times a plane through every open edge; an edge collapses
    to the minimiser of its ends' summed quadrics.  Each ROUND evaluates every edge, takes the cheapest half of what is still
    to go as its window, and collapses an independent set of the window at once (no two collapses share or neighbour a
    vertex), chosen by a hash so that it is large; edges whose collapse would cost more than `maximum_error`, flip a
    triangle, pinch the surface (link condition) or touch an edge with three or more faces are never taken.  The result has
    target or target - 1 triangles when the target can be reached, more when the rules stop first, and is a function of the
    input alone: two runs agree bit for bit.  Faces with two equal indices and vertices no face references are dropped.
    `rounds`, a list, receives (faces, edges, window, faces removed) of every round.
    Returns a new Mesh on the mesh's device.  CUDA tensors run csrc/mesh_decimate.hip, with the sorts, `unique` and scans
    in torch between the calls; CPU tensors run a Python / numpy form of the same rules, meant for small meshes.

        mesh = simplify_quadric_decimation(post_process_mesh(ex.extract_mesh_unbounded(resolution=1024)), 200_000)
    """
    verts, faces, colors = mesh.vertices, mesh.faces, mesh.colors
    target, max_err, bw = int(target_number_of_triangles), float(maximum_error), float(boundary_weight)
    if target < 0:
        raise ValueError(f"target_number_of_triangles must not be negative; got {target_number_of_triangles}")
    if not max_err >= 0.0:
        raise ValueError(f"maximum_error must not be negative or NaN; got {maximum_error}")
    if not (bw >= 0.0 and np.isfinite(bw)):
        raise ValueError(f"boundary_weight must be finite and not negative; got {boundary_weight}")
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype.is_floating_point:
        raise ValueError("vertices must be [Nv, 3] and faces an integer tensor [F, 3]")
    dev = verts.device
    Nv, F = verts.shape[0], faces.shape[0]
    if colors.dim() != 2 or tuple(colors.shape) != (Nv, 3):
        raise ValueError(f"{colors.shape[0]} colours for {Nv} vertices")
    if Nv > MAX_SIMPLIFY_VERTICES or F > MAX_CLUSTER_FACES:
        raise ValueError(f"more than 2^30 vertices or 2^28 triangles: {Nv}, {F}")
    if F == 0 or Nv == 0:
        return _empty_mesh(dev)
    verts = verts.to(torch.float32).contiguous()
    colors = colors.to(device=dev, dtype=torch.float32).contiguous()
    if not bool(torch.isfinite(torch.stack([verts.amin(), verts.amax()])).all()):   # (a NaN or an infinity reaches one of the two)
        raise ValueError("the vertices are not all finite")
    fmin, fmax = int(faces.min()), int(faces.max())
    if fmin < 0 or fmax >= Nv:
        raise ValueError(f"vertex index {fmin if fmin < 0 else fmax} with {Nv} vertices")
    faces = faces.to(device=dev, dtype=torch.int32).contiguous()
    if dev.type != "cuda":
        return _decimate(verts, colors, faces, target, max_err, bw, _DecimateNumpy(), rounds)
    with torch.cuda.device(dev):
        return _decimate(verts, colors, faces, target, max_err, bw, _DecimateHip(), rounds)


# ---- the extractor ----

def focus_point(origins, directions):
    """The point with the least summed squared distance to the rays (origins [n, 3], directions [n, 3], any length or sign):
    with the projectors P_i = I - d_i d_i^T onto each ray's normal plane it solves (sum P_i) x = sum P_i o_i.  What the
    reference's bounding-sphere estimate takes as the scene centre (focus_point_fn, render_utils.py:68-74)."""
    d = directions / np.linalg.norm(directions, axis=1, keepdims=True)
    P = np.eye(3)[None] - d[:, :, None] * d[:, None, :]
    return np.linalg.solve(P.sum(0), np.einsum("nij,nj->i", P, origins))


class GaussianExtractor:
    """mesh_utils.py:72-295 GaussianExtractor on this package's 2DGS render():

        ex = GaussianExtractor(gaussians, render, pipe)
        ex.reconstruction(cameras)
        mesh = ex.extract_mesh_unbounded(resolution=1024)
    """

    def __init__(self, gaussians, render, pipe, bg_color=None):
        if bg_color is None:
            bg_color = [0, 0, 0]
        self.gaussians = gaussians
        self.device = gaussians.get_xyz.device
        self.render = partial(render, pipe=pipe, bg_color=torch.tensor(bg_color, dtype=torch.float32, device=self.device))
        self.clean()

    @torch.no_grad()
    def clean(self):
        self.depthmaps = None    # [V, H, W] on the device
        self.rgbmaps = None      # [V, 3, H, W]
        self.full_proj = None    # [V, 4, 4]
        self.viewpoint_stack = []

    @torch.no_grad()
    def reconstruction(self, viewpoint_stack):
        """Render every camera and keep its colour and surface-depth maps (the 'render' and 'render_depth' keys)."""
        self.clean()
        self.viewpoint_stack = list(viewpoint_stack)
        if not self.viewpoint_stack:
            raise ValueError("reconstruction needs at least one camera")
        depths, rgbs = [], []
        for cam in self.viewpoint_stack:
            pkg = self.render(cam, self.gaussians)
            rgb, depth = pkg["render"], pkg["render_depth"]
            if depths and depth.shape != depths[0].shape:
                raise ValueError(f"all views must share one resolution: {tuple(depth.shape)} after {tuple(depths[0].shape)}")
            rgbs.append(rgb)
            depths.append(depth)
        self.depthmaps = torch.stack(depths, 0).reshape(len(depths), *depths[0].shape[-2:]).contiguous()
        self.rgbmaps = torch.stack(rgbs, 0).contiguous()
        self.full_proj = torch.stack([cam.full_proj_transform.to(self.device) for cam in self.viewpoint_stack], 0).contiguous()
        self.estimate_bounding_sphere()

    def estimate_bounding_sphere(self):
        """centre = the focus point of the cameras' optical axes, radius = the nearest camera's distance to it
        (mesh_utils.py:124-136).  world_view_transform is stored transposed, so its upper 3x3 holds the camera axes in world
        coordinates as columns: column 2 is the optical axis."""
        axes = np.stack([cam.world_view_transform[:3, 2].detach().cpu().numpy() for cam in self.viewpoint_stack]).astype(np.float64)
        eyes = np.stack([cam.camera_center.detach().cpu().numpy() for cam in self.viewpoint_stack]).astype(np.float64)
        center = focus_point(eyes, axes)
        self.radius = float(np.sqrt(((eyes - center) ** 2).sum(1)).min())
        self.center_host = tuple(float(np.float32(c)) for c in center)   # what the fusion calls take: no device read per call
        self.center = torch.tensor(self.center_host, dtype=torch.float32, device=self.device)

    def _need_maps(self):
        if self.depthmaps is None:
            raise RuntimeError("call reconstruction(viewpoint_stack) first")

    @torch.no_grad()
    def compute_unbounded_tsdf(self, samples, contracted, voxel_size, return_rgb=False):
        """mesh_utils.py:209-247 over the kept views; `contracted`: the samples lie in the contracted unit space of the
        bounding sphere (the reference's inv_contraction is not None).  samples: [M, 3] or a lattice (x, y, z)."""
        self._need_maps()
        return tsdf_fuse(self.depthmaps, self.rgbmaps if return_rgb else None, self.full_proj, samples, voxel_size,
                         contracted=bool(contracted), center=self.center_host, radius=self.radius)

    @torch.no_grad()
    def tsdf_volume(self, resolution, bounds=None):
        """(grid [N, N, N], (x, y, z)): the TSDF over the lattice linspace(-R, R, N)^3 of the contracted space, one dense
        grid.  R defaults to the reference's bound (mesh_utils.py:259-261): the 0.95 quantile of the contracted surfel
        radii plus 0.01, at most 1.9."""
        self._need_maps()
        N = int(resolution)
        if N < 2:
            raise ValueError(f"resolution must be at least 2; got {resolution}")
        if bounds is None:
            n = torch.linalg.vector_norm((self.gaussians.get_xyz.detach() - self.center) / self.radius, dim=-1)
            contracted_n = torch.where(n < 1, n, 2 - 1 / n)   # the norm of the contracted point
            R = min(float(np.quantile(contracted_n.cpu().numpy(), 0.95)) + 0.01, 1.9)
            lo, hi = (-R, -R, -R), (R, R, R)
        else:
            lo, hi = bounds
        coords = tuple(torch.linspace(float(a), float(b), N).to(self.device) for a, b in zip(lo, hi))
        voxel_size = self.radius * 2 / N
        return self.compute_unbounded_tsdf(coords, True, voxel_size), coords

    @torch.no_grad()
    def extract_mesh_unbounded(self, resolution=1024, method="surface_nets"):
        """mesh_utils.py:182-278: the TSDF volume of the contracted space, its zero surface (`method`: "surface_nets" or
        "marching_cubes", as in extract_surface), the vertices un-contracted and clipped to +-32, coloured by a second fusion
        pass over the vertices."""
        _check_method(method)
        grid, coords = self.tsdf_volume(resolution)
        verts, faces = extract_surface(grid, coords, level=0.0, method=method)
        voxel_size = self.radius * 2 / int(resolution)
        if verts.shape[0] == 0:
            return Mesh(verts, faces, torch.empty(0, 3, dtype=torch.float32, device=verts.device))
        verts = (uncontract(verts) * float(self.radius) + self.center).clamp(-MAX_RANGE, MAX_RANGE)
        _, colors = self.compute_unbounded_tsdf(verts, False, voxel_size, return_rgb=True)
        return Mesh(verts, faces, colors)

    def bounded_views(self, depth_trunc=3, mask_backgrond=True):
        """What extract_mesh_bounded hands to the volume (mesh_utils.py:45-69, 161-175): (depth [V, H, W] with 0 where the
        camera's gt_alpha_mask is below 0.5 - when it has one and masking is asked for - and where it exceeds depth_trunc,
        rgb uint8 [V, H, W, 3] = clip(rgb, 0, 1) * 255 truncated, world_to_cam [V, 3, 4], intrinsics [V, 4]), the last two
        taken as to_cam_open3d takes them from world_view_transform and projection_matrix."""
        self._need_maps()
        depth = self.depthmaps
        V, H, W = depth.shape
        dev = self.device
        alphas = [getattr(cam, "gt_alpha_mask", None) for cam in self.viewpoint_stack]
        drop = depth > float(depth_trunc)
        if mask_backgrond and any(a is not None for a in alphas):   # one stacked mask, no per-view indexing
            ones = torch.ones(H, W, device=dev)
            alpha = torch.stack([a.to(dev).reshape(H, W) if a is not None else ones for a in alphas])
            drop = drop | (alpha < 0.5)
        depth = torch.where(drop, torch.zeros((), dtype=depth.dtype, device=dev), depth)
        ndc2pix = torch.tensor([[W / 2, 0, 0, (W - 1) / 2], [0, H / 2, 0, (H - 1) / 2], [0, 0, 0, 1]], dtype=torch.float32, device=dev).T
        proj = torch.stack([cam.projection_matrix.to(dev) for cam in self.viewpoint_stack]).float()
        intrins = (proj @ ndc2pix)[:, :3, :3].transpose(1, 2)
        K = torch.stack([intrins[:, 0, 0], intrins[:, 1, 1], intrins[:, 0, 2], intrins[:, 1, 2]], 1)
        E = torch.stack([cam.world_view_transform.to(dev) for cam in self.viewpoint_stack]).float().transpose(1, 2)[:, :3]
        rgb = (self.rgbmaps.clamp(0.0, 1.0) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        return depth, rgb, E.contiguous(), K

    @torch.no_grad()
    def extract_mesh_bounded(self, voxel_size=0.004, sdf_trunc=0.02, depth_trunc=3, mask_backgrond=True, stride=4,
                             method="surface_nets"):
        """mesh_utils.py:138-180 (the keyword spelling is the reference's): fuse the kept views into a sparse volume of 16^3
        blocks of `voxel_size` voxels, truncation sdf_trunc, depths above depth_trunc dropped, and mesh its zero surface.
        The volume follows the rules written down in include/scorp_gs.h, not Open3D's ScalableTSDFVolume, whose output was
        never available to compare with; the surface is extracted by surface nets unless method="marching_cubes" asks for
        this project's marching cubes (scorp_amd/mc_table.py; its table was not compared with Open3D's either)."""
        _check_method(method)
        depth, rgb, world_to_cam, intrinsics = self.bounded_views(depth_trunc, mask_backgrond)
        return extract_surface_blocks(tsdf_blocks_fuse(depth, rgb, world_to_cam, intrinsics, voxel_size, sdf_trunc, stride=stride),
                                      method=method)

    @torch.no_grad()
    def export_image(self, path):
        """mesh_utils.py:280-294: renders/NNNNN.png, vis/depth_NNNNN.tiff and (where the camera has one) gt/NNNNN.png."""
        from PIL import Image
        self._need_maps()
        dirs = {k: os.path.join(path, k) for k in ("renders", "gt", "vis")}
        for d in dirs.values():
            os.makedirs(d, exist_ok=True)
        u8 = lambda img: Image.fromarray((np.clip(np.nan_to_num(img.permute(1, 2, 0).cpu().numpy()), 0.0, 1.0) * 255).astype(np.uint8))
        for idx, cam in enumerate(self.viewpoint_stack):
            gt = getattr(cam, "original_image", None)
            if gt is not None:
                u8(gt[0:3]).save(os.path.join(dirs["gt"], f"{idx:05d}.png"))
            u8(self.rgbmaps[idx]).save(os.path.join(dirs["renders"], f"{idx:05d}.png"))
            Image.fromarray(self.depthmaps[idx].cpu().numpy().astype(np.float32)).save(os.path.join(dirs["vis"], f"depth_{idx:05d}.tiff"))
