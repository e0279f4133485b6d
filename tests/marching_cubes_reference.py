"""Yardstick of the marching-cubes meshers (csrc/marching_cubes.hip, csrc/marching_cubes_blocks.hip and the numpy forms of
scorp_amd.mesh): the rules of include/scorp_gs.h in float64, written as plain loops over the lattice edges and the cells, in
the vertex and face order of the header.  The case table is the generator's (scorp_amd/mc_table.py); the fields and the mesh
invariants are those of tests/isosurface_reference.py, the block volumes those of tests/tsdf_blocks_reference.py."""
import functools

import numpy as np

from scorp_amd import mc_table
from tests import tsdf_blocks_reference as blk
from tests.isosurface_reference import (SHAPE, directed_edges, euler_characteristic, field, is_closed_and_oriented, lattice,  # noqa: F401
                                        max_edge, signed_volume)

CORNERS = [np.array([n >> 2, (n >> 1) & 1, n & 1]) for n in range(8)]
EYE = np.eye(3, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def case_triangles():
    """case -> list of triangles, each three (first corner, axis) pairs."""
    return tuple(tuple(tuple(mc_table.EDGES[e] for e in tri) for tri in mc_table.triangles(case)) for case in range(256))


def random_field():
    """(grid [24, 24, 24] float32, coords): seeded normal noise with the six rim faces set to +1 (outside), so that every
    crossing next to the rim has its inside end in the interior and the surface is closed.  All 256 cases occur."""
    g = np.random.default_rng(7).standard_normal((24, 24, 24)).astype(np.float32)
    for a in range(3):
        s = [slice(None)] * 3
        for at in (0, -1):
            s[a] = at
            g[tuple(s)] = 1.0
    c = np.linspace(-1.0, 1.0, 24).astype(np.float32)
    return g, (c, c, c)


def cell_cases(f, level=0.0):
    """The case of every cell of the dense grid f, [X - 1, Y - 1, Z - 1]."""
    inside = np.asarray(f).astype(np.float64) < level
    X, Y, Z = inside.shape
    return sum(inside[o[0]:X - 1 + o[0], o[1]:Y - 1 + o[1], o[2]:Z - 1 + o[2]].astype(np.int64) << n for n, o in enumerate(CORNERS))


def marching_cubes(f, coords, level=0.0):
    """(vertices [Nv, 3] float64, faces [Nf, 3] int64).  f [X, Y, Z] (its fp32 values, taken to float64), inside: f < level."""
    f = np.asarray(f).astype(np.float64)
    xyz = [np.asarray(c).astype(np.float64) for c in coords]
    dims = f.shape
    inside = f < level
    vid, verts = {}, []
    for q in np.ndindex(*dims):                                # ascending linear lattice index
        for a in range(3):                                     # then the axis
            if q[a] + 1 >= dims[a]:
                continue
            q1 = tuple(np.array(q) + EYE[a])
            if inside[q] == inside[q1]:
                continue
            t = (level - f[q]) / (f[q1] - f[q])
            p = [xyz[d][q[d]] for d in range(3)]
            p[a] = xyz[a][q[a]] + t * (xyz[a][q[a] + 1] - xyz[a][q[a]])
            vid[q + (a,)] = len(verts)
            verts.append(p)
    tris = case_triangles()
    faces = []
    for c in np.ndindex(dims[0] - 1, dims[1] - 1, dims[2] - 1):   # ascending linear cell index
        case = sum(int(inside[tuple(np.array(c) + o)]) << n for n, o in enumerate(CORNERS))
        for tri in tris[case]:                                    # then table order
            faces.append([vid[tuple(np.array(c) + CORNERS[n0]) + (a,)] for n0, a in tri])
    return np.array(verts, np.float64).reshape(-1, 3), np.array(faces, np.int64).reshape(-1, 3)


def marching_cubes_blocks(blocks, voxel_length):
    """blocks: {(bx, by, bz): (tsdf [4096], weight [4096], colour [4096, 3] or None)} -> (vertices [Nv, 3] float64, faces
    [Nf, 3] int64, colours [Nv, 3] float64 in [0, 1]), in the order of include/scorp_gs.h: plain loops over the crossed lattice
    edges and the valid cells of the blocks' bounding box; a voxel of a missing block has weight 0."""
    bs = sorted(blocks)
    rank = {b: r for r, b in enumerate(bs)}
    lo = np.min(np.array(bs), 0)
    dims = (np.max(np.array(bs), 0) - lo + 1) * 16
    T, Wt, C = np.zeros(dims), np.zeros(dims), np.zeros(tuple(dims) + (3,))
    for b in bs:
        o = (np.array(b) - lo) * 16
        sl = tuple(slice(o[k], o[k] + 16) for k in range(3))
        t, w, c = blocks[b]
        T[sl], Wt[sl] = np.asarray(t, np.float64).reshape(16, 16, 16), np.asarray(w, np.float64).reshape(16, 16, 16)
        if c is not None:
            C[sl] = np.asarray(c, np.float64).reshape(16, 16, 16, 3)
    valid, inside = Wt > 0, T < 0
    X, Y, Z = dims
    vl = np.float64(np.float32(voxel_length))

    @functools.lru_cache(maxsize=None)
    def cell_valid(p):
        if min(p) < 0 or p[0] > X - 2 or p[1] > Y - 2 or p[2] > Z - 2:
            return False
        return all(valid[tuple(np.array(p) + o)] for o in CORNERS)

    def order(p):   # (block rank, local linear index) of lattice point / cell p
        p = np.array(p)
        b = tuple(int(x) for x in (p // 16 + lo))
        l = p % 16
        return rank.get(b, -1), int((l[0] * 16 + l[1]) * 16 + l[2])

    edges = []
    for a in range(3):
        b, c = EYE[(a + 1) % 3], EYE[(a + 2) % 3]
        sl0 = tuple(slice(0, dims[k] - (k == a)) for k in range(3))
        sl1 = tuple(slice(int(k == a), dims[k]) for k in range(3))
        cross = (inside[sl0] != inside[sl1]) & valid[sl0] & valid[sl1]
        for q in np.argwhere(cross):
            if any(cell_valid(tuple(p)) for p in (q, q - b, q - b - c, q - c)):
                edges.append((order(q) + (a,), tuple(q), a))
    edges.sort(key=lambda x: x[0])
    vid, verts, cols = {}, [], []
    for _, q, a in edges:
        q1 = tuple(np.array(q) + EYE[a])
        t = (0.0 - T[q]) / (T[q1] - T[q])
        p = (np.array(q) + lo * 16) + 0.5
        p[a] += t
        vid[q + (a,)] = len(verts)
        verts.append(vl * p)
        cols.append((C[q] + t * (C[q1] - C[q])) / 255.0)
    tris = case_triangles()
    cells = [tuple(p) for p in np.argwhere(np.ones(dims - 1, bool)) if cell_valid(tuple(p))]
    cells.sort(key=order)
    faces = []
    for c in cells:
        case = sum(int(inside[tuple(np.array(c) + o)]) << n for n, o in enumerate(CORNERS))
        for tri in tris[case]:
            faces.append([vid[tuple(np.array(c) + CORNERS[n0]) + (a,)] for n0, a in tri])
    return (np.array(verts, np.float64).reshape(-1, 3), np.array(faces, np.int64).reshape(-1, 3),
            np.array(cols, np.float64).reshape(-1, 3))


def random_blocks():
    """(blocks, voxel_length): the eight blocks of a 32^3 box of seeded normal noise with its rim set to +1, every weight
    positive.  The box's outermost cells reach into blocks that do not exist and are invalid, but they hold no crossing."""
    g = np.random.default_rng(11).standard_normal((32, 32, 32)).astype(np.float32)
    for a in range(3):
        s = [slice(None)] * 3
        for at in (0, -1):
            s[a] = at
            g[tuple(s)] = 1.0
    blocks = {}
    for b in np.ndindex(2, 2, 2):
        sl = tuple(slice(16 * x, 16 * x + 16) for x in b)
        gl = np.array(b)[None] * 16 + blk.LOCAL
        col = np.stack([(37 * gl[:, 0] + 11 * gl[:, 1]) % 256, (53 * gl[:, 1] + 7 * gl[:, 2]) % 256, (29 * gl[:, 2] + 13 * gl[:, 0]) % 256], -1)
        blocks[tuple(int(x) for x in b)] = (g[sl].reshape(-1).copy(), np.ones(4096, np.float32), col.astype(np.float32))
    return blocks, blk.SURFACE_VOXEL


def canonical(v, f):
    """A mesh in an order that does not depend on how its vertices and faces were numbered: vertices sorted by position (they
    must be distinct), every face rotated to start at its smallest vertex, faces sorted."""
    order = np.lexsort(v.T[::-1])
    assert len(np.unique(v, axis=0)) == len(v)
    rank = np.empty(len(v), np.int64)
    rank[order] = np.arange(len(v))
    g = rank[f]
    first = np.argmin(g, 1)
    g = np.stack([g[np.arange(len(g)), (first + s) % 3] for s in range(3)], 1)
    return v[order], g[np.lexsort(g[:, ::-1].T)]
