"""Fixtures and the judge of the point-to-mesh distance tests (tests/test_mesh_distance_cpu.py, _gpu.py), each small enough
for a few seconds: fixture(name) = (vertices float32 [Nv, 3], faces int32 [F, 3], queries float32 [Q, 3], max_distance) and
reference(name) = the yardstick's (best d^2, face, least d^2 over the other faces), computed once per process and read-only.

The tolerance is MEASURED, not guessed: MEASURED_CPU_SPREAD is the largest |d^2 - yardstick d^2| / D^2 between the package's
numpy form and the yardstick over all fixtures here (D^2 the squared diagonal of the bounding box of mesh and finite
queries), taken on the CPU; TOL_REL = min(16 x that, 1e-9), so that an fp32 evaluation (1e-7) can never pass."""
import functools

import numpy as np

from tests import mesh_distance_reference as ref

MEASURED_CPU_SPREAD = 4e-17        # tests/test_mesh_distance_cpu.py prints the figure per fixture and holds it
TOL_REL = min(16.0 * MEASURED_CPU_SPREAD, 1e-9)
MARGIN_CAP = 0.05                  # the rule of tests/test_icp_search_gpu.py
BLOCK = 256                        # threads per block of the query kernel, keys per tile of the queries' sort
# Where the nearest point is on an edge or at a vertex two or more faces tie mathematically, so the index cannot be held:
# the mesh's own vertices (d = 0 at a vertex of about six faces), points outside a convex surface (the share of space whose
# nearest point is on an edge grows like distance / radius) and the few-face fixtures whose queries ring a closed solid.
TIE_FIXTURES = ("sphere_vertices", "sphere_random", "two_clusters")


def _f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    a.setflags(write=False)
    return a


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    a.setflags(write=False)
    return a


def _one_triangle():
    A, B, C = np.array([0.1, 0.2, 0.3]), np.array([1.2, 0.1, 0.5]), np.array([0.4, 1.0, 0.1])
    verts = _f32([A, B, C])
    A, B, C = (verts[k].astype(np.float64) for k in range(3))
    n = np.cross(B - A, C - A)
    n /= np.linalg.norm(n)
    w = np.arange(-1.0, 2.01, 0.25)                      # weights of B and C: all seven regions of the plane
    wb, wc = (g.reshape(-1) for g in np.meshgrid(w, w, indexing="ij"))
    flat = A + wb[:, None] * (B - A) + wc[:, None] * (C - A)
    q = [flat + s * n for s in (-0.5, 0.0, 0.5)]         # both sides of the plane, and on it
    q.append(np.stack([A, B, C, 0.5 * (A + B), 0.5 * (B + C), 0.5 * (C + A)]))      # at the vertices (d = 0), on the edges
    extent = np.ptp(verts, axis=0).max()
    q.append(1e3 * extent * np.array([[1, 1, 1], [-1, 1, -1], [1, -1, 0.5], [0, 0, -1]], np.float64))   # far away
    return verts, _i32([[0, 1, 2]]), _f32(np.concatenate(q)), np.inf


def _collinear():
    rng = np.random.default_rng(11)
    return _f32([[0, 0, 0], [2, 2, 2], [1, 1, 1]]), _i32([[0, 1, 2]]), _f32(rng.uniform(-1, 3, (200, 3))), np.inf


def _point_faces():
    rng = np.random.default_rng(12)
    verts = _f32([[0.5, 0.25, -1.0], [-1, 2, 0.5], [-1, 2, 0.5], [-1, 2, 0.5]])
    return verts, _i32([[0, 0, 0], [1, 2, 3]]), _f32(rng.uniform(-2, 3, (200, 3))), np.inf


_OCTA_V = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
_OCTA_F = [[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]]


def _mixed_degenerate():
    """an octahedron with a collinear face and a point face inside it; the queries mostly inside (outside a convex solid the
    nearest point is on an edge for a large share of space)"""
    rng = np.random.default_rng(13)
    verts = _OCTA_V + [[-0.25, -0.25, 0.0], [0.25, 0.25, 0.0], [0.0, 0.0, 0.0], [0.1, -0.2, 0.15]]
    faces = _OCTA_F + [[6, 7, 8], [9, 9, 9]]
    inside = rng.uniform(-1, 1, (4000, 3))
    inside = inside[np.abs(inside).sum(1) < 0.9][:390]
    return _f32(verts), _i32(faces), _f32(np.concatenate([inside, rng.uniform(-2, 2, (10, 3))])), np.inf


def _flat_mesh(seed=14):
    rng = np.random.default_rng(seed)
    nx, ny = 6, 5
    x, y = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), indexing="ij")
    v = np.stack([x + rng.uniform(-0.3, 0.3, x.shape), y + rng.uniform(-0.3, 0.3, x.shape), np.full(x.shape, 0.25)], -1).reshape(-1, 3)
    idx = np.arange(nx * ny).reshape(nx, ny)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    return _f32(v), _i32(np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]))


def _flat():
    rng = np.random.default_rng(15)
    verts, faces = _flat_mesh()
    q = np.concatenate([rng.uniform([0.5, 0.5, -2], [4.5, 3.5, 2.5], (1100, 3)), rng.uniform([-2, -2, -2], [7, 6, 2], (40, 3))])
    return verts, faces, _f32(q), np.inf


def _faces1():
    rng = np.random.default_rng(16)
    return _f32([[0, 0, 0], [1e-3, 0, 0], [0, 1e-3, 1e-3]]), _i32([[0, 1, 2]]), _f32(rng.uniform(-2e-3, 3e-3, (100, 3))), np.inf


def _faces2():
    rng = np.random.default_rng(17)
    verts = _f32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.2, 0.2, 0.7], [1.2, 0.3, 0.9], [0.1, 1.4, 0.8]])
    return verts, _i32([[0, 1, 2], [3, 4, 5]]), _f32(rng.uniform(-1, 2, (200, 3))), np.inf


def _two_clusters():
    rng = np.random.default_rng(18)
    o = np.array(_OCTA_V, np.float64)
    verts = np.concatenate([o, 0.5 * o + [100.0, 3.0, -2.0]])
    faces = np.concatenate([np.array(_OCTA_F), np.array(_OCTA_F) + 6])
    t = rng.random((300, 1))
    q = (1 - t) * np.array([0.0, 0, 0]) + t * np.array([100.0, 3.0, -2.0]) + rng.normal(0, 2.0, (300, 3))
    return _f32(verts), _i32(faces), _f32(q), np.inf


def _scene_sized():
    """the ground plane after decimation: two triangles whose bounding boxes are the whole scene (one planar quad, the plane
    z = x of the cube [-10, 10]^3, so that no crease ties them) and 508 small ones on a flat patch.  With F = 510 the grid
    starts at 16^3 = 4096 cells (cap 8 F + 64 = 4144); the two large triangles alone are then 8192 pairs, above the cap of
    8 F + 4096 = 8176, and the cell has to grow."""
    rng = np.random.default_rng(19)
    n = 17
    x, y = np.meshgrid(np.linspace(-0.5, 0.5, n), np.linspace(-0.5, 0.5, n), indexing="ij")
    patch = np.stack([x + rng.uniform(-0.01, 0.01, x.shape), y + rng.uniform(-0.01, 0.01, x.shape), np.full(x.shape, 5.0)], -1).reshape(-1, 3)
    idx = np.arange(n * n).reshape(n, n) + 4
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    verts = np.concatenate([[[-10, -10, -10], [10, -10, 10], [10, 10, 10], [-10, 10, -10]], patch])
    faces = np.concatenate([[[0, 1, 2], [0, 2, 3]], np.stack([a, b, c], 1), np.stack([a, c, d], 1)[:-4]])
    q = np.concatenate([rng.uniform(-10, 10, (300, 3)), rng.uniform([-0.7, -0.7, 4.3], [0.7, 0.7, 5.6], (300, 3))])
    return _f32(verts), _i32(faces), _f32(q), np.inf


@functools.lru_cache(maxsize=None)
def sphere_mesh(method="surface_nets", n=18, radius=1.0):
    """the closed sphere of extract_surface (the numpy form) on an n^3 lattice over [-1.3, 1.3]^3: between one and two thousand faces at n = 18"""
    import torch
    from scorp_amd.mesh import extract_surface
    c = torch.linspace(-1.3, 1.3, n)
    x, y, z = torch.meshgrid(c, c, c, indexing="ij")
    v, f = extract_surface(torch.sqrt(x * x + y * y + z * z) - radius, (c, c, c), method=method)
    return _f32(v.numpy()), _i32(f.numpy())


def _unit(n, rng):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _sphere_shell():
    """within a quarter of a cell of the surface, where the wedge of space whose nearest point is on an edge is thin"""
    rng = np.random.default_rng(20)
    return sphere_mesh() + (_f32(_unit(2048, rng) * rng.uniform(0.96, 1.04, (2048, 1))), np.inf)


def _sphere_random():
    rng = np.random.default_rng(21)
    return sphere_mesh() + (_f32(rng.uniform(-1.3, 1.3, (4096, 3))), np.inf)


def _sphere_vertices():
    verts, faces = sphere_mesh()
    return verts, faces, verts, np.inf


def _sphere_analytic():
    rng = np.random.default_rng(22)
    return sphere_mesh() + (_f32(_unit(1024, rng)), np.inf)


def _sliver():
    """aspect ratio 1e6, in two orientations; queries around them and right above the thin faces"""
    rng = np.random.default_rng(23)
    verts = _f32([[0, 0, 0], [1, 0, 0], [0.5, 1e-6, 0], [0.2, 0.3, 0.4], [0.9, 1.0, 1.1], [0.55 + 7e-7, 0.65 - 7e-7, 0.75]])
    above = np.stack([rng.uniform(0.1, 0.9, 60), rng.uniform(0, 1e-6, 60) * 0.4, rng.uniform(-0.05, 0.05, 60)], 1)
    q = np.concatenate([rng.uniform([-0.5, -0.5, -0.5], [1.5, 1.5, 1.5], (300, 3)), above])
    return verts, _i32([[0, 1, 2], [3, 4, 5]]), _f32(q), np.inf


def _max_distance():
    """queries over the interior of the flat mesh (z = 0.25) at heights just inside and just outside max_distance = 0.5"""
    rng = np.random.default_rng(24)
    verts, faces = _flat_mesh()
    n = 240
    rel = np.repeat([-1e-2, -1e-4, 1e-4, 1e-2, -0.5, 0.5], n // 6)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    q = np.stack([rng.uniform(1, 4, n), rng.uniform(1, 3, n), 0.25 + sign * 0.5 * (1.0 + rel)], 1)
    return verts, faces, _f32(q), 0.5


BUILDERS = {"one_triangle": _one_triangle, "collinear": _collinear, "point_faces": _point_faces, "mixed_degenerate": _mixed_degenerate,
            "flat": _flat, "faces1": _faces1, "faces2": _faces2, "two_clusters": _two_clusters, "scene_sized": _scene_sized,
            "sphere_shell": _sphere_shell, "sphere_random": _sphere_random, "sphere_vertices": _sphere_vertices,
            "sphere_analytic": _sphere_analytic, "sliver": _sliver, "max_distance": _max_distance}
FIXTURES = tuple(BUILDERS)
# query counts at the block edges of the query kernel and of the sort's tiles, on the "flat" fixture's first queries
# (the kernel has no passes: one thread per query, any count in one launch; 1025 needs a fifth block)
BLOCK_EDGE_COUNTS = (1, BLOCK - 1, BLOCK, BLOCK + 1, 4 * BLOCK + 1)


@functools.lru_cache(maxsize=None)
def fixture(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    verts, faces, q, _ = fixture(name)
    out = ref.brute_force(q, verts, faces)
    for a in out:
        a.setflags(write=False)
    return out


def diagonal2(verts, q):
    """D^2: the squared diagonal of the bounding box of the mesh and the finite queries"""
    pts = np.concatenate([verts.astype(np.float64), q.astype(np.float64)[np.isfinite(q).all(1)]])
    return float((np.ptp(pts, axis=0) ** 2).sum())


def lacks_margin(name, rows=slice(None)):
    """per query: the second-best face is within twice the tolerance of the best, or the best within it of the cut-off"""
    verts, faces, q, r = fixture(name)
    best, _, second = (a[rows] for a in reference(name))
    tol = TOL_REL * diagonal2(verts, q)
    return ~(second - best > 2.0 * tol) | (np.abs(best - r * r) <= 2.0 * tol)


def judge(name, d2, face, closest, rows=slice(None)):
    """Every assertion on one point_mesh_distance result (numpy arrays) for the fixture's queries[rows]; returns the largest
    |d^2 - yardstick| / D^2 over the hits."""
    verts, faces, q, r = fixture(name)
    best, bface, second = (a[rows] for a in reference(name))
    D2 = diagonal2(verts, q)
    q = q[rows]
    tol = TOL_REL * D2
    assert d2.dtype == np.float64 and face.dtype == np.int32 and closest.dtype == np.float32
    assert d2.shape == (len(q),) and face.shape == (len(q),) and closest.shape == (len(q), 3)
    hit = face >= 0
    near_cut = np.abs(best - r * r) <= 2.0 * tol
    want_hit = best <= r * r
    bad = (hit != want_hit) & ~near_cut
    assert not bad.any(), f"{name}: hit flag differs from the yardstick's at {np.flatnonzero(bad)[:5]} (best {best[bad][:5]}, cut-off {r * r})"
    assert np.isinf(d2[~hit]).all() and (d2[~hit] > 0).all() and np.isnan(closest[~hit]).all()
    assert (face[hit] < len(faces)).all()
    err = np.abs(d2[hit] - best[hit])
    worst = float(err.max() / D2) if hit.any() else 0.0
    assert (err <= tol).all(), f"{name}: d^2 off the yardstick's minimum by {worst:.3g} D^2 (tolerance {TOL_REL:.3g} D^2)"
    c_ref, d_ref = ref.on_faces(q[hit], verts, faces, face[hit])
    assert (np.abs(d_ref - best[hit]) <= tol).all(), f"{name}: the returned face is not a nearest one"
    margin = ~lacks_margin(name, rows)
    bad = margin & (face != np.where(want_hit, bface, -1))
    assert not bad.any(), f"{name}: with the margin, another face than the yardstick's at {np.flatnonzero(bad)[:5]}"
    ulp = np.spacing(np.float32(max(np.abs(verts).max(), np.abs(c_ref).max() if hit.any() else 0.0))).astype(np.float64)
    off = np.abs(closest[hit].astype(np.float64) - c_ref)
    assert (off <= ulp).all(), f"{name}: closest off the yardstick's point on the returned face by {off.max() / ulp:.3g} ulp"
    return worst
