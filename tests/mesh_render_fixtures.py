"""Fixtures of the mesh-render tests: the smallest scenes at which each rule of the mesh-render block of include/scorp_gs.h can
go wrong, with the yardstick's answer (tests/mesh_render_reference.py) computed once per fixture and shared.

Most scenes are written in PIXELS through `pixel_camera`: a full_proj with w = z and sx = x / z, sy = y / z, so a vertex
(px z, py z, z) lands on pixel (px, py) at depth z and a test can put vertices exactly on pixel centres.  The images are
37 x 53 (W x H) and 64 x 64: neither side is a multiple of a block shape.  The sphere and the cube use look_at_camera.

Every fixture but the deliberately coplanar one is asserted to have no two different faces whose exact depths at a pixel
agree to within 1e-6 relative (an fp32 ulp is 6e-8): the kernel breaks ties of the ROUNDED depth by index, the yardstick
of the exact one, and only with that gap do the two rules name the same face."""
import functools
import math

import numpy as np

from tests import mesh_render_reference as ref

SMALL = (53, 37)      # H, W
SQUARE = (64, 64)
LARGE_GROUPS = 1024   # kMeshRenderLargeGroups of csrc/mesh_render.hip: the workgroups per view that stride over the large list
SMALL_BOX = 64        # kMeshRenderSmallBox: the pixel centres one thread walks
COUNT_EDGES = (1, 255, 256, 257)                                   # faces at the edges of a 256-thread block
LARGE_EDGES = (LARGE_GROUPS - 1, LARGE_GROUPS, LARGE_GROUPS + 1)   # large-list lengths at the edges of its stride
MIN_DEPTH_GAP = 1e-6


def pixel_camera(H, W):
    m = np.zeros((4, 4), np.float32)
    m[0, 0], m[2, 0] = 2.0 / W, 1.0 / W - 1.0
    m[1, 1], m[2, 1] = 2.0 / H, 1.0 / H - 1.0
    m[2, 2] = m[2, 3] = 1.0
    return m.reshape(1, 16)


def at_pixels(points):
    """[(px, py, z)] -> world vertices float32 [n, 3] that pixel_camera puts there"""
    p = np.asarray(points, np.float64)
    return np.stack([p[:, 0] * p[:, 2], p[:, 1] * p[:, 2], p[:, 2]], 1).astype(np.float32)


def _scene(points, faces, size, **kw):
    H, W = size
    return dict(verts=at_pixels(points), faces=np.asarray(faces, np.int32).reshape(-1, 3), full_proj=pixel_camera(H, W), H=H, W=W,
                near=0.01, cull=False, **kw)


TRIANGLE = [(5.3, 4.1, 1.0), (30.6, 8.2, 2.0), (12.4, 40.7, 4.0)]


def _quad():
    """corners on pixel centres, the diagonal through the centres (k, k): owns [4, 20) x [4, 20), each centre once"""
    return _scene([(4, 4, 1.0), (20, 4, 1.0), (20, 20, 2.0), (4, 20, 2.0)], [[0, 1, 2], [0, 2, 3]], SMALL, owned=16 * 16, once=True)


def _grid():
    """a lattice of step 4.75 pixels from (-1, -1) past the far corner: every pixel of the image is owned exactly once (some
    lattice lines run through pixel centres: x = 18, y = 18 and 37)"""
    H, W = SMALL
    nx, ny = 8, 12
    pts = [(-1 + 4.75 * a, -1 + 4.75 * b, 2.0 + 0.25 * ((3 * a + 5 * b) % 7)) for b in range(ny + 1) for a in range(nx + 1)]
    faces = []
    for b in range(ny):
        for a in range(nx):
            k = b * (nx + 1) + a
            faces += [[k, k + 1, k + nx + 2], [k, k + nx + 2, k + nx + 1]] if (a + b) % 2 else [[k, k + 1, k + nx + 1], [k + 1, k + nx + 2, k + nx + 1]]
    return _scene(pts, faces, SMALL, owned=H * W, once=True)


OVERLAP = [(3.2, 3.3, 2.0), (33.1, 6.4, 2.5), (8.7, 44.2, 3.0), (10.4, 1.2, 1.0), (35.3, 30.8, 1.5), (1.9, 35.6, 1.25)]


def _small_triangles(n, cols, step_x, step_y, rng, z_lo=0.5, z_hi=0.9):
    """n triangles about a pixel across (most own one centre or none), on a jittered lattice so that no two overlap"""
    pts, faces = [], []
    for k in range(n):
        cx, cy = 2.0 + step_x * (k % cols) + rng.uniform(-0.4, 0.4), 2.0 + step_y * (k // cols) + rng.uniform(-0.4, 0.4)
        for ang in rng.uniform(0, 2 * math.pi) + np.array([0.0, 2.1, 4.2]):
            pts.append((cx + 0.75 * math.cos(ang), cy + 0.75 * math.sin(ang), rng.uniform(z_lo, z_hi)))
        faces.append([3 * k, 3 * k + 1, 3 * k + 2] if k % 2 else [3 * k, 3 * k + 2, 3 * k + 1])
    return pts, faces


COVERING = [(-1000.0, -1000.0, 2.0), (3000.0, -1000.0, 3.0), (-1000.0, 3000.0, 5.0)]   # far off-screen, covers the whole image


def _large_mix():
    pts, faces = _small_triangles(300, 20, 3.0, 4.0, np.random.default_rng(11))
    n = len(pts)
    return _scene(pts + COVERING, faces[:150] + [[n, n + 1, n + 2]] + faces[150:], SQUARE, owned=64 * 64)


def _counts():
    pts, faces = _small_triangles(257, 17, 3.5, 3.7, np.random.default_rng(12))
    return _scene(pts, faces, SQUARE)


def _large_list():
    """LARGE_GROUPS + 1 slivers whose boxes hold about a hundred centres (more than SMALL_BOX) and that cover a handful"""
    rng = np.random.default_rng(13)
    pts, faces = [], []
    for k in range(LARGE_GROUPS + 1):
        x, y = rng.uniform(0, 53), rng.uniform(0, 53)
        pts += [(x, y, rng.uniform(1, 4)), (x + 9.3, y + 8.1, rng.uniform(1, 4)), (x + 8.2, y + 9.4, rng.uniform(1, 4))]
        faces.append([3 * k, 3 * k + 1, 3 * k + 2])
    return _scene(pts, faces, SQUARE)


def _near():
    """face 0 has one vertex behind near = 0.01 and is dropped whole; face 1 lies just in front of it and stays"""
    return _scene([(5, 5, 0.005), (30, 8, 1.0), (12, 40, 1.0), (5.5, 5.5, 0.0101), (30.5, 8.5, 0.0101), (12.5, 40.5, 0.0101)],
                  [[0, 1, 2], [3, 4, 5]], SMALL, only_face=1)


def _snap_bound():
    """2^29 / 256 = 2 097 152 pixels: face 0 has a vertex past it and is dropped, face 1 stays within it and covers the image"""
    return _scene([(-100, -100, 1.0), (2097200, -100, 1.0), (-100, 2097200, 1.0), (-100, -100, 2.0), (2097000, -100, 2.0), (-100, 2097000, 2.0)],
                  [[0, 1, 2], [3, 4, 5]], SMALL, only_face=1)


def _degenerate():
    """collinear corners on exact positions (A = 0), repeated indices, and one honest triangle"""
    return _scene([(2, 2, 1.0), (12, 12, 1.0), (22, 22, 1.0)] + TRIANGLE, [[0, 1, 2], [0, 0, 1], [3, 3, 3], [3, 4, 5], [4, 1, 4]], SMALL, only_face=3)


def _bad_indices():
    """faces 0 and 2 name vertices that are not there: dropped, never followed (Python refuses such a mesh; this goes to
    _render_mesh_numpy and the raw C call)"""
    return _scene(TRIANGLE, [[0, 1, 3], [0, 1, 2], [-1, 1, 2], [0, 2 ** 31 - 1, 2]], SMALL, only_face=1)


def icosphere(subdivisions=3):
    """(vertices float32 on the unit sphere, faces int32) wound counter-clockwise seen from outside; 20 x 4^s faces"""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, out = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = out
    return np.array(v, np.float32), np.array(f, np.int32)


SPHERE_EYES = [(3.0, 0.4, 0.3), (-1.2, 2.6, 0.9), (0.5, -0.8, -2.9)]
SPHERE_FOV = 0.9


def look_at_proj(eyes, target, fov, H, W):
    from scorp_amd.camera import look_at_camera
    cams = [look_at_camera(e, target, (0.0, 0.0, 1.0) if abs(e[2]) < 2 else (0.0, 1.0, 0.0), fov, (W, H)) for e in eyes]
    return np.stack([c.full_proj_transform.numpy().reshape(16) for c in cams]).astype(np.float32), cams


def _sphere():
    verts, faces = icosphere(3)
    H, W = SQUARE
    fp, _ = look_at_proj(SPHERE_EYES, (0.0, 0.0, 0.0), SPHERE_FOV, H, W)
    return dict(verts=verts, faces=faces, full_proj=fp, H=H, W=W, near=0.01, cull=False)


CUBE_EYES = [(3.0, 2.0, 1.5), (2.5, -2.2, 1.8)]     # both see +x and +z; the first sees +y, the second -y; nobody sees -x or -z


def _cube():
    v = np.array([(x, y, z) for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)], np.float32)   # index 4 x + 2 y + z
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]   # -x +x -y +y -z +z, outward
    faces = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)
    H, W = SQUARE
    fp, _ = look_at_proj(CUBE_EYES, (0.0, 0.0, 0.0), 0.7, H, W)
    return dict(verts=v, faces=faces, full_proj=fp, H=H, W=W, near=0.01, cull=False,
                views_per_side={"-x": 0, "+x": 2, "-y": 1, "+y": 1, "-z": 0, "+z": 2})


BUILDERS = {
    "triangle": lambda: _scene(TRIANGLE, [[0, 1, 2]], SMALL),
    "triangle_reversed": lambda: _scene(TRIANGLE, [[0, 2, 1]], SMALL),
    "quad": _quad,
    "grid": _grid,
    "overlap": lambda: _scene(OVERLAP, [[0, 1, 2], [3, 4, 5]], SMALL),
    "overlap_swapped": lambda: _scene(OVERLAP, [[3, 4, 5], [0, 1, 2]], SMALL),
    "coplanar": lambda: _scene(TRIANGLE + TRIANGLE + OVERLAP[:3], [[6, 7, 8], [3, 4, 5], [0, 1, 2]], SMALL, duplicates=True),
    "interpenetrating": lambda: _scene([(2.3, 5.1, 1.0), (34.6, 7.2, 3.0), (16.3, 48.4, 1.5), (1.2, 30.7, 1.9), (35.1, 2.4, 2.0), (30.8, 50.3, 2.1)],
                                       [[0, 1, 2], [3, 4, 5]], SMALL),
    "covering": lambda: _scene(COVERING, [[0, 1, 2]], SQUARE, owned=64 * 64, once=True),
    "large_mix": _large_mix,
    "counts": _counts,
    "large_list": _large_list,
    "near": _near,
    "snap_bound": _snap_bound,
    "degenerate": _degenerate,
    "bad_indices": _bad_indices,
    "sphere": _sphere,
    "cube": _cube,
}
FIXTURES = tuple(BUILDERS)
CHECKED_IN_PYTHON = tuple(n for n in FIXTURES if n != "bad_indices")   # (check_mesh refuses that one)


@functools.lru_cache(maxsize=None)
def fixture(name):
    return BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def owners(name, cull=False):
    """the yardstick's owners of every view, and the fixture's own soundness: the depth gap"""
    fx = fixture(name)
    out = [ref.owners_of_view(fx["verts"], fx["faces"], fx["full_proj"][v], fx["H"], fx["W"], fx["near"], cull)
           for v in range(len(fx["full_proj"]))]
    if not fx.get("duplicates"):
        gap = min(ref.closest_depth_pair(o) for o in out)
        assert gap > MIN_DEPTH_GAP, f"fixture {name}: two faces within {gap:.3g} relative at one pixel"
    return out


@functools.lru_cache(maxsize=None)
def expected(name, cull=False, num_faces=None):
    """(face [V, H, W], depth [V, H, W] correctly rounded, visible_views [F]) of the yardstick"""
    fx = fixture(name)
    views = [ref.resolve(o, fx["H"], fx["W"], num_faces) for o in owners(name, cull)]
    F = len(fx["faces"]) if num_faces is None else num_faces
    visible = np.zeros(F, np.int32)
    for _, _, seen in views:
        visible[sorted(seen)] += 1
    return np.stack([v[0] for v in views]), np.stack([v[1] for v in views]), visible
