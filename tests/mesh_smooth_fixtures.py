"""Fixtures of the mesh-smooth tests: the smallest meshes at which each rule of the mesh-smooth block of include/scorp_gs.h can
go wrong, with the yardstick's answers (tests/mesh_smooth_reference.py) computed once per fixture and shared.  The strips
put the vertex and the face counts at the edges of the kernels' 256-thread block."""
import functools
import math

import numpy as np

from tests import mesh_smooth_reference as ref
from tests.mesh_render_fixtures import icosphere

BLOCK = 256                # kMeshSmoothThreads of csrc/mesh_smooth.hip
GRID_SIDE = 9
FAN_VALENCE = 300
LAMBDA, MU = 0.5, -0.53
LAPLACIAN_ITERATIONS = (1, 2, 5)
TAUBIN_ITERATIONS = (1, 10)
WEIGHTS = ("uniform", "inverse_distance")
WEIGHTINGS = ("area", "uniform")


def _mesh(verts, faces):
    return np.ascontiguousarray(np.asarray(verts, np.float32).reshape(-1, 3)), np.ascontiguousarray(np.asarray(faces, np.int32).reshape(-1, 3))


def _grid(extra_vertex=None, extra_faces=()):
    """9 x 9 vertices at (i / 8, j / 8, 0): every coordinate, difference, product and sum of the rules is exact"""
    n = GRID_SIDE
    verts = [(i / 8.0, j / 8.0, 0.0) for j in range(n) for i in range(n)]
    faces = []
    for j in range(n - 1):
        for i in range(n - 1):
            k = j * n + i
            faces += [(k, k + 1, k + n), (k + 1, k + n + 1, k + n)]
    if extra_vertex is not None:
        verts.append(extra_vertex)
    return _mesh(verts, faces + list(extra_faces))


def _fan():
    """a hub of valence 300: the step kernel's loop, far past any fixed-size array"""
    rng = np.random.default_rng(3)
    verts = [(0.0, 0.0, 0.3)] + [(math.cos(2 * math.pi * k / FAN_VALENCE) * (1 + 0.1 * rng.standard_normal()),
                                  math.sin(2 * math.pi * k / FAN_VALENCE) * (1 + 0.1 * rng.standard_normal()), 0.05 * rng.standard_normal())
                                 for k in range(FAN_VALENCE)]
    return _mesh(verts, [(0, 1 + k, 1 + (k + 1) % FAN_VALENCE) for k in range(FAN_VALENCE)])


def _strip(num_vertices):
    """an open zigzag strip of num_vertices - 2 triangles, off the plane"""
    rng = np.random.default_rng(num_vertices)
    verts = [(0.1 * (k // 2) + 0.02 * rng.standard_normal(), 0.1 * (k % 2) + 0.02 * rng.standard_normal(), 0.02 * rng.standard_normal())
             for k in range(num_vertices)]
    return _mesh(verts, [(k, k + 1, k + 2) if k % 2 == 0 else (k + 1, k, k + 2) for k in range(num_vertices - 2)])


def _noisy_sphere():
    verts, faces = icosphere(3)
    scale = 1.0 + 0.03 * np.random.default_rng(5).standard_normal(len(verts))
    return _mesh(verts.astype(np.float64) * scale[:, None], faces)


_G = GRID_SIDE
STRIP_VERTICES = tuple(range(BLOCK - 1, BLOCK + 4))    # 255 ... 259 vertices, so 253 ... 257 faces: both counts at 255, 256, 257
BUILDERS = {
    "triangle": lambda: _mesh([(0.1, 0.2, 0.3), (1.3, 0.1, 0.2), (0.4, 1.1, 0.9)], [(0, 1, 2)]),
    "two_triangles": lambda: _mesh([(0.0, 0.0, 0.1), (1.0, 0.1, 0.0), (0.9, 1.0, 0.3), (-0.1, 0.8, -0.2)], [(0, 1, 2), (0, 2, 3)]),
    "tetrahedron": lambda: _mesh([(1.0, 1.0, 1.0), (1.0, -1.0, -1.0), (-1.0, 1.0, -1.0), (-1.0, -1.0, 1.0)],
                                 [(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)]),
    "icosphere2": lambda: _mesh(*icosphere(2)),
    "icosphere3": lambda: _mesh(*icosphere(3)),
    "grid": _grid,
    "grid_unreferenced": lambda: _grid(extra_vertex=(0.5, 0.5, 2.0)),
    "grid_duplicate_face": lambda: _grid(extra_faces=[(4 * _G + 4, 4 * _G + 5, 5 * _G + 4)]),
    "grid_equal_indices": lambda: _grid(extra_faces=[(4 * _G + 4, 4 * _G + 4, 5 * _G + 4), (3, 3, 3)]),
    "grid_non_manifold": lambda: _grid(extra_vertex=(0.5625, 0.5, 0.25), extra_faces=[(4 * _G + 4, 4 * _G + 5, _G * _G)]),
    "fan": _fan,
    **{f"strip{n}": functools.partial(_strip, n) for n in STRIP_VERTICES},
    "noisy_sphere": _noisy_sphere,
}
FIXTURES = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def fixture(name):
    verts, faces = BUILDERS[name]()
    verts.setflags(write=False)
    faces.setflags(write=False)
    return verts, faces


def mesh_of(name, dev):
    import torch
    from scorp_amd.mesh import Mesh
    verts, faces = fixture(name)
    return Mesh(torch.from_numpy(verts.copy()).to(dev), torch.from_numpy(faces.copy()).to(dev), torch.zeros(len(verts), 3, device=dev))


@functools.lru_cache(maxsize=None)
def expected_adjacency(name):
    verts, faces = fixture(name)
    return ref.adjacency(len(verts), faces)


@functools.lru_cache(maxsize=None)
def expected_normals(name, weighting):
    return ref.vertex_normals(*fixture(name), weighting)


@functools.lru_cache(maxsize=None)
def expected_face_normals(name, normalized):
    return ref.face_normals(*fixture(name), normalized)


@functools.lru_cache(maxsize=None)
def _expected_steps(name, kind, weights, fix_boundary):
    factors = [LAMBDA] * max(LAPLACIAN_ITERATIONS) if kind == "laplacian" else [LAMBDA, MU] * max(TAUBIN_ITERATIONS)
    return ref.half_steps(*fixture(name), factors, weights, fix_boundary)


def expected_smooth(name, kind, iterations, weights, fix_boundary):
    """the yardstick's positions after `iterations` of the filter (a filter of n iterations is a prefix of a longer one)"""
    steps = _expected_steps(name, kind, weights, fix_boundary)
    return steps[iterations - 1] if kind == "laplacian" else steps[2 * iterations - 1]


def bits(a):
    """the float32 bits of an array or tensor, for comparisons that tell -0 from +0"""
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    assert a.dtype == np.float32, a.dtype
    return np.ascontiguousarray(a).view(np.uint32)
