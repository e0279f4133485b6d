"""The clouds of tests/test_cloud_cpu.py and tests/test_cloud_gpu.py, and the cached yardstick results on them
(tests/cloud_reference.py: computed once per process and shared; callers do not modify them).  No fixture is larger than
4 200 points."""
import functools

import numpy as np

from tests import cloud_reference as ref

SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099)   # the wave, the radix tile, the bbox kernel's 1024
                                                                        # threads and kIcpChunk, several tiles
KNNS = (1, 2, 20, 32)
SIZED_MIN_POINTS = 6
EXACT_RADIUS = 5.0 / 64.0       # the planted pair of blobs_exact_pair lies at exactly this distance


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def blobs(offset=100.0):
    """517 points: two blobs, a sparse bridge between them, uniform noise; moved by `offset` and stored as float32 (spacing
    7.6e-6 at +100, 4.9e-4 at +4096: an fp32 d^2 decides pairs near eps wrongly), in a random order.  With EPS and MIN_POINTS."""
    rng = np.random.default_rng(7)
    A = rng.normal(0, 0.05, (250, 3))
    B = rng.normal(0, 0.05, (200, 3)) + [0.6, 0, 0]
    bridge = np.linspace([0.15, 0, 0], [0.45, 0, 0], 7)
    noise = rng.uniform(-1, 1.6, (60, 3))
    P = (np.concatenate([A, B, bridge, noise]) + offset).astype(np.float32)
    return _frozen(P[rng.permutation(len(P))])


EPS, MIN_POINTS = 0.06, 8


@functools.lru_cache(maxsize=None)
def blobs_exact_pair(offset=100.0):
    """blobs(offset) and two points well away from them whose d^2 is exactly EXACT_RADIUS^2: they differ by (3, 4, 0) / 64,
    which float32 holds exactly at either offset."""
    P = blobs(offset)
    a = np.array([offset, offset, offset + 3.0], np.float32)
    b = a + np.array([3.0 / 64.0, 4.0 / 64.0, 0.0], np.float32)
    return _frozen(np.concatenate([P, a[None], b[None]]))


def d2_fp32(a, b, fused=False):
    """d^2 as an fp32 implementation would form it from the float32 coordinates: every operation rounded to float32, or with
    fused multiply-adds (one rounding each) as fmaf(dx, dx, fmaf(dy, dy, dz dz))"""
    d = (np.asarray(a, np.float32) - np.asarray(b, np.float32)).astype(np.float32)
    if not fused:
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    e = d.astype(np.float64)   # (the product of two float32 is exact in float64, and so is each sum below before its rounding)
    inner = (e[..., 1] * e[..., 1] + (d[..., 2] * d[..., 2]).astype(np.float64)).astype(np.float32)
    return (e[..., 0] * e[..., 0] + inner.astype(np.float64)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def blobs_fp32_traps():
    """blobs(100) and, well away from it and from each other, 8 pairs that an fp32 d^2 decides wrongly at EPS.  Around 100
    the float32 grid is u = 2^-17, so a pair (i, j, k) u apart has d^2 = (i^2 + j^2 + k^2) u^2 exactly in float64; near
    EPS^2 / u^2 = 6.2e7 float32 holds only every fourth integer.  The pairs are searched for: d^2 on one side of EPS^2 in
    float64, on the other in fp32, plain and fused alike (here all eight lie just outside: float32 rounds their integers,
    and EPS^2 itself, down to the same multiple of four).  (The 517 points alone do not have such a pair, and at +4096 they
    cannot: there u = 2^-11, the integers stay below 2^24 and an fp32 d^2 is exact.)"""
    u, r2 = 2.0 ** -17, np.float64(EPS) * np.float64(EPS)
    rng = np.random.default_rng(17)
    top = int(EPS / u)
    ij = rng.integers(0, int(top / np.sqrt(2.0)), (2_000_000, 2))
    k = np.rint(np.sqrt(r2 / (u * u) - (ij.astype(np.float64) ** 2).sum(1))).astype(np.int64)
    step = np.concatenate([ij, k[:, None]], 1).astype(np.float64) * u
    a = np.full(3, 100.0, np.float32)
    b = (a.astype(np.float64) + step).astype(np.float32)
    d2 = (step[:, 0] * step[:, 0] + step[:, 1] * step[:, 1]) + step[:, 2] * step[:, 2]
    inside = d2 <= r2
    wrong = ((d2_fp32(a, b) <= np.float32(r2)) != inside) & ((d2_fp32(a, b, fused=True) <= np.float32(r2)) != inside)
    chosen = np.nonzero(wrong)[0][:8]
    assert len(chosen) == 8
    extra = []
    for t, c in enumerate(chosen):
        base = np.array([105.0 + t, 98.0, 98.0])
        extra += [base, base + step[c]]
    return _frozen(np.concatenate([blobs(100.0), np.asarray(extra).astype(np.float32)]))


@functools.lru_cache(maxsize=None)
def sized(n):
    """n points in a box at +10 with a surface-like sheet, a few exact duplicates and a few far points; (points, radius):
    the radius is 1.2 mean spacings of a uniform cloud (7 points in the ball on average, more on the sheet), so that
    DBSCAN at SIZED_MIN_POINTS finds core, border and noise points and several clusters."""
    rng = np.random.default_rng(1000 + n)
    P = rng.uniform(0.0, 1.0, (n, 3))
    P[: n // 2, 2] = 0.5 + 0.02 * np.sin(7.0 * P[: n // 2, 0])          # half of them on a wavy sheet
    if n >= 8:
        P[rng.integers(0, n, n // 8)] = P[rng.integers(0, n, n // 8)]  # exact duplicates: ties on d^2 = 0
        P[rng.integers(0, n, 2)] += 3.0                                  # floaters
    P = (P + 10.0).astype(np.float32)
    return _frozen(P), 1.2 * (1.0 / max(n, 1)) ** (1.0 / 3.0)


@functools.lru_cache(maxsize=None)
def lattice():
    """the 16^3 integer lattice, n = 4096, in index order z, y, x: with radius sqrt(2.0) an interior point has 19 neighbours,
    and every distance is tied many times over"""
    g = np.arange(16, dtype=np.float32)
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    return _frozen(np.stack([x, y, z], -1).reshape(-1, 3))


@functools.lru_cache(maxsize=None)
def degenerate(name):
    rng = np.random.default_rng(11)
    if name == "identical":
        P = np.tile(np.array([[1.25, -3.5, 100.0]]), (300, 1))
    elif name == "line":
        t = np.sort(rng.uniform(0.0, 1.0, 500))
        P = np.array([5.0, 5.0, 5.0]) + t[:, None] * np.array([0.3, -0.7, 0.648])
    elif name == "plane":
        P = np.concatenate([rng.uniform(0.0, 1.0, (900, 2)), np.full((900, 1), 7.0)], 1)
    elif name == "dense_cell":   # 2 000 points inside one grid cell, 100 spread wide
        P = np.concatenate([rng.normal(0.0, 1e-3, (2000, 3)), rng.uniform(-1.0, 1.0, (100, 3))]) + 50.0
    elif name == "uniform":      # (for the radius above the extent and the radius below every spacing)
        P = rng.uniform(0.0, 1.0, (1025, 3)) + 2.0
    else:
        raise KeyError(name)
    return _frozen(P.astype(np.float32))


DEGENERATE = ("identical", "line", "plane", "dense_cell")
DEGENERATE_RADIUS = {"identical": 0.5, "line": 0.004, "plane": 0.05, "dense_cell": 2e-4}


@functools.lru_cache(maxsize=None)
def chain():
    """2 000 points in index order along a helix, neighbours 0.01 apart: with eps 0.015 and min_points 2 one cluster, and the
    union-find hooks every point under its predecessor"""
    t = np.arange(2000) * 0.01
    P = np.stack([np.cos(t / 1.0), np.sin(t / 1.0), 0.05 * t], -1) * 1.0
    return _frozen((P + 20.0).astype(np.float32)), 0.015, 2


def _cube(n, spacing, at):
    g = np.arange(n) * spacing
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    return np.stack([x, y, z], -1).reshape(-1, 3) + np.asarray(at, np.float64)


@functools.lru_cache(maxsize=None)
def bridge():
    """Two 3^3 lattices of spacing 0.1 (every point core at eps 0.11, min_points 4) and between their facing sides ONE point
    within eps of a core point of each but with only 3 neighbours itself: not core, so the lattices stay two clusters."""
    P = np.concatenate([_cube(3, 0.1, (0.0, 0.0, 0.0)), _cube(3, 0.1, (0.4, 0.0, 0.0)), [[0.3, 0.1, 0.1]]])
    return _frozen(P.astype(np.float32)), 0.11, 4


@functools.lru_cache(maxsize=None)
def tie(order):
    """Two 2^3 unit cubes (x in {0, 1} and x in {4, 5}; every point core at eps 1.5, min_points 7) and the point (2.5, 0, 0),
    exactly 1.5 from a core point of each: the lower core index wins.  `order` "ab" lists the cube at x = 0 first, "ba" the
    other one, so the winner changes."""
    a, b = _cube(2, 1.0, (0.0, 0.0, 0.0)), _cube(2, 1.0, (4.0, 0.0, 0.0))
    P = np.concatenate([a, b] if order == "ab" else [b, a])
    return _frozen(np.concatenate([P, [[2.5, 0.0, 0.0]]]).astype(np.float32)), 1.5, 7


@functools.lru_cache(maxsize=None)
def voxel_cloud(name):
    """(points, colours, voxel_size): "blobs" at h = 0.05, and "faces": multiples of h / 2 at +100, so that points sit on
    cell faces (they belong to the upper cell) and cells hold exact duplicates"""
    rng = np.random.default_rng(5)
    if name == "blobs":
        P, h = blobs(100.0), 0.05
    else:
        P, h = (rng.integers(0, 40, (3000, 3)) * 0.125 + 100.0).astype(np.float32), 0.25
    return _frozen(np.asarray(P)), _frozen(rng.uniform(0, 1, P.shape).astype(np.float32)), h


# ---- the yardstick on them, once ----

@functools.lru_cache(maxsize=None)
def ref_knn(key, k):
    return ref.knn(cloud(key), k)


@functools.lru_cache(maxsize=None)
def ref_count(key, radius):
    return _frozen(ref.radius_count(cloud(key), radius))


@functools.lru_cache(maxsize=None)
def ref_dbscan(key, eps, min_points):
    return ref.dbscan(cloud(key), eps, min_points)


def cloud(key):
    """the points of a fixture by a hashable key: ("blobs", offset), ("exact", offset), ("traps",), ("sized", n), ("lattice",),
    ("degenerate", name), ("chain",), ("bridge",), ("tie", order), ("shuffled", key, seed)"""
    kind = key[0]
    if kind == "blobs":
        return blobs(key[1])
    if kind == "exact":
        return blobs_exact_pair(key[1])
    if kind == "traps":
        return blobs_fp32_traps()
    if kind == "sized":
        return sized(key[1])[0]
    if kind == "lattice":
        return lattice()
    if kind == "degenerate":
        return degenerate(key[1])
    if kind == "chain":
        return chain()[0]
    if kind == "bridge":
        return bridge()[0]
    if kind == "tie":
        return tie(key[1])[0]
    if kind == "shuffled":
        return cloud(key[1])[permutation(key)]
    raise KeyError(key)


def permutation(key):
    return np.random.default_rng(key[2]).permutation(len(cloud(key[1])))
