"""The clouds of tests/test_orient_cpu.py and tests/test_orient_gpu.py and the cached yardstick results on them
(tests/orient_reference.py: computed once per process and shared; callers do not modify them).  A case is (points [n, 3]
float32, normals [n, 3] float32, neighbours [n, k] int32, center or None)."""
import functools

import numpy as np

from tests import fpfh_fixtures as ffx
from tests import orient_reference as ref

SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257)
SIZED_K = 8            # columns of the sized cases' lists: above n for n = 1, 2, 3, whose rows are padded
CUP = dict(outer=1.0, inner=0.7, height=1.5, bottom=0.3, n=4000, jitter=0.005, seed=1, knn=12)


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def _unit(rng, n):
    v = rng.normal(0.0, 1.0, (n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _sized(n):
    """n points of the jittered surface of the FPFH fixtures, analytic normals with a seeded half negated, the 8 nearest
    (itself included) as the list"""
    P, N = ffx.surface(n, 300 + n)
    rng = np.random.default_rng(n)
    N = np.where(rng.random(n)[:, None] < 0.5, -N, N).astype(np.float32)
    return np.array(P), N, ref.knn(P, SIZED_K), None


def _plane_of_ties():
    """24 x 24 lattice in z = 0, every normal exactly (0, 0, +-1): every weight is exactly 0, so O3's index part decides the
    whole forest.  The list: the 8 nearest others ((d2, index) order)."""
    g = np.arange(24, dtype=np.float64) / 8.0
    P = np.stack([np.repeat(g, 24), np.tile(g, 24), np.zeros(576)], axis=1).astype(np.float32)
    N = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (576, 1))
    N[np.random.default_rng(5).permutation(576)[:288]] *= -1.0
    return P, N, np.ascontiguousarray(ref.knn(P, 9)[:, 1:]), None


def _chain():
    """700 collinear points, each listing its 2 nearest others, random unit normals: hook chains and many rounds"""
    n = 700
    P = np.zeros((n, 3), np.float32)
    P[:, 0] = np.arange(n) / 64.0
    nb = np.stack([np.arange(n) - 1, np.arange(n) + 1], axis=1)
    nb[0], nb[-1] = (1, 2), (n - 2, n - 3)
    return P, _unit(np.random.default_rng(17), n), nb.astype(np.int32), None


def _one_sided(seed):
    """A cluster of 40 points that list their 4 nearest others, and 10 far points that list 4 cluster members each and are
    listed by nobody"""
    rng = np.random.default_rng(seed)
    A = rng.uniform(-0.5, 0.5, (40, 3))
    F = rng.normal(0.0, 1.0, (10, 3))
    F = 6.0 * F / np.linalg.norm(F, axis=1, keepdims=True)
    P = np.concatenate([A, F]).astype(np.float32)
    nb = np.full((50, 4), -1, dtype=np.int32)
    nb[:40] = ref.knn(P[:40], 5)[:, 1:]
    for f in range(10):
        nb[40 + f] = rng.choice(40, 4, replace=False)
    return P, _unit(rng, 50), nb, None


def one_sided_vertices(N, nb):
    """The vertices whose smallest incident edge in O3's order (their component's minimum outgoing edge in the first round)
    is listed only in the OTHER end's row"""
    e, _, _ = ref.sorted_edges(N, nb)
    seen, out = set(), []
    for a, b in e.tolist():
        for v, u in ((a, b), (b, a)):
            if v not in seen:
                seen.add(v)
                if u not in nb[v].tolist():
                    out.append(v)
    return out


@functools.lru_cache(maxsize=None)
def one_sided_seed():
    """The first seed at which a CLUSTER point's smallest edge is one only a far point lists"""
    for seed in range(200):
        P, N, nb, _ = _one_sided(seed)
        if any(v < 40 for v in one_sided_vertices(N, nb)):
            return seed
    raise AssertionError("no seed below 200 gives a one-sided minimum edge")


TIE_PAIR = (120, 121)   # the two members of the component of _two_components that ties


def _two_components():
    """Two clusters of 60 farther apart than their lists reach (the 6 nearest of the own cluster), point 7's row all -1
    (others still list it), and a pair of points that list each other.  About the given centre (the origin, midway) cluster
    A's normals point mostly away and stay, cluster B's mostly towards it and are flipped, the pair ties at votes = 0."""
    rng = np.random.default_rng(29)
    A = rng.normal(0.0, 0.3, (60, 3)) + [4.0, 0.0, 0.0]
    B = rng.normal(0.0, 0.3, (60, 3)) + [-4.0, 0.0, 0.0]
    P = np.concatenate([A, B, [[5.0, 30.0, 0.0], [25.0, 1.0, 0.0]]]).astype(np.float32)
    N = np.zeros((122, 3), np.float32)
    N[:60] = [1.0, 0.0, 0.0]
    N[60:120] = [1.0, 0.0, 0.0]                                   # towards the origin from x = -4
    N[:120] += rng.normal(0.0, 0.2, (120, 3)).astype(np.float32)
    N[[3, 11, 64, 90]] *= -1.0                                    # a few against their cluster
    N[120], N[121] = (0.0, 1.0, 0.0), (0.8, -0.6, 0.0)            # dot < 0: opposite; dd = 30 and, with its O4 sign, -(20 - 0.6)
    nb = np.full((122, 6), -1, dtype=np.int32)
    nb[:60] = ref.knn(P[:60], 7)[:, 1:]
    nb[60:120] = ref.knn(P[60:120], 7)[:, 1:] + 60
    nb[7] = -1
    nb[120, 0], nb[121, 0] = 121, 120
    return P, N, nb, np.zeros(3)


def _perpendicular():
    """Pairs (1,0,0) / (0,1,0) whose dot is exactly 0 (no flip, weight 1), a zero normal (its flip is -0.0), and non-unit
    normals that give w < 0; every row lists the next two points round the ring, point 9 also itself and a duplicate."""
    N = np.array([[1, 0, 0], [0, 1, 0], [-1, 0, 0], [0, -1, 0], [0, 0, 0], [0, 0, 2], [0, 0, -3], [1.5, 1.5, 0], [-2, 0.5, 0],
                  [0, 1, 0], [1, 0, 0], [0.5, 0.5, -4]], dtype=np.float32)
    n = len(N)
    P = np.stack([np.cos(np.arange(n) * 0.5), np.sin(np.arange(n) * 0.5), 0.1 * np.arange(n)], axis=1).astype(np.float32)
    nb = np.stack([(np.arange(n) + 1) % n, (np.arange(n) + 2) % n, np.full(n, -1), np.full(n, -1)], axis=1).astype(np.int32)
    nb[9, 2], nb[9, 3] = 9, 10
    return P, N, nb, None


def cup_surface(n=CUP["n"], seed=CUP["seed"], jitter=CUP["jitter"], handle=0):
    """(points, outward unit normals) float64 on a thick-walled cup about the z axis - outer wall, inner wall, outer bottom,
    inner bottom, rim - sampled uniformly in proportion to area, every coordinate jittered by N(0, jitter).  handle > 0: that
    many further points on the five outer faces of a solid block on the wall at +x (a mug: no symmetry axis left)."""
    R, r, H, b = CUP["outer"], CUP["inner"], CUP["height"], CUP["bottom"]
    rng = np.random.default_rng(seed)
    area = np.array([2 * np.pi * R * H, 2 * np.pi * r * (H - b), np.pi * R * R, np.pi * r * r, np.pi * (R * R - r * r)])
    part = rng.choice(5, n, p=area / area.sum())
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    u, v = rng.random(n), rng.random(n)
    c, s, zero, one = np.cos(phi), np.sin(phi), np.zeros(n), np.ones(n)
    disc_R, disc_r, ring = R * np.sqrt(u), r * np.sqrt(u), np.sqrt(r * r + u * (R * R - r * r))
    P = np.select([(part == k)[:, None] for k in range(5)],
                  [np.stack([R * c, R * s, H * v], 1), np.stack([r * c, r * s, b + (H - b) * v], 1),
                   np.stack([disc_R * c, disc_R * s, zero], 1), np.stack([disc_r * c, disc_r * s, zero + b], 1),
                   np.stack([ring * c, ring * s, zero + H], 1)])
    N = np.select([(part == k)[:, None] for k in range(5)],
                  [np.stack([c, s, zero], 1), np.stack([-c, -s, zero], 1), np.stack([zero, zero, -one], 1),
                   np.stack([zero, zero, one], 1), np.stack([zero, zero, one], 1)])
    if handle:
        lo, hi = np.array([R - 0.02, -0.15, 0.5]), np.array([R + 0.45, 0.15, 1.1])     # the block; its -x face is inside the wall
        e = hi - lo
        faces = [(0, 1), (1, 0), (1, 1), (2, 0), (2, 1)]                              # (axis, side): +x, -y, +y, -z, +z
        fa = np.array([e[(a + 1) % 3] * e[(a + 2) % 3] for a, _ in faces])
        pick = rng.choice(5, handle, p=fa / fa.sum())
        Q = lo + rng.random((handle, 3)) * e
        M = np.zeros((handle, 3))
        for k, (a, side) in enumerate(faces):
            sel = pick == k
            Q[sel, a] = hi[a] if side else lo[a]
            M[sel, a] = 1.0 if side else -1.0
        P, N = np.concatenate([P, Q]), np.concatenate([N, M])
    return P + rng.normal(0.0, jitter, P.shape), N


@functools.lru_cache(maxsize=None)
def cup():
    """(points float32, analytic outward normals float64)"""
    P, N = cup_surface()
    return _frozen(P.astype(np.float32), N)


@functools.lru_cache(maxsize=None)
def cup_pca():
    """(PCA normals float32, their list [n, 12] int32) of the cup in numpy"""
    return _frozen(*ref.pca_normals(cup()[0], CUP["knn"]))


MUG = dict(n=4000, handle=600, source=3200, jitter=0.003)


@functools.lru_cache(maxsize=None)
def mug_pair():
    """The concave registration pair: dict of target (the cup of 4000 points plus 600 on a solid block as a handle, float32),
    target_normals (analytic, float64), source (3200 of its points, jittered and carried by the INVERSE of `truth`),
    source_normals, truth [4, 4] (source -> target: the 120-degree pose of the FPFH fixtures), diagonal."""
    P, N = cup_surface(n=MUG["n"], handle=MUG["handle"])
    rng = np.random.default_rng(11)
    subset = np.sort(rng.choice(len(P), MUG["source"], replace=False))
    R = ffx.rotation([0.3, -0.5, 0.8], 120.0)
    t = np.array([0.4, -0.3, 0.25])
    src = ((P[subset] + rng.normal(0.0, MUG["jitter"], (len(subset), 3))) - t) @ R
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, t
    tgt = P.astype(np.float32)
    out = {"target": tgt, "target_normals": N, "source": src.astype(np.float32), "source_normals": N[subset] @ R, "truth": M,
           "diagonal": float(np.linalg.norm(tgt.astype(np.float64).max(0) - tgt.astype(np.float64).min(0)))}
    _frozen(*out.values())
    return out


def outward_fraction(normals, truth):
    return float((np.einsum("ij,ij->i", np.asarray(normals, np.float64), truth) > 0).mean())


@functools.lru_cache(maxsize=None)
def cases():
    """{name: (points, normals, neighbours, center)}"""
    out = {f"sized_{n}": _sized(n) for n in SIZES}
    out["plane_of_ties"] = _plane_of_ties()
    out["chain"] = _chain()
    out["one_sided"] = _one_sided(one_sided_seed())
    out["two_components"] = _two_components()
    out["perpendicular"] = _perpendicular()
    out["cup"] = (cup()[0],) + cup_pca() + (None,)
    for case in out.values():
        _frozen(*case)
    return out


@functools.lru_cache(maxsize=None)
def reference(name, component_sign="majority_away", default_center=False):
    """The yardstick's result on a case (default_center: the case's own centre set aside)"""
    P, N, nb, center = cases()[name]
    out = ref.orient(P, N, nb, None if default_center else center, component_sign)
    _frozen(*out.values())
    return out
