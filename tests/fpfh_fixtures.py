"""The clouds of tests/test_fpfh_cpu.py and tests/test_fpfh_gpu.py, and the cached yardstick results on them
(tests/fpfh_reference.py: computed once per process and shared; callers do not modify them).  No fixture is larger than 700
points.  Every fixture is held to the margin cap by tests/test_fpfh_cpu.py: at most MARGIN_CAP of its points may have a
pair whose bin coordinate lies within 1e-9 of an integer."""
import functools

import numpy as np

from tests import fpfh_reference as ref

MARGIN_CAP = 0.01
SIZES = (1, 2, 3, 63, 64, 65, 257, 700)
SURFACE_RADIUS, SURFACE_MAX_NN = 0.3, 64
RANSAC_DISTANCE, RANSAC_HYPOTHESES = 0.08, 4096
JITTER = 0.003
SCALE = 0.6        # of the surface: at 700 points a ball of SURFACE_RADIUS then holds some 40 of them


def _frozen(a):
    a.setflags(write=False)
    return a


# g(d) = sum of c x^a y^b z^e over (c, a, b, e): low orders make the shape asymmetric (no symmetry plane or axis), the
# fourth- and fifth-order terms give it ridges a ball of SURFACE_RADIUS can tell apart (on a smoother shape - the first
# three terms alone - the reference matched 32 of 500 descriptors correctly, on this one 317)
TERMS = ((0.30, 1, 1, 0), (0.20, 0, 0, 3), (0.15, 1, 0, 0), (1.5, 2, 1, 1), (-1.6, 1, 2, 2), (1.0, 3, 0, 1), (0.9, 0, 3, 1),
         (-1.0, 1, 3, 0), (1.2, 2, 2, 1))


def _radius_of(d):
    """r(d) = 1 + g(d) on unit directions (times SCALE in surface_points; a uniform scale leaves the normals alone), and
    grad g; r stays within [0.45, 1.65], so the surface is star-shaped about the origin"""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    g, grad = np.zeros(len(d)), np.zeros((len(d), 3))
    for c, a, b, e in TERMS:
        g += c * x ** a * y ** b * z ** e
        if a:
            grad[:, 0] += c * a * x ** (a - 1) * y ** b * z ** e
        if b:
            grad[:, 1] += c * b * x ** a * y ** (b - 1) * z ** e
        if e:
            grad[:, 2] += c * e * x ** a * y ** b * z ** (e - 1)
    return 1.0 + g, grad


def surface_points(n, seed):
    """(points [n, 3], unit outward normals [n, 3]) float64 on the surface |p| = r(p / |p|): jittered Fibonacci directions.
    The normal is the gradient of F(p) = |p| - r(p / |p|): d - (I - d d^T) grad g(d) / |p|."""
    rng = np.random.default_rng(seed)
    k = np.arange(n) + 0.5
    phi = np.arccos(1.0 - 2.0 * k / n)
    theta = np.pi * (1.0 + 5.0 ** 0.5) * k
    d = np.stack([np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)], axis=1)
    d = d + rng.normal(0.0, 0.35 / np.sqrt(n), d.shape)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r, grad = _radius_of(d)
    tangential = grad - d * (grad * d).sum(1, keepdims=True)
    nrm = d - tangential / r[:, None]
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    order = rng.permutation(n)
    return (SCALE * r[:, None] * d)[order], nrm[order]


@functools.lru_cache(maxsize=None)
def surface(n=700, seed=3):
    """The n-point surface as float32 (points, normals)."""
    P, N = surface_points(n, seed)
    return _frozen(P.astype(np.float32)), _frozen(N.astype(np.float32))


def rotation(axis, degrees):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.radians(degrees)
    return np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * (K @ K)


@functools.lru_cache(maxsize=None)
def registration_pair():
    """The 700 / 500 pair: dict of target, target_normals (the 700-point surface), source, source_normals (500 of its
    points, jittered by JITTER and carried by the INVERSE of `truth`, analytic normals carried along), truth [4, 4] (source
    -> target: a rotation of 120 degrees and a translation), subset (the target index of every source point), diagonal
    (of the target's bounding box)."""
    P, N = surface()
    rng = np.random.default_rng(11)
    subset = np.sort(rng.choice(len(P), 500, replace=False))
    R = rotation([0.3, -0.5, 0.8], 120.0)
    t = np.array([0.4, -0.3, 0.25])
    Q = P[subset].astype(np.float64) + rng.normal(0.0, JITTER, (500, 3))
    src = (Q - t) @ R                     # rows: R^T (q - t)
    src_n = N[subset].astype(np.float64) @ R
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, t
    P64 = P.astype(np.float64)
    return {"target": P, "target_normals": N, "source": _frozen(src.astype(np.float32)),
            "source_normals": _frozen(src_n.astype(np.float32)), "truth": _frozen(M), "subset": _frozen(subset),
            "diagonal": float(np.linalg.norm(P64.max(0) - P64.min(0)))}


def _lattice():
    """8 x 8 points 1/8 apart in the plane z = 1/4, all normals (0, 0, 1): every coordinate dyadic, so d^2 is exact and
    ties abound ((d^2, index) decides the lists), and every pair has f1 = f2 = f3 = 0, bin 5 of each block."""
    g = np.arange(8) / 8.0
    P = np.stack([np.repeat(g, 8), np.tile(g, 8), np.full(64, 0.25)], axis=1)
    return P.astype(np.float32), np.tile(np.array([0.0, 0.0, 1.0], np.float32), (64, 1))


def _duplicates():
    """65 surface points of which the last 6 repeat the first 6, three with their normals and three with other normals"""
    P, N = surface(59, 5)
    P2 = np.concatenate([P, P[:6]])
    N2 = np.concatenate([N, N[:3], N[10:13]])
    return P2, N2


def _along_normal():
    """Points 0 and 1 lie exactly along their common normal (dp x u = 0: no feature, but each counts in the other's m);
    four more points in general position around them give both some features."""
    rng = np.random.default_rng(23)
    P = np.concatenate([[[0, 0, 0], [0, 0, 0.25]], rng.uniform(-0.2, 0.2, (4, 3))])
    N = rng.normal(0, 1, (6, 3))
    N /= np.linalg.norm(N, axis=1, keepdims=True)
    N[0] = N[1] = [0, 0, 1]
    return P.astype(np.float32), N.astype(np.float32)


def _sized(n):
    """n surface points, the radius grown as the cloud thins so that a point has a dozen neighbours or so"""
    P, N = surface(n, 100 + n)
    return P, N, float(min(0.2 * np.sqrt(700.0 / n), 1.0))


@functools.lru_cache(maxsize=None)
def cases():
    """{name: (points, normals, radius, max_nn)}"""
    out = {}
    for n in SIZES:
        P, N, r = _sized(n)
        out[f"sized_{n}"] = (P, N, r, 7 if n != 700 else 33)      # (at 7 the radius holds more: truncated)
    P, N = surface()
    out["surface_nn1"] = (P, N, SURFACE_RADIUS, 1)
    out["surface_nn64"] = (P, N, 0.45, 64)                                      # truncated at 64
    out["surface_all"] = (P, N, SURFACE_RADIUS, 64)                             # nothing truncated
    P257, N257, _ = _sized(257)
    out["sparse_257"] = (P257, N257, 0.13, 7)                                   # some points have m = 0
    out["lattice"] = _lattice() + (0.26, 7)
    out["lattice_wide"] = _lattice() + (0.5, 64)
    out["duplicates"] = _duplicates() + (0.6, 64)
    out["along_normal"] = _along_normal() + (0.4, 64)
    pair = registration_pair()
    out["pair_target"] = (pair["target"], pair["target_normals"], SURFACE_RADIUS, SURFACE_MAX_NN)
    out["pair_source"] = (pair["source"], pair["source_normals"], SURFACE_RADIUS, SURFACE_MAX_NN)
    return out


@functools.lru_cache(maxsize=None)
def ref_fpfh(name):
    P, N, radius, max_nn = cases()[name]
    out = ref.fpfh(P, N, radius, max_nn)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def pair_features():
    """(source feature, target feature) [., 33] float64 of the registration pair by the reference"""
    return ref_fpfh("pair_source")["feature"], ref_fpfh("pair_target")["feature"]


@functools.lru_cache(maxsize=None)
def pair_ransac():
    """(samples [RANSAC_HYPOTHESES, 3], the reference's RANSAC result on them): fixed triples over the reference's
    correspondences of the registration pair, analytic normals"""
    pair = registration_pair()
    fs, ft = pair_features()
    c = len(ref.correspondences(fs, ft))
    samples = _frozen(np.random.default_rng(13).integers(0, c, (RANSAC_HYPOTHESES, 3)))
    return samples, ref.ransac(pair["source"], pair["target"], fs, ft, RANSAC_DISTANCE, samples)


@functools.lru_cache(maxsize=None)
def integer_features(ns, nt, seed=0, straddle=()):
    """(src [ns, 33], tgt [nt, 33]) float32 with small integer entries, so every D2 is an exact integer and ties are real:
    the target rows are drawn from few distinct rows (duplicates abound: the lower index must win), and for every b in
    `straddle` (with 1 <= b < nt) rows b - 1 and b are the same row, which is also some source row's exact match."""
    rng = np.random.default_rng([seed, ns, nt])
    pool = rng.integers(0, 4, (max(2, nt // 3), 33))
    tgt = pool[rng.integers(0, len(pool), nt)]
    src = rng.integers(0, 4, (ns, 33))
    for k, b in enumerate(b for b in straddle if 1 <= b < nt):
        row = rng.integers(4, 9, 33)          # unlike every pool row
        tgt[b - 1] = tgt[b] = row
        src[k % ns] = row
    return _frozen(src.astype(np.float32)), _frozen(tgt.astype(np.float32))
