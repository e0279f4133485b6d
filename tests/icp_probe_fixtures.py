"""Fixtures of the ICP search probe (tests/test_icp_search_gpu.py, tests/test_icp_cpu.py): seeded builders that return
(target, queries, r) in fp32, the float64 brute-force nearest neighbour they are judged by, and a restatement of the
grid formulas of icp_grid_setup_kernel (for failure messages and for checking that a fixture reaches the grid it is
meant to reach).  No GPU.

The probe: registration_icp with a source of ONE point at the origin and inits[j] = translation by queries[j] returns,
per query, whether a target point lies within r (fitness), its float64 distance (inlier_rmse) and, after one update,
the chosen target point itself (transformation[:3, 3])."""
import functools

import numpy as np
from scipy.spatial import cKDTree

MARGIN_CAP = 0.05          # share of a fixture's queries that may lack the margin
MIN_SEPARATION = 1e-6      # targets are pairwise distinct by at least this share of E (far more than 1e-9 of the extent)


# ---- the reference ----

def centre_of(target):
    """The target's bounding-box centre in float64 (exact: the mean of two fp32 values)."""
    t = np.asarray(target, np.float64)
    return 0.5 * (t.min(axis=0) + t.max(axis=0))


def slack(target, queries):
    """(E, delta): E the largest |coordinate - target bounding-box centre| over targets and queries, delta = 2^-20 E."""
    c = centre_of(target)
    E = max(np.abs(np.asarray(target, np.float64) - c).max(), np.abs(np.asarray(queries, np.float64) - c).max())
    return float(E), float(E) * 2.0 ** -20


def positions_of(target):
    """Per target point the id of its position (equal ids: the same three fp32 values) and the lowest original index
    at that position."""
    _, first, inv = np.unique(np.asarray(target), axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    lowest = np.full(len(first), len(target), np.int64)
    np.minimum.at(lowest, inv, np.arange(len(target)))
    return inv, lowest[inv]


def brute_nearest(target, queries, chunk=1024):
    """Float64 brute force on the fp32 values: (i1, d1, d2, ties).  i1 the nearest target point (the lowest index among
    exactly equal d^2), d1 its distance, d2 the distance to the nearest target point at ANOTHER position (inf if there
    is none: duplicates of the nearest point are the same answer, not a rival), ties the number of positions at exactly
    d1."""
    t = np.asarray(target, np.float64)
    q = np.asarray(queries, np.float64)
    pos, _ = positions_of(target)
    weight = 1.0 / np.bincount(pos)[pos]           # a position held by m points counts once
    i1 = np.empty(len(q), np.int64)
    d1 = np.empty(len(q))
    d2 = np.empty(len(q))
    ties = np.empty(len(q), np.int64)
    for b in range(0, len(q), chunk):
        dd = np.zeros((len(q[b:b + chunk]), len(t)))
        for a in range(3):                         # all pairwise d^2, (x^2 + y^2) + z^2
            u = q[b:b + chunk, a, None] - t[None, :, a]
            u *= u
            dd += u
        j = dd.argmin(axis=1)                      # the first minimum: the lowest index
        m = dd[np.arange(len(j)), j]
        i1[b:b + chunk] = j
        d1[b:b + chunk] = np.sqrt(m)
        ties[b:b + chunk] = np.rint(((dd == m[:, None]) * weight[None, :]).sum(axis=1))
        dd[pos[None, :] == pos[j][:, None]] = np.inf
        d2[b:b + chunk] = np.sqrt(dd.min(axis=1))
    return i1, d1, d2, ties


def tree_nearest(target, queries):
    """The same through scipy's cKDTree (k = 2), for targets without duplicate positions and where brute force is too
    large: (i1, d1, d2)."""
    d, i = cKDTree(np.asarray(target, np.float64)).query(np.asarray(queries, np.float64), k=min(2, len(target)))
    if len(target) == 1:
        d, i = d.reshape(-1, 1), i.reshape(-1, 1)
        return i[:, 0].astype(np.int64), d[:, 0], np.full(len(d), np.inf)
    return i[:, 0].astype(np.int64), d[:, 0], d[:, 1]


def has_margin(d1, d2, r, delta):
    """Queries whose answer no rounding of size delta can change: the runner-up is farther by more than 2 delta and
    the nearest distance is not within 2 delta of r."""
    return (d2 - d1 > 2.0 * delta) & (np.abs(d1 - r) > 2.0 * delta)


def min_separation(target):
    """Smallest distance between two target points at different positions (inf for a single position)."""
    t = np.unique(np.asarray(target), axis=0).astype(np.float64)
    if len(t) < 2:
        return np.inf
    return float(cKDTree(t).query(t, k=2)[0][:, 1].min())


# ---- the grid, restated from icp_grid_setup_kernel ----

K_MAX_GRID_DIM = 1024


def grid_of(target):
    """dict(ct, pad, lo, h, dims, grow, cap, radix_passes) of the uniform grid the kernel builds over `target`: cell edge
    h = cbrt(V / nt) over the padded box with every extent at least 1/1024 of the largest, grown by 1.25 until the grid
    has at most cap = max(2 nt, 64) cells; lo relative to ct."""
    t32 = np.asarray(target, np.float32)
    nt = len(t32)
    tlo, thi = t32.min(axis=0).astype(np.float64), t32.max(axis=0).astype(np.float64)
    ct = 0.5 * (tlo + thi)
    ext = thi - tlo
    maxe = float(ext.max())
    pad = 1e-5 * maxe if maxe > 0.0 else 1e-6 * max(1.0, float(np.abs(ct).sum()))
    ext = ext + 2.0 * pad
    floor_e = (maxe + 2.0 * pad) / K_MAX_GRID_DIM
    vol = float(np.prod(np.maximum(ext, floor_e)))
    h = max(float(np.cbrt(vol / nt)), floor_e)
    cap = max(2 * nt, 64)
    grow = 0
    while True:
        n = np.floor(ext / h) + 1.0
        dims = np.clip(n, 1, K_MAX_GRID_DIM).astype(np.int64)
        if int(np.prod(dims)) <= cap:
            break
        h *= 1.25
        grow += 1
    passes = 1
    while passes < 4 and (1 << (8 * passes)) <= cap:
        passes += 1
    return {"ct": ct, "pad": pad, "lo": tlo - ct - pad, "h": h, "dims": dims, "grow": grow, "cap": cap,
            "floor": floor_e, "radix_passes": passes}


def cell_of(grid, x):
    """The cell of a point as the search takes it: per axis floor((x - ct - lo) / h), clamped to [-1, dim]."""
    c = np.floor((np.asarray(x, np.float64) - grid["ct"] - grid["lo"]) / grid["h"])
    return np.clip(c, -1, grid["dims"]).astype(np.int64)


# ---- the builders ----

def _f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    a.setflags(write=False)
    return a


def _lattice(n, spacing, jitter, rng):
    g = np.stack(np.meshgrid(*[np.arange(n) * spacing] * 3, indexing="ij"), -1).reshape(-1, 3)
    return g + rng.uniform(-jitter, jitter, g.shape)


SHELL_DISTANCES = (0.2, 0.6, 0.95, 1.05, 1.5, 3.0, 12.0)    # of r, from the target's bounding box


def _shells(lo, hi, r, per, rng):
    """Points outside the box [lo, hi]: for every face, edge and corner (26 sign patterns) `per` points at each of
    SHELL_DISTANCES x r from the box, inside its extent on the other axes."""
    out = []
    for s in np.ndindex(3, 3, 3):
        s = np.array(s) - 1
        if not s.any():
            continue
        m = np.count_nonzero(s)
        for u in SHELL_DISTANCES:
            p = lo + rng.random((per, 3)) * (hi - lo)
            off = u * r / np.sqrt(m)
            for a in range(3):
                if s[a] < 0:
                    p[:, a] = lo[a] - off
                elif s[a] > 0:
                    p[:, a] = hi[a] + off
            out.append(p)
    return np.concatenate(out)


def _cube64(seed):
    """The jittered 10^3 lattice and its queries in float64 (before the fp32 cast): 1 500 uniform inside the bounding
    box, 1 820 on the shells outside every face, edge and corner."""
    rng = np.random.default_rng(seed)
    tgt = _lattice(10, 0.1, 0.03, rng)
    r = 0.06
    lo, hi = tgt.min(axis=0), tgt.max(axis=0)
    q = np.concatenate([lo + rng.random((1500, 3)) * (hi - lo), _shells(lo, hi, r, 10, rng)])
    return tgt, q, r


def _cube(seed):
    return _cube64(seed)


def _big_r(seed):
    tgt, q, _ = _cube64(seed)
    return tgt, q, 3.0 * float(np.ptp(tgt, axis=0).max())


def _tiny_r(seed):
    tgt, q, _ = _cube64(seed)
    return tgt, q, 0.3 * 0.1


def _offset(seed):
    tgt, q, r = _cube64(seed)
    off = np.array([1000.0, -1000.0, 1000.0])
    return tgt + off, q + off, r


def _plane(seed):
    rng = np.random.default_rng(seed)
    n, r = 1500, 0.05
    tgt = np.column_stack([rng.random((n, 2)), np.full(n, 0.25)])
    nq = 3000
    side = np.where(rng.random(nq) < 0.5, -1.0, 1.0)
    q = np.column_stack([rng.uniform(-0.05, 1.05, (nq, 2)), 0.25 + side * rng.uniform(0.2, 1.5, nq) * r])
    return tgt, q, r


def _line(seed):
    rng = np.random.default_rng(seed)
    n, r = 800, 0.004
    x = (np.arange(n) + rng.uniform(-0.3, 0.3, n)) / n
    tgt = np.column_stack([x[rng.permutation(n)], np.full(n, 0.3), np.full(n, -0.7)])
    nq = 2500
    rho, phi = rng.uniform(0.1, 1.5, nq) * r, rng.uniform(0.0, 2.0 * np.pi, nq)
    q = np.column_stack([rng.uniform(-0.01, 1.01, nq), 0.3 + rho * np.cos(phi), -0.7 + rho * np.sin(phi)])
    return tgt, q, r


def _ball(n, radius, rng):
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v * (radius * rng.random(n) ** (1.0 / 3.0))[:, None]


def _two_clusters(seed):
    """Two blobs of diameter 0.02, 50 diameters apart; r = 1.2 is longer than the gap, so every query hits and the
    search decides between the blobs by the stopping bound alone."""
    rng = np.random.default_rng(seed)
    a, b = np.zeros(3), np.array([1.0, 0.0, 0.0])
    tgt = np.concatenate([a + _ball(500, 0.01, rng), b + _ball(500, 0.01, rng)])
    tgt = tgt[rng.permutation(len(tgt))]
    mid = np.column_stack([rng.uniform(0.05, 0.95, 1000), rng.uniform(-0.05, 0.05, (1000, 2))])
    half = np.column_stack([rng.uniform(0.49, 0.51, 400), rng.uniform(-0.05, 0.05, (400, 2))])
    q = np.concatenate([mid, half, a + _ball(550, 0.012, rng), b + _ball(550, 0.012, rng)])
    return tgt, q, 1.2


def _elongated(seed):
    rng = np.random.default_rng(seed)
    size = np.array([1000.0, 0.5, 0.5])
    tgt = rng.random((2000, 3)) * size
    q = np.column_stack([rng.uniform(-2.0, 1002.0, 3000), rng.uniform(-0.5, 1.0, (3000, 2))])
    return tgt, q, 0.6


def _few(nt):
    def build(seed):
        rng = np.random.default_rng(seed)
        pts = np.array([[0.3, -0.2, 0.5], [0.35, -0.2, 0.5], [0.3, -0.17, 0.52]])[:nt]
        r = 0.1
        q = pts[rng.integers(0, nt, 2000)] + _ball(2000, 2.0 * r, rng)
        return pts, q, r
    return build


def _dup64(seed):
    rng = np.random.default_rng(seed)
    pts = np.repeat(np.array([[0.3, -0.2, 0.5]]), 64, axis=0)
    r = 0.1
    return pts, pts[:1] + _ball(2000, 2.0 * r, rng), r


def _tiles(nt):
    def build(seed):
        rng = np.random.default_rng(seed)
        return rng.random((nt, 3)), rng.random((1000, 3)), 0.8 * nt ** (-1.0 / 3.0)
    return build


def _three_pass(seed):
    rng = np.random.default_rng(seed)
    nt = 40000
    return rng.random((nt, 3)), rng.random((2000, 3)), 0.8 * nt ** (-1.0 / 3.0)


BUILDERS = {
    "cube": _cube, "plane": _plane, "line": _line, "two_clusters": _two_clusters, "big_r": _big_r, "tiny_r": _tiny_r,
    "elongated": _elongated, "few1": _few(1), "few2": _few(2), "few3": _few(3), "dup64": _dup64,
    "tiles255": _tiles(255), "tiles256": _tiles(256), "tiles257": _tiles(257), "tiles1025": _tiles(1025),
    "three_pass": _three_pass, "offset": _offset,
}
TREE_REFERENCE = ("three_pass",)       # nt x queries too large for the brute force
MARGIN_FIXTURES = tuple(BUILDERS)      # every one of them is held to MARGIN_CAP ("ties" is asserted exactly instead)


def _reference(name, tgt, q):
    if name in TREE_REFERENCE:
        i1, d1, d2 = tree_nearest(tgt, q)
        return i1, d1, d2, np.ones(len(q), np.int64)
    return brute_nearest(tgt, q)


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(target, queries, r, reference = (i1, d1, d2, ties)) of a margin fixture: the first seed whose fp32 clouds have
    pairwise distinct positions (dup64 apart) and meet MARGIN_CAP by the float64 reference alone.  Read-only arrays."""
    for seed in range(50):
        tgt, q, r = BUILDERS[name](seed)
        tgt, q, r = _f32(tgt), _f32(q), float(r)
        E, delta = slack(tgt, q)
        if name != "dup64" and (len(np.unique(tgt, axis=0)) != len(tgt) or min_separation(tgt) < MIN_SEPARATION * E):
            continue
        ref = _reference(name, tgt, q)
        if np.mean(~has_margin(ref[1], ref[2], r, delta)) <= MARGIN_CAP:
            for a in ref:
                a.setflags(write=False)
            return tgt, q, r, ref
    raise AssertionError(f"{name}: no seed gave the margin property")


@functools.lru_cache(maxsize=None)
def ties_fixture(shuffle):
    """The integer lattice 8^3 in a shuffled row order and the exact midpoints of its edges, faces and cells (2, 4 and
    8 equidistant points), r = 2: every coordinate, the centre 3.5 and every d^2 are exact in fp32 and in float64.
    Returns (target, queries, r, reference, lattice index of each row)."""
    n = 8
    lat = np.stack(np.meshgrid(*[np.arange(n)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    order = np.random.default_rng(100 + shuffle).permutation(len(lat))
    q = []
    for half in np.ndindex(2, 2, 2):
        half = np.array(half)
        if not half.any():
            continue
        cnt = [n - 1 if b else n for b in half]                      # a midpoint axis has n - 1 places
        base = np.stack(np.meshgrid(*[np.arange(c) for c in cnt], indexing="ij"), -1).reshape(-1, 3)
        q.append(base + 0.5 * half)
    tgt, q = _f32(lat[order]), _f32(np.concatenate(q))
    ref = brute_nearest(tgt, q)
    for a in ref:
        a.setflags(write=False)
    return tgt, q, 2.0, ref, order


# ---- the aggregate path (part 2): a multi-point source with an unambiguous pairing ----

AGGREGATE_NS = (1, 255, 256, 257, 1023, 1024, 1025, 4097, 64 * 1024, 64 * 1024 + 1025)


def aggregate_inits():
    """The identity and a 2 degree rotation about the lattice's centre."""
    b = np.deg2rad(2.0)
    T = np.stack([np.eye(4)] * 2)
    R = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    c = np.full(3, 0.45)
    T[1, :3, :3] = R
    T[1, :3, 3] = c - R @ c
    return T


@functools.lru_cache(maxsize=None)
def aggregate_target():
    return _f32(_lattice(10, 0.1, 0.012, np.random.default_rng(7)))


@functools.lru_cache(maxsize=None)
def aggregate_fixture(ns):
    """_margin_fixture's construction at ns source points: a jittered lattice (spacing 0.1) as the target, lattice
    points sampled with replacement, moved a little (3 degrees, a shift) and given noise as the source.  The first seed
    at which EVERY source point has the margin at both init poses.  Returns (source, target, r, inits, pairs) with
    pairs[j] = (hit mask, nearest index) of the float64 brute force under inits[j]."""
    tgt = aggregate_target()
    r = 0.045
    inits = aggregate_inits()
    a = np.deg2rad(3.0)
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    t64 = tgt.astype(np.float64)
    for seed in range(200):
        rng = np.random.default_rng(1000 + seed)
        sub = t64[rng.integers(0, len(tgt), ns)]
        src = _f32((sub - 0.45) @ R + 0.45 + (0.01, -0.01, 0.005) + rng.normal(scale=0.002, size=sub.shape))
        pairs = []
        for T in inits:
            x = src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
            _, delta = slack(tgt, x)
            i1, d1, d2 = tree_nearest(tgt, x)
            if not has_margin(d1, d2, r, delta).all():
                break
            pairs.append((x, delta))
        else:
            out = []
            for x, _ in pairs:
                i1, d1, _, _ = brute_nearest(tgt, x, chunk=2048)
                out.append((d1 <= r, i1))
            return src, tgt, r, inits, out
    raise AssertionError(f"ns = {ns}: no seed gave every source point the margin")
