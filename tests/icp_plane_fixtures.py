"""Fixtures of the point-to-plane ICP and normal-estimation tests (tests/test_icp_plane_cpu.py checks their properties
with the float64 yardstick alone; tests/test_icp_plane_gpu.py and tests/test_normals_gpu.py assert them again and then
hold the kernels to the yardstick on them).  Seeded, cached, read-only.  No GPU.

Which conditions apply where.  A fixture whose GPU result is compared with the yardstick's number for number (the
aggregate sizes, the margin fixture, the rank-deficient cases) must pair every source point unambiguously at every pose
the run searches (icp_probe_fixtures.has_margin; the margin fixture and the rank-deficient cases test_icp_gpu._margin_ok
as well) and must keep every eigenvalue ratio of its
A matrices out of [1e-14, 1e-10], so that the 1e-12 cut falls the same way on both sides.  The planted-pose fixture is
run to convergence and only asked for the pose and the update counts, so it is held to the eigenvalue condition alone.
A normals fixture may exclude points that lack the neighbour margin (k-th and (k + 1)-th neighbour distances more than
2 slack apart) or the eigen-gap (l_1 - l_0 >= 1e-3 l_2): at most MARGIN_CAP of them."""
import functools

import numpy as np

from tests import icp_plane_reference as pref
from tests import icp_probe_fixtures as fx
from tests import icp_reference as ref
from tests.test_icp_gpu import _margin_ok

MARGIN_CAP = fx.MARGIN_CAP
EIGEN_GAP = 1e-3
RUN_UPDATES = 5


def _f32(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    a.setflags(write=False)
    return a


def unit_normals(n, seed):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return _f32(v / np.linalg.norm(v, axis=1, keepdims=True))


def poses_have_margin(src, tgt, poses, r, relative=True):
    """icp_probe_fixtures.has_margin for every source point at every pose; with `relative` also test_icp_gpu._margin_ok
    (the aggregate fixtures, built on has_margin alone at up to 66 561 points, are held to the first only)."""
    s64, t64 = np.asarray(src, np.float64), np.asarray(tgt, np.float64)
    if relative and len(t64) > 1 and not _margin_ok(s64, t64, poses, r):
        return False
    for T in poses:
        x = s64 @ T[:3, :3].T + T[:3, 3]
        _, delta = fx.slack(tgt, x)
        _, d1, d2 = fx.tree_nearest(tgt, x)
        if not fx.has_margin(d1, d2, r, delta).all():
            return False
    return True


# ---- one update at the block edges ----

@functools.lru_cache(maxsize=None)
def aggregate_normals():
    return unit_normals(len(fx.aggregate_target()), 11)


# ---- runs of 0, 1 and 5 updates ----

@functools.lru_cache(maxsize=None)
def margin_fixture():
    """test_icp_gpu._margin_fixture's construction with seeded unit normals on the lattice: (source, target, normals, r,
    inits, per init the yardstick's run of RUN_UPDATES updates).  The first seed whose every searched pose has the margin
    and whose A matrices meet the eigenvalue condition."""
    g = np.stack(np.meshgrid(*[np.arange(8) * 0.1] * 3, indexing="ij"), -1).reshape(-1, 3)
    for seed in range(50):
        rng = np.random.default_rng(seed)
        tgt = _f32(g + rng.uniform(-0.012, 0.012, g.shape))
        nrm = unit_normals(len(tgt), 100 + seed)
        a = np.deg2rad(3.0)
        R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        sub = tgt[rng.choice(len(tgt), 300, replace=False)].astype(np.float64)
        src = _f32((sub - 0.35) @ R + 0.35 + (0.01, -0.01, 0.005) + rng.normal(scale=0.002, size=sub.shape))
        r = 0.045
        inits = np.stack([np.eye(4)] * 3)
        inits[1, :3, 3] = (-0.008, 0.006, -0.004)
        b = np.deg2rad(-2.0)
        inits[2, :3, :3] = [[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]]
        runs = [pref.registration_icp(src, tgt, nrm, r, T0, max_iteration=RUN_UPDATES, relative_fitness=0.0, relative_rmse=0.0)
                for T0 in inits]
        poses = [T for y in runs for T in y["poses"]]
        if poses_have_margin(src, tgt, poses, r) and all(pref.eig_ratios_clear(y["eigenvalues"]) for y in runs):
            return src, tgt, nrm, r, inits, runs
    raise AssertionError("no seed gave the margin property")


# ---- rank-deficient systems ----

def _planar(seed):
    """A jittered 33 x 33 lattice in the plane z = 0 (spacing 0.03) and a translated copy of 400 of its points."""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(33) * 0.03, np.arange(33) * 0.03, indexing="ij"), -1).reshape(-1, 2)
    tgt = np.column_stack([g + rng.uniform(-0.005, 0.005, g.shape), np.zeros(len(g))])
    src = tgt[rng.choice(len(tgt), 400, replace=False)] + (0.004, -0.003, 0.01)
    return src, tgt, np.tile([0.0, 0.0, 1.0], (len(tgt), 1)), 0.05


def _one_source_point(seed):
    rng = np.random.default_rng(seed)
    tgt = rng.random((500, 3))
    return tgt[:1] + rng.normal(scale=0.01, size=(1, 3)), tgt, unit_normals(500, seed), 0.08


def _one_pair(seed):
    rng = np.random.default_rng(seed)
    tgt = rng.random((500, 3))
    src = np.concatenate([tgt[7:8] + rng.normal(scale=0.01, size=(1, 3)), 3.0 + rng.random((40, 3))])   # one point in reach
    return src, tgt, unit_normals(500, seed), 0.08


def _identical64(seed):
    rng = np.random.default_rng(seed)
    tgt = np.repeat(np.array([[0.3, -0.2, 0.5]]), 64, axis=0)
    src = tgt[:1] + rng.normal(scale=0.02, size=(30, 3))
    return src, tgt, np.tile(unit_normals(1, seed), (64, 1)), 0.2


RANK_DEFICIENT = {"planar": _planar, "one_source_point": _one_source_point, "one_pair": _one_pair, "identical64": _identical64}


@functools.lru_cache(maxsize=None)
def rank_deficient(name):
    """(source, target, normals, r, the yardstick's run of one update from the identity): the first seed with the
    margin at the searched poses and the eigenvalue condition."""
    for seed in range(50):
        src, tgt, nrm, r = RANK_DEFICIENT[name](seed)
        src, tgt, nrm = _f32(src), _f32(tgt), _f32(nrm)
        y = pref.registration_icp(src, tgt, nrm, r, np.eye(4), max_iteration=1, relative_fitness=0.0, relative_rmse=0.0)
        # (identical64: every target point is the same position, the pairing is the lowest index by rule)
        ok = name == "identical64" or poses_have_margin(src, tgt, y["poses"], r)
        if ok and pref.eig_ratios_clear(y["eigenvalues"]) and y["passes"][0] >= 1:
            return src, tgt, nrm, r, y
    raise AssertionError(f"{name}: no seed gave the fixture properties")


# ---- the planted pose ----

PLANTED_MAX_ITERATION = 200


@functools.lru_cache(maxsize=None)
def planted():
    """Target: asymmetric_object with yardstick-estimated normals.  Source: a copy 5 degrees and 2 % of the extent off.
    (source, target, normals, r, R0, t0, the point-to-plane yardstick's run, the point-to-point yardstick's run) of the
    first seed at which point-to-plane reaches the planted pose within 0.02 in strictly fewer updates than
    point-to-point."""
    for seed in range(20):
        tgt = _f32(ref.asymmetric_object(3000, seed))
        t64 = tgt.astype(np.float64)
        nrm = _f32(pref.estimate_normals(t64, 30))
        a = np.deg2rad(5.0)
        R0 = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        extent = float(np.ptp(t64, axis=0).max())
        t0 = 0.02 * extent * np.array([0.6, -0.64, 0.48])            # a vector of length 2 % of the extent
        src = _f32((t64 - t0) @ R0)                                   # q = R0 p + t0 maps it back
        r = float(np.ptp(t64, axis=0).mean() * 0.16)
        yp = pref.registration_icp(src, tgt, nrm, r, np.eye(4), max_iteration=PLANTED_MAX_ITERATION)
        y2 = ref.registration_icp(src, tgt, r, np.eye(4), max_iteration=PLANTED_MAX_ITERATION)
        T = yp["transformation"]
        if (np.abs(T[:3, :3] - R0).max() < 0.02 and np.abs(T[:3, 3] - t0).max() < 0.02
                and yp["iterations"] < y2["iterations"] and pref.eig_ratios_clear(yp["eigenvalues"])):
            return src, tgt, nrm, r, R0, t0, yp, y2
    raise AssertionError("no seed gave the planted-pose property")


# ---- normals ----

def _uniform(n):
    return lambda: np.random.default_rng(n).random((n, 3))


def _shifted_lattice():
    tgt, _, _ = fx._cube64(3)
    return tgt + np.array([1000.0, -1000.0, 1000.0])


# name -> (builder, knn, rows checked by brute force: None = all)
NORMALS = {
    "u255_k30": (_uniform(255), 30, None), "u256_k30": (_uniform(256), 30, None), "u257_k3": (_uniform(257), 3, None),
    "u257_k30": (_uniform(257), 30, None), "u257_k32": (_uniform(257), 32, None), "u40000_k30": (_uniform(40000), 30, 2000),
    "n20_k30": (_uniform(20), 30, None), "shifted_k30": (_shifted_lattice, 30, None),
}


@functools.lru_cache(maxsize=None)
def normals_fixture(name):
    """dict(points fp32, knn, rows = the points the brute force answers for, idx = their neighbours, margin = rows whose
    neighbour SET no rounding of size slack can change, normals = the yardstick's, gap = rows with the eigen-gap too)."""
    build, knn, sample = NORMALS[name]
    pts = _f32(build())
    n = len(pts)
    rows = np.arange(n) if sample is None else np.sort(np.random.default_rng(5).choice(n, sample, replace=False))
    idx, dk, dk1 = pref.knn_brute(pts, knn, rows)
    E = float(np.abs(pts.astype(np.float64) - fx.centre_of(pts)).max())
    margin = dk1 - dk > 2.0 * E * 2.0 ** -20
    nrm, lam = pref.normals_of(pts, idx)
    gap = margin & (lam[:, 1] - lam[:, 0] >= EIGEN_GAP * lam[:, 2])
    out = {"points": pts, "knn": knn, "rows": rows, "idx": idx, "margin": margin, "normals": nrm, "gap": gap}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
