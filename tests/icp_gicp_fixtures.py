"""Fixtures of the generalized ICP tests (tests/test_icp_gicp_cpu.py checks their properties with the float64 yardstick
alone; tests/test_icp_gicp_gpu.py asserts them again and then holds the kernels to the yardstick on them).  Seeded,
cached, read-only.  No GPU.  Every covariance is rounded to fp32 before the yardstick sees it.

Target covariances come from normals by the epsilon = 1e-3 rule (I - (1 - epsilon) n n^T).  Source covariances are a
DIFFERENT random symmetric positive definite matrix per point, condition number <= 1e3: a gather of them through the
wrong order cannot pass.  The conditions of tests/icp_plane_fixtures.py apply unchanged - an unambiguous pairing at every
pose the GENERALIZED yardstick searches, and no eigenvalue ratio of its A matrices within [1e-14, 1e-10].  The inits of
the margin fixture and the second start of the planted pair are rotated by ROTATED_DEGREES (>= 30): there A_T C_p A_T^T
is far from C_p."""
import functools

import numpy as np

from tests import icp_gicp_reference as gref
from tests import icp_plane_fixtures as pfx
from tests import icp_plane_reference as pref
from tests import icp_probe_fixtures as fx

EPSILON = 1e-3
CONDITION_CAP = 1e3
RUN_UPDATES = pfx.RUN_UPDATES
ROTATED_DEGREES = 40.0

_f32 = pfx._f32


def covariances_of_normals(normals, epsilon=EPSILON):
    """[n, 6] fp32: I - (1 - epsilon) n n^T in float64, then rounded."""
    n = np.asarray(normals, np.float64)
    C = np.eye(3)[None] - (1.0 - epsilon) * n[:, :, None] * n[:, None, :]
    return _f32(gref.pack(C))


def random_spd(n, seed):
    """[n, 6] fp32: per point Q diag(l) Q^T with a random rotation Q and eigenvalues whose ratio stays below 10^2.7, at
    an overall scale in [0.5, 2]."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    lam = 10.0 ** rng.uniform(-2.7, 0.0, (n, 3)) * rng.uniform(0.5, 2.0, (n, 1))
    return _f32(gref.pack(np.einsum("nab,nb,ncb->nac", Q, lam, Q)))


def condition_numbers(c6):
    lam = np.linalg.eigvalsh(gref.unpack(c6))
    return lam[:, 2] / lam[:, 0]


def rotation_about(axis, degrees):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(degrees)
    return np.eye(3) + np.sin(t) * K + (1.0 - np.cos(t)) * K @ K


def about(R, centre):
    """The 4x4 that rotates by R about `centre`."""
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = centre - R @ centre
    return T


def rotation_angle_degrees(R):
    return float(np.rad2deg(np.arccos(np.clip((np.trace(R) - 1.0) / 2.0, -1.0, 1.0))))


# ---- one update at the block edges ----

@functools.lru_cache(maxsize=None)
def aggregate_target_covariances():
    return covariances_of_normals(pfx.aggregate_normals())


@functools.lru_cache(maxsize=None)
def aggregate_source_covariances(ns):
    return random_spd(ns, 500 + ns)


# ---- runs of 0, 1 and 5 updates ----

@functools.lru_cache(maxsize=None)
def margin_fixture():
    """icp_plane_fixtures.margin_fixture's construction, the source turned back by ROTATED_DEGREES about the lattice's
    centre and every init turned forward by it, searched at the GENERALIZED yardstick's poses: (source, source
    covariances, target, target covariances, r, inits, per init the yardstick's run of RUN_UPDATES updates).  The first
    seed whose every searched pose has the margin and whose A matrices meet the eigenvalue condition."""
    g = np.stack(np.meshgrid(*[np.arange(8) * 0.1] * 3, indexing="ij"), -1).reshape(-1, 3)
    turn = about(rotation_about((1.0, 2.0, 3.0), ROTATED_DEGREES), np.full(3, 0.35))
    back = np.linalg.inv(turn)
    for seed in range(50):
        rng = np.random.default_rng(seed)
        tgt = _f32(g + rng.uniform(-0.012, 0.012, g.shape))
        Cq = covariances_of_normals(pfx.unit_normals(len(tgt), 100 + seed))
        a = np.deg2rad(3.0)
        R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        sub = tgt[rng.choice(len(tgt), 300, replace=False)].astype(np.float64)
        near = (sub - 0.35) @ R + 0.35 + (0.01, -0.01, 0.005) + rng.normal(scale=0.002, size=sub.shape)
        src = _f32(near @ back[:3, :3].T + back[:3, 3])
        Cp = random_spd(len(src), 200 + seed)
        r = 0.045
        inits = np.stack([np.eye(4)] * 3)
        inits[1, :3, 3] = (-0.008, 0.006, -0.004)
        b = np.deg2rad(-2.0)
        inits[2, :3, :3] = [[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]]
        inits = np.stack([T @ turn for T in inits])
        runs = [gref.registration_icp(src, tgt, Cp, Cq, r, T0, max_iteration=RUN_UPDATES, relative_fitness=0.0, relative_rmse=0.0)
                for T0 in inits]
        poses = [T for y in runs for T in y["poses"]]
        if pfx.poses_have_margin(src, tgt, poses, r) and all(pref.eig_ratios_clear(y["eigenvalues"]) for y in runs):
            inits.setflags(write=False)
            return src, Cp, tgt, Cq, r, inits, runs
    raise AssertionError("no seed gave the margin property")


def first_pairs(src, tgt, T0, r):
    """(x of the pairs, source index of the pairs, target index of the pairs) of the float64 brute force under T0."""
    x = np.asarray(src, np.float64) @ T0[:3, :3].T + T0[:3, 3]
    i1, d1, _, _ = fx.brute_nearest(tgt, x)
    hit = d1 <= r
    return x[hit], np.flatnonzero(hit), i1[hit]


def one_update_bound(xs, qs, Cs, Cq, ct, s, T0, extent, rng):
    """(the yardstick's transformation after one update, the bound on |GPU - yardstick|, the yardstick's own sensitivity to
    the order of its pairs, its sensitivity to the inverse).  The bound is the largest of 10x either sensitivity and the
    floor 1e-13 (1 + extent): test_icp_plane_gpu._one_update_bound's rule with the inverse's term added.  Both
    sensitivities are measured on the yardstick alone."""
    want = gref.reference_update(xs, qs, Cs, Cq, ct, s) @ T0
    perm = rng.permutation(len(xs))
    own = float(np.abs(gref.reference_update(xs[perm], qs[perm], Cs[perm], Cq[perm], ct, s) @ T0 - want).max())
    inv = float(np.abs(gref.reference_update(xs, qs, Cs, Cq, ct, s, inverse="numpy") @ T0 - want).max())
    return want, max(10.0 * own, 10.0 * inv, 1e-13 * (1.0 + extent)), own, inv


def first_pass(src, Cp, tgt, Cq, r, T0, rotate_source=True):
    """(xs, qs, rotated source covariances, target covariances) of the brute-force pairs under T0."""
    xs, si, ti = first_pairs(src, tgt, T0, r)
    C = gref.unpack(Cp)[si]
    return xs, tgt.astype(np.float64)[ti], (gref.rotate(C, T0[:3, :3]) if rotate_source else C), gref.unpack(Cq)[ti]


@functools.lru_cache(maxsize=None)
def quarter_zero():
    """The margin fixture with a seeded quarter of the source covariances zero and the target covariances of their
    partners under every init's first pass zero too: those pairs have M = 0 and must add nothing to the update.
    (source covariances, target covariances, per init the source indices zeroed that found a partner)."""
    src, Cp, tgt, Cq, r, inits, _ = margin_fixture()
    Cp, Cq = np.array(Cp), np.array(Cq)
    zero = np.random.default_rng(9).choice(len(src), len(src) // 4, replace=False)
    Cp[zero] = 0.0
    hit = []
    for T0 in inits:
        _, si, ti = first_pairs(src, tgt, T0, r)
        sel = np.isin(si, zero)
        Cq[ti[sel]] = 0.0
        hit.append(si[sel])
    return _f32(Cp), _f32(Cq), hit


# ---- degenerate systems ----

RANK_DEFICIENT = ("one_source_point", "one_pair", "identical64")


@functools.lru_cache(maxsize=None)
def rank_deficient(name):
    """icp_plane_fixtures.RANK_DEFICIENT's clouds with covariances: (source, source covariances, target, target
    covariances, r, the yardstick's run of one update from the identity), the first seed with the margin at the
    searched poses and the eigenvalue condition."""
    for seed in range(50):
        src, tgt, nrm, r = pfx.RANK_DEFICIENT[name](seed)
        src, tgt = _f32(src), _f32(tgt)
        Cp, Cq = random_spd(len(src), 300 + seed), covariances_of_normals(_f32(nrm))
        y = gref.registration_icp(src, tgt, Cp, Cq, r, np.eye(4), max_iteration=1, relative_fitness=0.0, relative_rmse=0.0)
        ok = name == "identical64" or pfx.poses_have_margin(src, tgt, y["poses"], r)
        if ok and pref.eig_ratios_clear(y["eigenvalues"]) and y["passes"][0] >= 1:
            return src, Cp, tgt, Cq, r, y
    raise AssertionError(f"{name}: no seed gave the fixture properties")


# ---- the planted pose ----

@functools.lru_cache(maxsize=None)
def planted():
    """icp_plane_fixtures.planted() with covariances from yardstick normals of both clouds (knn 30, epsilon 1e-3), and a
    second start: the source turned back by ROTATED_DEGREES about the target's centroid, with the covariances of ITS
    normals, from the init that turns it forward again.  dict(target, target_covariances, r, R0, t0, plane, point = the
    yardsticks' runs of the other two estimators, starts = [(source, source covariances, init, planted 4x4, the
    generalized yardstick's run)])."""
    src, tgt, nrm, r, R0, t0, yp, y2 = pfx.planted()
    Cq = covariances_of_normals(nrm)
    want = np.eye(4)
    want[:3, :3], want[:3, 3] = R0, t0
    turn = about(rotation_about((2.0, -1.0, 2.0), ROTATED_DEGREES), tgt.astype(np.float64).mean(axis=0))
    back = np.linalg.inv(turn)
    starts = []
    for s, T0, W in ((src, np.eye(4), want), (_f32(src.astype(np.float64) @ back[:3, :3].T + back[:3, 3]), turn, want @ turn)):
        Cp = covariances_of_normals(_f32(pref.estimate_normals(s.astype(np.float64), 30)))
        y = gref.registration_icp(s, tgt, Cp, Cq, r, T0, max_iteration=pfx.PLANTED_MAX_ITERATION)
        starts.append((s, Cp, T0, W, y))
    return {"target": tgt, "target_covariances": Cq, "r": r, "R0": R0, "t0": t0, "plane": yp, "point": y2, "starts": starts}
