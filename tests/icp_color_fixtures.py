"""Fixtures of the coloured ICP and colour-gradient tests (tests/test_icp_color_cpu.py checks their properties with the
float64 yardstick alone; tests/test_icp_color_gpu.py and tests/test_color_gradients_gpu.py assert them again and then hold
the kernels to the yardstick on them).  Seeded, cached, read-only.  No GPU.  Every attribute is rounded to fp32 before the
yardstick sees it.

Target attributes of the number-for-number fixtures: random intensities in [0, 1] and random tangent gradients of length
0.5 - 4 on seeded unit normals.  Source intensities are a DIFFERENT random value per point (the aggregate and rank-deficient
fixtures) or that of the lattice point a source point was drawn from plus gradient times its offset plus noise (the margin
fixture): a gather of them through the wrong order cannot pass.  The conditions of tests/icp_plane_fixtures.py apply
unchanged - an unambiguous pairing at every pose the COLOURED yardstick searches, and no eigenvalue ratio of its A
matrices, nor of the gradient rule's M, within [1e-14, 1e-10]."""
import functools

import numpy as np

from tests import icp_color_reference as cref
from tests import icp_plane_fixtures as pfx
from tests import icp_plane_reference as pref
from tests import icp_probe_fixtures as fx

LAMBDAS = (0.968, 0.5)
RUN_UPDATES = pfx.RUN_UPDATES
MARGIN_CAP = pfx.MARGIN_CAP

_f32 = pfx._f32


def tangent_gradients(normals, seed, lo=0.5, hi=4.0):
    """[n, 3] fp32: per point a random direction orthogonal to its normal (any direction for a zero normal), of a length
    uniform in [lo, hi]."""
    rng = np.random.default_rng(seed)
    n = np.asarray(normals, np.float64)
    v = rng.normal(size=n.shape)
    v -= (v * n).sum(axis=1, keepdims=True) * n
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return _f32(v * rng.uniform(lo, hi, (len(n), 1)))


def random_intensity(n, seed):
    return _f32(np.random.default_rng(seed).random(n))


def smooth_texture(points):
    """[n] float64 in [0.05, 0.95]: a smooth texture function of position, for clouds that bring no colour (the planted
    pair of icp_plane_fixtures, the scripts' asymmetric object)."""
    p = np.asarray(points, np.float64)
    return 0.5 + 0.3 * np.sin(5.0 * p[:, 0] + 0.3) * np.sin(4.0 * p[:, 1] - 0.2) + 0.15 * np.sin(6.0 * p[:, 2] + 1.0)


def target_attributes(normals, seed):
    """(intensity [n], gradients [n, 3]) of a target with the given normals."""
    return random_intensity(len(normals), seed), tangent_gradients(normals, seed + 1)


# ---- one update at the block edges ----

@functools.lru_cache(maxsize=None)
def aggregate_target_attributes():
    return target_attributes(pfx.aggregate_normals(), 700)


@functools.lru_cache(maxsize=None)
def aggregate_source_intensity(ns):
    return random_intensity(ns, 800 + ns)


def first_pairs(src, tgt, T0, r):
    """(x of the pairs, source index of the pairs, target index of the pairs) of the float64 brute force under T0."""
    x = np.asarray(src, np.float64) @ T0[:3, :3].T + T0[:3, 3]
    i1, d1, _, _ = fx.brute_nearest(tgt, x)
    hit = d1 <= r
    return x[hit], np.flatnonzero(hit), i1[hit]


def first_pass(src, Ip, tgt, nrm, Iq, grad, r, T0):
    """(xs, qs, normals, gradients, I_q, I_p) of the brute-force pairs under T0, float64."""
    xs, si, ti = first_pairs(src, tgt, T0, r)
    f = lambda a: np.asarray(a, np.float64)
    return xs, f(tgt)[ti], f(nrm)[ti], f(grad)[ti], f(Iq)[ti], f(Ip)[si]


def one_update_bound(pairs, lam, ct, s, T0, extent, rng):
    """(the yardstick's transformation after one update, the bound on |GPU - yardstick|, the yardstick's own sensitivity to
    the order of its pairs).  The bound is the larger of 10x that sensitivity and the floor 1e-13 (1 + extent):
    icp_gicp_fixtures.one_update_bound's rule without the inverse's term (there is no inverse here).  Measured on the
    yardstick alone."""
    want = cref.reference_update(*pairs, lam, ct, s) @ T0
    perm = rng.permutation(len(pairs[0]))
    own = float(np.abs(cref.reference_update(*(a[perm] for a in pairs), lam, ct, s) @ T0 - want).max())
    return want, max(10.0 * own, 1e-13 * (1.0 + extent)), own


# ---- runs of 0, 1 and 5 updates ----

def _run(src, Ip, tgt, nrm, Iq, grad, r, T0, lam, n=RUN_UPDATES):
    return cref.registration_icp(src, Ip, tgt, nrm, Iq, grad, r, T0, lam, max_iteration=n, relative_fitness=0.0,
                                 relative_rmse=0.0)


@functools.lru_cache(maxsize=None)
def margin_fixture():
    """icp_plane_fixtures.margin_fixture's construction with target attributes; the source intensity is that of the
    lattice point it was drawn from, plus gradient times its offset, plus noise 0.002.  (source, source intensity, target,
    normals, target intensity, gradients, r, inits, {lambda: per init the yardstick's run of RUN_UPDATES updates}).  The
    first seed whose every searched pose, at every lambda of LAMBDAS, has the margin and whose A matrices meet the
    eigenvalue condition."""
    g = np.stack(np.meshgrid(*[np.arange(8) * 0.1] * 3, indexing="ij"), -1).reshape(-1, 3)
    for seed in range(50):
        rng = np.random.default_rng(seed)
        tgt = _f32(g + rng.uniform(-0.012, 0.012, g.shape))
        nrm = pfx.unit_normals(len(tgt), 100 + seed)
        Iq, grad = target_attributes(nrm, 400 + seed)
        a = np.deg2rad(3.0)
        R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        pick = rng.choice(len(tgt), 300, replace=False)
        sub = tgt[pick].astype(np.float64)
        off = rng.normal(scale=0.002, size=sub.shape)
        src = _f32((sub - 0.35) @ R + 0.35 + (0.01, -0.01, 0.005) + off)
        # the offset in the target's frame: the move undone
        Ip = _f32(Iq[pick].astype(np.float64) + (grad[pick].astype(np.float64) * (off @ R.T)).sum(axis=1)
                  + rng.normal(scale=0.002, size=len(sub)))
        r = 0.045
        inits = np.stack([np.eye(4)] * 3)
        inits[1, :3, 3] = (-0.008, 0.006, -0.004)
        b = np.deg2rad(-2.0)
        inits[2, :3, :3] = [[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]]
        runs = {lam: [_run(src, Ip, tgt, nrm, Iq, grad, r, T0, lam) for T0 in inits] for lam in LAMBDAS}
        every = [y for ys in runs.values() for y in ys]
        poses = [T for y in every for T in y["poses"]]
        if pfx.poses_have_margin(src, tgt, poses, r) and all(pref.eig_ratios_clear(y["eigenvalues"]) for y in every):
            inits.setflags(write=False)
            return src, Ip, tgt, nrm, Iq, grad, r, inits, runs
    raise AssertionError("no seed gave the margin property")


@functools.lru_cache(maxsize=None)
def quarter_zero():
    """The margin fixture with a seeded quarter of the target normals zero (their pairs add the colour term only) and
    another quarter of the target gradients zero, the source points paired with those given their partner's intensity
    (the geometric term only).  (source intensity, normals, gradients, the target indices without a normal, those without
    a gradient)."""
    src, Ip, tgt, nrm, Iq, grad, r, inits, _ = margin_fixture()
    Ip, nrm, grad = np.array(Ip), np.array(nrm), np.array(grad)
    order = np.random.default_rng(9).permutation(len(tgt))
    no_normal, no_gradient = np.sort(order[:len(tgt) // 4]), np.sort(order[len(tgt) // 4:len(tgt) // 2])
    nrm[no_normal] = 0.0
    grad[no_gradient] = 0.0
    partner = np.full(len(src), -1)
    for T0 in inits:
        _, si, ti = first_pairs(src, tgt, T0, r)
        assert ((partner[si] == -1) | (partner[si] == ti)).all()      # one partner per source point under every init
        partner[si] = ti
    sel = np.isin(partner, no_gradient)
    Ip[sel] = Iq[partner[sel]]
    return _f32(Ip), _f32(nrm), _f32(grad), no_normal, no_gradient


# ---- degenerate systems ----

RANK_DEFICIENT = ("one_source_point", "one_pair", "identical64", "planar")


@functools.lru_cache(maxsize=None)
def rank_deficient(name, lam=LAMBDAS[0]):
    """icp_plane_fixtures.RANK_DEFICIENT's clouds with colours: (source, source intensity, target, normals, target
    intensity, gradients, r, the yardstick's run of one update from the identity), the first seed with the margin at the
    searched poses and the eigenvalue condition."""
    for seed in range(50):
        src, tgt, nrm, r = pfx.RANK_DEFICIENT[name](seed)
        src, tgt, nrm = _f32(src), _f32(tgt), _f32(nrm)
        Iq, grad = target_attributes(nrm, 600 + seed)
        Ip = random_intensity(len(src), 650 + seed)
        y = _run(src, Ip, tgt, nrm, Iq, grad, r, np.eye(4), lam, 1)
        ok = name == "identical64" or pfx.poses_have_margin(src, tgt, y["poses"], r)
        if ok and pref.eig_ratios_clear(y["eigenvalues"]) and y["passes"][0] >= 1:
            return src, Ip, tgt, nrm, Iq, grad, r, y
    raise AssertionError(f"{name}: no seed gave the fixture properties")


# ---- the textured sheet ----

SHEET_R = 0.06
SHEET_KNN = 20
SHEET_MAX_ITERATION = 100


def sheet_height(x):
    return 0.02 * np.sin(3.0 * x)


def sheet_texture(x, y):
    """A smooth texture with several periods across the unit sheet: a sum of products of sines, within [0.1, 0.9]."""
    return 0.5 + 0.22 * np.sin(2 * np.pi * 3.0 * x + 0.4) * np.sin(2 * np.pi * 2.0 * y + 1.1) \
        + 0.18 * np.sin(2 * np.pi * 1.5 * x - 0.7) * np.sin(2 * np.pi * 3.5 * y + 0.3)


def sheet_truth():
    """The planted pose: 2 degrees about z through the sheet's centre, then (0.03, -0.02, 0.004)."""
    a = np.deg2rad(2.0)
    T = np.eye(4)
    T[:3, :3] = [[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]
    c = np.array([0.4875, 0.4875, 0.0])
    T[:3, 3] = c - T[:3, :3] @ c + (0.03, -0.02, 0.004)
    return T


def rms_alignment_error(T, src, want=None):
    """RMS over the source points of |T p - T_true p|."""
    want = sheet_truth() if want is None else want
    p = np.asarray(src, np.float64)
    return float(np.sqrt((((p @ T[:3, :3].T + T[:3, 3]) - (p @ want[:3, :3].T + want[:3, 3])) ** 2).sum(axis=1).mean()))


@functools.lru_cache(maxsize=None)
def textured_sheet():
    """Target: a 40 x 40 lattice (spacing 0.025, jitter 0.006) on z = 0.02 sin(3 x) with sheet_texture, normals and
    gradients by the yardstick at knn 20.  Source: 900 independent samples of the inner 70 % with their own texture values,
    moved off by the inverse of sheet_truth().  dict(source, source_intensity, target, normals, target_intensity, gradients,
    r, truth, start = the RMS alignment error at the identity, colored = {lambda: the coloured yardstick's run}, plane = the
    point-to-plane yardstick's run) of the first seed at which, at every lambda of LAMBDAS, the coloured yardstick's RMS
    alignment error is below a tenth of the point-to-plane yardstick's and the search margins hold at its poses
    (icp_probe_fixtures.has_margin, as for the aggregate fixtures: 900 independent samples at several poses cannot all
    keep the relative margin of test_icp_gpu._margin_ok as well)."""
    want = sheet_truth()
    back = np.linalg.inv(want)
    for seed in range(20):
        rng = np.random.default_rng(seed)
        g = np.stack(np.meshgrid(np.arange(40) * 0.025, np.arange(40) * 0.025, indexing="ij"), -1).reshape(-1, 2)
        xy = g + rng.uniform(-0.006, 0.006, g.shape)
        tgt = _f32(np.column_stack([xy, sheet_height(xy[:, 0])]))
        t64 = tgt.astype(np.float64)
        Iq = _f32(sheet_texture(t64[:, 0], t64[:, 1]))
        nrm = _f32(pref.estimate_normals(t64, SHEET_KNN))
        grad = _f32(cref.estimate_color_gradients(t64, Iq.astype(np.float64), nrm.astype(np.float64), SHEET_KNN)[0])
        lo, hi = 0.15 * 0.975, 0.85 * 0.975
        sxy = rng.uniform(lo, hi, (900, 2))
        samples = np.column_stack([sxy, sheet_height(sxy[:, 0])])
        Ip = _f32(sheet_texture(sxy[:, 0], sxy[:, 1]))
        src = _f32(samples @ back[:3, :3].T + back[:3, 3])
        yp = pref.registration_icp(src, tgt, nrm, SHEET_R, np.eye(4), max_iteration=SHEET_MAX_ITERATION)
        yc = {lam: cref.registration_icp(src, Ip, tgt, nrm, Iq, grad, SHEET_R, np.eye(4), lam, max_iteration=SHEET_MAX_ITERATION)
              for lam in LAMBDAS}
        ep = rms_alignment_error(yp["transformation"], src)
        if (all(rms_alignment_error(y["transformation"], src) < 0.1 * ep and y["iterations"] < SHEET_MAX_ITERATION
                and pref.eig_ratios_clear(y["eigenvalues"]) and pfx.poses_have_margin(src, tgt, y["poses"], SHEET_R, relative=False)
                for y in yc.values())):
            return {"source": src, "source_intensity": Ip, "target": tgt, "normals": nrm, "target_intensity": Iq,
                    "gradients": grad, "r": SHEET_R, "truth": want, "start": rms_alignment_error(np.eye(4), src),
                    "colored": yc, "plane": yp, "seed": seed}
    raise AssertionError("no seed gave the textured-sheet property")


# ---- colour gradients ----

def _pad(idx, knn):
    nb = np.full((len(idx), knn), -1, np.int32)
    nb[:, :idx.shape[1]] = idx
    nb.setflags(write=False)
    return nb


def gradient_order_sensitivity(points, normals, intensity, neighbors, rows, want, rng):
    """Per row: the largest change of the yardstick's gradient when the row's entries are shuffled."""
    shuffled = np.array([rng.permutation(r) for r in neighbors])
    return np.abs(cref.color_gradients(points, normals, intensity, shuffled, rows) - want).max(axis=1)


def gradient_bound(want, sensitivity):
    """Per row: the larger of 10x the yardstick's sensitivity to the neighbour order and one fp32 ulp of the row's largest
    component (the store rounds to fp32)."""
    return np.maximum(10.0 * sensitivity, np.spacing(np.abs(want).max(axis=1).astype(np.float32)).astype(np.float64))


def _plane_linear():
    """An axis-aligned plane z = 0.25 with the linear intensity I = 0.25 + slope . p, exact in fp32 (coordinates on a
    2^-16 raster, a dyadic slope): (points, normals, intensity, knn, slope).  The slope has a normal component, which the
    rule must drop."""
    rng = np.random.default_rng(3)
    pts = _f32(np.column_stack([rng.integers(0, 65536, (300, 2)) / 65536.0, np.full(300, 0.25)]))
    slope = np.array([1.5, -0.75, 2.0])
    inten = 0.25 + pts.astype(np.float64) @ slope
    assert np.array_equal(inten, inten.astype(np.float32).astype(np.float64))
    return pts, _f32(np.tile([0.0, 0.0, 1.0], (300, 1))), inten, 12, slope


def _line():
    """Points on the line along (3, 4, 0) / 5 with a linear intensity, all exact in fp32, the normal (0, 0, 1) orthogonal
    to it: (points, normals, intensity, knn, slope, direction)."""
    rng = np.random.default_rng(4)
    t = np.sort(rng.choice(65536, 200, replace=False)) / 65536.0
    pts = _f32(t[:, None] * np.array([0.375, 0.5, 0.0]))
    slope = np.array([0.5, -1.0, 2.0])
    inten = 0.125 + pts.astype(np.float64) @ slope
    assert np.array_equal(inten, inten.astype(np.float32).astype(np.float64))
    return pts, _f32(np.tile([0.0, 0.0, 1.0], (200, 1))), inten, 8, slope, np.array([0.6, 0.8, 0.0])


@functools.lru_cache(maxsize=None)
def gradient_fixture(name):
    """dict(points, normals, intensity fp32; knn; rows = the points the yardstick answers for; neighbors = the yardstick's
    lists of those rows, padded with -1; margin = rows whose neighbour SET no rounding of size slack can change;
    gradients, eigenvalues = the yardstick's; sensitivity = its own to the order of a row).  Names: plane_linear, line,
    one_neighbour, knn_over_n, and u<n> for the normals_fixture clouds of 255, 256, 257 and 40000 points."""
    rng = np.random.default_rng(17)
    extra = {}
    if name.startswith("u"):
        f = pfx.normals_fixture(f"{name}_k30")
        pts, knn, rows, idx, margin = f["points"], f["knn"], f["rows"], f["idx"], f["margin"]
        nrm = pfx.unit_normals(len(pts), 900 + len(pts))
        inten = random_intensity(len(pts), 950 + len(pts))
    else:
        if name == "plane_linear":
            pts, nrm, inten, knn, extra["slope"] = _plane_linear()
        elif name == "line":
            pts, nrm, inten, knn, extra["slope"], extra["axis"] = _line()
        elif name == "one_neighbour":
            pts = _f32([[0.1, 0.2, 0.3], [0.15, 0.2, 0.35]])
            nrm, inten, knn = _f32([[0.0, 0.0, 1.0]] * 2), np.array([0.2, 0.9]), 3
        elif name == "knn_over_n":
            pts = _f32(np.random.default_rng(5).random((20, 3)))
            nrm, inten, knn = pfx.unit_normals(20, 6), np.random.default_rng(7).random(20), 30
        else:
            raise KeyError(name)
        inten = _f32(inten)
        rows = np.arange(len(pts))
        idx, dk, dk1 = pref.knn_brute(pts, knn)
        E = float(np.abs(pts.astype(np.float64) - fx.centre_of(pts)).max())
        margin = dk1 - dk > 2.0 * E * 2.0 ** -20
    nb = _pad(idx, knn)
    want, eig = cref.color_gradients(pts, nrm, inten, nb, rows, return_eig=True)
    out = {"points": pts, "normals": nrm, "intensity": inten, "knn": knn, "rows": rows, "neighbors": nb, "margin": margin,
           "gradients": want, "eigenvalues": eig,
           "sensitivity": gradient_order_sensitivity(pts, nrm, inten, nb, rows, want, rng), **extra}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


GRADIENTS = ("plane_linear", "line", "one_neighbour", "knn_over_n", "u255", "u256", "u257", "u40000")
