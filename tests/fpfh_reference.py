"""The yardstick of the global-registration kernels (csrc/cloud_fpfh.hip, csrc/feature_match.hip): rules F1 - F5 and M1 of
the global-registration block of include/scorp_gs.h as a float64 brute force in numpy - every pair's d^2, no grid - and the
RANSAC driver of scorp_amd/global_registration.py on numpy's SVD.  Operations are taken elementwise over arrays of pairs,
which rounds each product, sum, quotient and square root on its own exactly as a scalar loop would; wherever the ORDER of a
sum matters (d^2, the dot products, F5's run down the list, the blocks' totals, M1) the sum is written out term by term or
looped, never handed to np.sum, whose pairwise summation would change it.  Nothing here imports scorp_amd."""
import numpy as np

BINS, DIM = 11, 33
MARGIN = 1e-9      # a bin coordinate closer than this to an integer: atan2's last place may decide the bin
TWO_PI = 2.0 * np.pi


def _f64(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def d2_all(P):
    """R1 for every pair: (dx dx + dy dy) + dz dz"""
    P = _f64(P)
    d = P[:, None, :] - P[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def neighbors(P, radius, max_nn):
    """F1: (neighbours [n, max_nn] int32 padded with -1, degree [n] int32, their d2 [n, max_nn], 0 where padded)"""
    n = len(P)
    r2 = np.float64(radius) * np.float64(radius)
    D = d2_all(P)
    nb = np.full((n, max_nn), -1, np.int32)
    deg = np.zeros(n, np.int32)
    nd = np.zeros((n, max_nn))
    index = np.arange(n)
    for i in range(n):
        member = (D[i] <= r2) & (index != i)          # self is left out by index: a duplicate stays
        cand = index[member]
        order = cand[np.lexsort((cand, D[i][cand]))][:max_nn]   # ascending (d2, j)
        deg[i] = len(order)
        nb[i, :len(order)] = order
        nd[i, :len(order)] = D[i][order]
    return nb, deg, nd


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def pair_features(P, N, i, j):
    """F2 and F3 for the pairs (i[k], j[k]): dict of has [K] bool (the pair has a feature), f [K, 3] = (f1, f2, f3),
    x [K, 3] the three bin coordinates before the floor, bins [K, 3] int, margin [K, 3] = |x - nearest integer| and
    gap [K] = ||a1| - |a2||.  Rows without a feature hold zeros, margin +inf."""
    P, N = _f64(P), _f64(N)
    K = len(i)
    pi, pj, ni, nj = P[i], P[j], N[i], N[j]
    dp = pj - pi
    d2 = (dp[:, 0] * dp[:, 0] + dp[:, 1] * dp[:, 1]) + dp[:, 2] * dp[:, 2]
    f4 = np.sqrt(d2)
    has = f4 != 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        a1 = _dot(ni, dp) / f4
        a2 = _dot(nj, dp) / f4
        swap = np.abs(a1) < np.abs(a2)
        u = np.where(swap[:, None], nj, ni)
        n2 = np.where(swap[:, None], ni, nj)
        dq = np.where(swap[:, None], -dp, dp)
        f3 = np.where(swap, -a2, a1)
        v = _cross(dq, u)
        vn = np.sqrt(_dot(v, v))
        has &= vn != 0.0
        v = v / vn[:, None]
        w = _cross(u, v)
        f2 = _dot(v, n2)
        f1 = np.arctan2(_dot(w, n2), _dot(u, n2))
        x = np.stack([(11.0 * (f1 + np.pi)) / TWO_PI, 11.0 * ((f2 + 1.0) * 0.5), 11.0 * ((f3 + 1.0) * 0.5)], axis=1)
        gap = np.abs(np.abs(a1) - np.abs(a2))
    x = np.where(has[:, None], x, 0.0)
    bins = np.clip(np.floor(x), 0, 10).astype(np.int64)
    margin = np.where(has[:, None], np.abs(x - np.rint(x)), np.inf)
    f = np.where(has[:, None], np.stack([f1, f2, f3], axis=1), 0.0)
    return {"has": has, "f": f, "x": x, "bins": bins, "margin": margin, "gap": np.where(has, gap, 0.0)}


def fpfh(P, N, radius, max_nn):
    """F1 - F5.  dict: feature [n, 33] float64, count [n, 33] int32, neighbors, degree, spfh [n, 33], pair_margin
    [n, max_nn, 3] (+inf where there is no pair or no feature), pair_gap [n, max_nn], excluded [n] bool (a pair of the
    point's own list has a bin coordinate within MARGIN of an integer), feature_ok [n] bool (the point is not excluded and
    neither its own list nor its neighbours' lists hold an excluded point), pairs = the number of (i, j) pairs."""
    n = len(P)
    nb, deg, nd = neighbors(P, radius, max_nn)
    ii, aa = np.nonzero(nb >= 0)
    jj = nb[ii, aa].astype(np.int64)
    pf = pair_features(P, N, ii, jj)
    count = np.zeros((n, DIM), np.int32)
    for k in range(3):
        np.add.at(count, (ii[pf["has"]], BINS * k + pf["bins"][pf["has"], k]), 1)   # integers: the order is free
    margin = np.full((n, max_nn, 3), np.inf)
    margin[ii, aa] = pf["margin"]
    gap = np.zeros((n, max_nn))
    gap[ii, aa] = pf["gap"]
    excluded = (margin < MARGIN).any(axis=(1, 2))
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.where(deg > 0, 100.0 / deg.astype(np.float64), 0.0)
    spfh = count.astype(np.float64) * scale[:, None]
    s = np.zeros((n, DIM))
    for a in range(max_nn):                              # F5: down the list, in list order
        j = nb[:, a]
        use = (j >= 0) & (nd[:, a] > 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            term = spfh[np.where(use, j, 0)] / nd[:, a][:, None]
        s = np.where(use[:, None], s + term, s)
    for k in range(3):
        t = np.zeros(n)
        for e in range(BINS):                            # ascending from 0.0
            t = t + s[:, BINS * k + e]
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.where(t != 0.0, 100.0 / t, 1.0)
        s[:, BINS * k:BINS * (k + 1)] = np.where((t != 0.0)[:, None], s[:, BINS * k:BINS * (k + 1)] * f[:, None],
                                                 s[:, BINS * k:BINS * (k + 1)])
    feature = s + spfh
    listed = nb >= 0
    safe = np.where(listed, nb, 0)
    list_clean = ~(excluded[safe] & listed).any(axis=1)              # no excluded point in the point's own list
    nb_lists_clean = (list_clean[safe] | ~listed).all(axis=1)        # ... nor in its neighbours' lists
    feature_ok = ~excluded & list_clean & nb_lists_clean
    return {"feature": feature, "count": count, "neighbors": nb, "degree": deg, "spfh": spfh, "pair_margin": margin,
            "pair_gap": gap, "excluded": excluded, "feature_ok": feature_ok, "pairs": len(ii)}


def match(src, tgt, chunk=256):
    """M1: (index [ns] int32, D2 [ns] float64) of the target row of smallest (D2, index) per source row; the rows are
    rounded to float32 once, D2 is summed for k = 0 .. 32 in ascending order from 0.0."""
    S = np.asarray(src).astype(np.float32).astype(np.float64)
    T = np.asarray(tgt).astype(np.float32).astype(np.float64)
    index = np.empty(len(S), np.int32)
    best = np.empty(len(S))
    for lo in range(0, len(S), chunk):
        acc = np.zeros((min(chunk, len(S) - lo), len(T)))
        for k in range(S.shape[1]):
            d = S[lo:lo + chunk, k, None] - T[None, :, k]
            acc = acc + d * d
        arg = acc.argmin(axis=1)                          # the first minimum: the lowest index
        index[lo:lo + chunk] = arg
        best[lo:lo + chunk] = acc[np.arange(len(arg)), arg]
    return index, best


def match_mutual(src, tgt):
    """(index, D2, mutual [ns] bool): mutual[i] = back[index[i]] == i, back the match with the roles swapped"""
    index, d2 = match(src, tgt)
    back, _ = match(tgt, src)
    return index, d2, back[index] == np.arange(len(index))


def orient_away(P, N, center=None):
    P64 = np.asarray(P, dtype=np.float64)
    c = P64.sum(0) / len(P64) if center is None else np.asarray(center, dtype=np.float64)
    d = P64 - c
    N64 = np.asarray(N, dtype=np.float64)
    dot = (N64[:, 0] * d[:, 0] + N64[:, 1] * d[:, 1]) + N64[:, 2] * d[:, 2]
    return np.where((dot < 0)[:, None], -np.asarray(N), np.asarray(N))


def edge_length_mask(S, T, tri, thr):
    S, T = np.asarray(S, np.float64), np.asarray(T, np.float64)
    ok = np.ones(len(tri), bool)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        ls = np.linalg.norm(S[tri[:, a]] - S[tri[:, b]], axis=1)
        lt = np.linalg.norm(T[tri[:, a]] - T[tri[:, b]], axis=1)
        ok &= (ls >= thr * lt) & (lt >= thr * ls)
    return ok


def kabsch(S, T):
    """(R, t) of T ~ R S + t, the pose fit's rule: cov = sum (s - sm)(t - tm)^T = U S V^T, R = V D U^T"""
    sm, tm = S.mean(0), T.mean(0)
    U, _, Vt = np.linalg.svd((S - sm).T @ (T - tm))
    D = np.diag([1.0, 1.0, -1.0 if np.linalg.det(U @ Vt) < 0 else 1.0])
    R = Vt.T @ D @ U.T
    return R, tm - R @ sm


def correspondences(src_feature, tgt_feature, mutual_filter=True):
    index, _, mutual = match_mutual(src_feature, tgt_feature)
    src = np.arange(len(index))
    if mutual_filter and mutual.sum() >= 3:
        src = src[mutual]
    return np.stack([src, index[src].astype(np.int64)], axis=1)


def ransac(source, target, src_feature, tgt_feature, distance, samples, mutual_filter=True, edge_length_threshold=0.9):
    """The driver of registration_ransac_based_on_feature_matching: dict(transformation, inlier_count, fitness,
    correspondences, inlier_mask, counts)."""
    corr = correspondences(src_feature, tgt_feature, mutual_filter)
    S, T = np.asarray(source, np.float64)[corr[:, 0]], np.asarray(target, np.float64)[corr[:, 1]]
    tri = np.asarray(samples, dtype=np.int64)
    tri = tri[(tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 0] != tri[:, 2])]
    tri = tri[edge_length_mask(S, T, tri, edge_length_threshold)]
    if len(tri) == 0:
        raise ValueError("no sample triple passes the distinct-index and edge-length checks")
    counts = np.zeros(len(tri), np.int32)
    for h, t3 in enumerate(tri):
        R, t = kabsch(S[t3], T[t3])
        counts[h] = (np.linalg.norm(S @ R.T + t - T, axis=1) < distance).sum()
    win = int(np.argmax(counts))                          # the first with the highest count
    R, t = kabsch(S[tri[win]], T[tri[win]])
    mask = np.linalg.norm(S @ R.T + t - T, axis=1) < distance
    if mask.sum() < 3:
        raise ValueError("No inliers found in RANSAC.")
    R, t = kabsch(S[mask], T[mask])
    M = np.eye(4)
    M[:3, :3], M[:3, 3] = R, t
    return {"transformation": M, "inlier_count": int(counts[win]), "fitness": counts[win] / len(corr), "correspondences": corr,
            "inlier_mask": mask, "counts": counts}


def pose_error(M, M_true):
    """(rotation error in degrees, translation error) of M against M_true"""
    dR = M[:3, :3] @ M_true[:3, :3].T
    ang = np.degrees(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0)))
    return float(ang), float(np.linalg.norm(M[:3, 3] - M_true[:3, 3]))
