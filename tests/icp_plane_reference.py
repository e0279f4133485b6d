"""The yardstick of the point-to-plane ICP and normal-estimation tests: the rules of include/scorp_gs.h
(scorp_icp_point_to_plane, scorp_estimate_normals) restated in float64 numpy - np.linalg.eigh for both eigen problems,
scipy's cKDTree for the ICP pairing as tests/icp_reference.py does, all pairwise distances for the k nearest neighbours.
Written from the header text, not from the kernels.  No GPU, no Open3D."""
import numpy as np
from scipy.spatial import cKDTree

EIG_CUT = 1e-12          # eigenvalues of A at or below this share of the largest are left out of the step


def frame(target):
    """(c_t, s): the centre of the target's bounding box and half its largest edge (1 if that is 0)."""
    t = np.asarray(target, np.float64)
    lo, hi = t.min(axis=0), t.max(axis=0)
    e = float((hi - lo).max())
    return 0.5 * (lo + hi), (0.5 * e if e > 0.0 else 1.0)


def system(xs, qs, ns, ct, s):
    """A = sum J J^T and b = sum J rho of the pairs, J = [(x cross n) / s ; n], rho = n . (x - q), relative to c_t."""
    x, q = xs - ct, qs - ct
    J = np.hstack([np.cross(x, ns) / s, ns])
    rho = (ns * (x - q)).sum(axis=1)
    return J.T @ J, J.T @ rho


def min_norm_step(A, b):
    """(xi, eigenvalues): xi = - sum over { l_i > 1e-12 l_max } of v_i (v_i . b) / l_i; zero when l_max = 0."""
    lam, V = np.linalg.eigh(A)
    lmax = lam.max()
    if not lmax > 0.0:
        return np.zeros(6), lam
    keep = lam > EIG_CUT * lmax
    return -(V[:, keep] * ((V[:, keep].T @ b) / lam[keep])).sum(axis=1), lam


def rotation_zyx(w):
    """Rz(w_z) Ry(w_y) Rx(w_x)."""
    cx, sx, cy, sy, cz, sz = np.cos(w[0]), np.sin(w[0]), np.cos(w[1]), np.sin(w[1]), np.cos(w[2]), np.sin(w[2])
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def reference_update(xs, qs, ns, ct, s, return_eig=False):
    """The 4x4 update of one pass's pairs (absolute coordinates): x' -> R x' + tau about c_t; the identity for no pairs."""
    U = np.eye(4)
    lam = np.zeros(6)
    if len(xs):
        A, b = system(np.asarray(xs, np.float64), np.asarray(qs, np.float64), np.asarray(ns, np.float64), ct, s)
        xi, lam = min_norm_step(A, b)
        R = rotation_zyx(xi[:3] / s)
        U[:3, :3] = R
        U[:3, 3] = xi[3:] + ct - R @ ct
    return (U, lam) if return_eig else U


def correspondence_pass(tree, target, source, T, r):
    """(fitness, inlier_rmse, x of the pairs, target index of the pairs) of the source under T: the nearest target point
    with d^2 <= r^2."""
    x = source @ T[:3, :3].T + T[:3, 3]
    d, idx = tree.query(x, k=1, distance_upper_bound=r * (1.0 + 1e-9))
    ok = np.isfinite(d) & (idx < len(target))
    ok[ok] = ((x[ok] - target[idx[ok]]) ** 2).sum(axis=1) <= r * r
    c = int(ok.sum())
    if c == 0:
        return 0.0, 0.0, x[ok], idx[ok]
    d2 = ((x[ok] - target[idx[ok]]) ** 2).sum(axis=1)
    return c / len(source), float(np.sqrt(d2.sum() / c)), x[ok], idx[ok]


def registration_icp(source, target, normals, r, init, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """dict(transformation, fitness, inlier_rmse, iterations, passes = pair count of every pass, poses = T at every pass,
    eigenvalues = those of every update's A)."""
    source, target, normals = (np.asarray(a, np.float64) for a in (source, target, normals))
    ct, s = frame(target)
    tree = cKDTree(target)
    T = np.asarray(init, np.float64).copy()
    fit, rmse, xs, idx = correspondence_pass(tree, target, source, T, r)
    passes, poses, eig, it = [len(idx)], [T.copy()], [], 0
    for i in range(max_iteration):
        U, lam = reference_update(xs, target[idx], normals[idx], ct, s, return_eig=True)
        eig.append(lam)
        T = U @ T
        pf, pr = fit, rmse
        fit, rmse, xs, idx = correspondence_pass(tree, target, source, T, r)
        passes.append(len(idx))
        poses.append(T.copy())
        it = i + 1
        if abs(pf - fit) < relative_fitness and abs(pr - rmse) < relative_rmse:
            break
    return {"transformation": T, "fitness": fit, "inlier_rmse": rmse, "iterations": it, "passes": passes, "poses": poses,
            "eigenvalues": eig}


def eig_ratios_clear(eigenvalues):
    """No eigenvalue ratio l_i / l_max of any A within [1e-14, 1e-10]: the 1e-12 cut decides the same way in any float64."""
    for lam in eigenvalues:
        lmax = lam.max()
        if lmax > 0.0 and np.any((lam / lmax >= 1e-14) & (lam / lmax <= 1e-10)):
            return False
    return True


# ---- normals ----

def knn_brute(points, knn, rows=None, chunk=512):
    """Per point of `rows` (all by default): (idx [m, k] its k = min(knn, n) nearest points sorted by (d^2, index), itself
    included; dk the distance of the k-th; dk1 that of the (k + 1)-th, inf if there is none).  All pairwise d^2 in
    float64 on the given values."""
    p = np.asarray(points, np.float64)
    n = len(p)
    k = min(knn, n)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    idx = np.empty((len(rows), k), np.int64)
    dk, dk1 = np.empty(len(rows)), np.full(len(rows), np.inf)
    for b in range(0, len(rows), chunk):
        x = p[rows[b:b + chunk]]
        dd = np.zeros((len(x), n))
        for a in range(3):
            u = x[:, a, None] - p[None, :, a]
            u *= u
            dd += u
        order = np.argsort(dd, axis=1, kind="stable")[:, :k + 1]     # stable: equal d^2 in index order
        sd = np.take_along_axis(dd, order, axis=1)
        idx[b:b + chunk] = order[:, :k]
        dk[b:b + chunk] = np.sqrt(sd[:, k - 1])
        if k < n:
            dk1[b:b + chunk] = np.sqrt(sd[:, k])
    return idx, dk, dk1


def normals_of(points, idx):
    """(normals [m, 3], eigenvalues [m, 3] ascending) from the neighbour lists: covariance about the mean, the eigenvector
    of the smallest eigenvalue, unit length, the component of largest magnitude (the first of equal ones) positive;
    fewer than 3 points: (0, 0, 1)."""
    p = np.asarray(points, np.float64)
    m = len(idx)
    if len(p) < 3:
        return np.tile([0.0, 0.0, 1.0], (m, 1)), np.zeros((m, 3))
    nb = p[idx]                                                       # [m, k, 3]
    e = nb - nb.mean(axis=1, keepdims=True)
    C = np.einsum("mka,mkb->mab", e, e) / idx.shape[1]
    lam, V = np.linalg.eigh(C)
    v = V[:, :, 0]
    v = v / np.linalg.norm(v, axis=1, keepdims=True)
    big = np.take_along_axis(v, np.abs(v).argmax(axis=1)[:, None], axis=1)
    return v * np.where(big < 0.0, -1.0, 1.0), lam


def estimate_normals(points, knn=30):
    idx, _, _ = knn_brute(points, knn)
    return normals_of(points, idx)[0]
