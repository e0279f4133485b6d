"""The yardstick of the coloured ICP and colour-gradient tests: the rules of include/scorp_gs.h (scorp_icp_colored,
scorp_color_gradients) restated in float64 numpy - np.linalg.eigh for both eigen problems, the pair search, the
minimum-norm step, Rz Ry Rx and the frame of tests/icp_plane_reference.py.  Written from the header text, not from the
kernels.  No GPU, no Open3D."""
import numpy as np
from scipy.spatial import cKDTree

from tests import icp_plane_reference as pref

frame = pref.frame
EIG_CUT = pref.EIG_CUT      # the same share of the largest eigenvalue cuts the gradient rule's M


# ---- the gradient rule ----

def gradient_system(points, normals, intensity, row, i):
    """(M, g, neighbours used) of point i over its neighbour row: entries j >= 0, j != i, in row order."""
    p, I = np.asarray(points, np.float64), np.asarray(intensity, np.float64)
    n = np.asarray(normals, np.float64)[i]
    with np.errstate(over="ignore", invalid="ignore"):
        ln = np.sqrt((n * n).sum())
    nh = n / ln if np.isfinite(ln) and ln > 0.0 else np.zeros(3)
    js = np.array([j for j in np.asarray(row) if 0 <= j < len(p) and j != i], np.int64)
    if not len(js):
        return np.zeros((3, 3)), np.zeros(3), 0
    u = p[js] - p[i]
    e = u - (u @ nh)[:, None] * nh
    delta = I[js] - I[i]
    M = e.T @ e + (e * e).sum() * np.outer(nh, nh)
    return M, e.T @ delta, len(js)


def gradient_of(M, g, used):
    """(d, eigenvalues of M): d = sum over { l_k > 1e-12 l_max } of v_k (v_k . g) / l_k; zero when fewer than two
    neighbours were used or l_max = 0."""
    lam, V = np.linalg.eigh(M)
    lmax = lam.max()
    if used < 2 or not lmax > 0.0:
        return np.zeros(3), lam
    keep = lam > EIG_CUT * lmax
    return (V[:, keep] * ((V[:, keep].T @ g) / lam[keep])).sum(axis=1), lam


def color_gradients(points, normals, intensity, neighbors, rows=None, return_eig=False):
    """Gradients [m, 3] float64 of the points `rows` (all by default); neighbors[k] is the row of rows[k]."""
    rows = np.arange(len(neighbors)) if rows is None else np.asarray(rows)
    out, eig = np.zeros((len(rows), 3)), np.zeros((len(rows), 3))
    for k, i in enumerate(rows):
        out[k], eig[k] = gradient_of(*gradient_system(points, normals, intensity, neighbors[k], int(i)))
    return (out, eig) if return_eig else out


def estimate_color_gradients(points, intensity, normals=None, knn=30):
    """(gradients, normals) by the yardstick's own neighbour lists (icp_plane_reference.knn_brute, padded with -1)."""
    idx, _, _ = pref.knn_brute(points, knn)
    if normals is None:
        normals = pref.normals_of(points, idx)[0]
    nb = np.full((len(idx), knn), -1, np.int64)
    nb[:, :idx.shape[1]] = idx
    return color_gradients(points, normals, intensity, nb), normals


# ---- the estimator ----

def system(xs, qs, ns, ds, Iq, Ip, lam, ct, s):
    """A = sum lambda J_G J_G^T + (1 - lambda) J_C J_C^T and b = sum lambda J_G rho_G + (1 - lambda) J_C rho_C of the
    pairs, J_G = [(x cross n) / s ; n], rho_G = n . (x - q), J_C = [(x cross d) / s ; d], rho_C = d . (x - q) + (I_q - I_p),
    relative to c_t."""
    x, q = np.asarray(xs, np.float64) - ct, np.asarray(qs, np.float64) - ct
    JG = np.hstack([np.cross(x, ns) / s, ns])
    JC = np.hstack([np.cross(x, ds) / s, ds])
    rG = (ns * (x - q)).sum(axis=1)
    rC = (ds * (x - q)).sum(axis=1) + (Iq - Ip)
    return lam * (JG.T @ JG) + (1.0 - lam) * (JC.T @ JC), lam * (JG.T @ rG) + (1.0 - lam) * (JC.T @ rC)


def reference_update(xs, qs, ns, ds, Iq, Ip, lam, ct, s, return_eig=False):
    """The 4x4 update of one pass's pairs (absolute coordinates): x' -> R x' + tau about c_t; the identity for no pairs
    or when nothing constrains the step."""
    U = np.eye(4)
    eig = np.zeros(6)
    if len(xs):
        A, b = system(xs, qs, *(np.asarray(a, np.float64) for a in (ns, ds, Iq, Ip)), lam, ct, s)
        xi, eig = pref.min_norm_step(A, b)
        R = pref.rotation_zyx(xi[:3] / s)
        U[:3, :3] = R
        U[:3, 3] = xi[3:] + ct - R @ ct
    return (U, eig) if return_eig else U


def _rows(a):
    a = np.ascontiguousarray(a, np.float64)
    return a.view([("", np.float64)] * 3).ravel()


def pairs_of(tree, target, source, T, r):
    """icp_plane_reference.correspondence_pass with the source index of every pair: (fitness, inlier_rmse, x, target
    index, source index)."""
    fit, rmse, xs, idx = pref.correspondence_pass(tree, target, source, T, r)
    x = source @ T[:3, :3].T + T[:3, 3]              # the pass's own expression: the same bits
    sel = np.flatnonzero(np.isin(_rows(x), _rows(xs)))
    assert len(sel) == len(xs) and np.array_equal(x[sel], xs)
    return fit, rmse, xs, idx, sel


def registration_icp(source, source_intensity, target, normals, target_intensity, gradients, r, init, lambda_geometric=0.968,
                     max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6):
    """dict(transformation, fitness, inlier_rmse, iterations, passes = pair count of every pass, poses = T at every pass,
    eigenvalues = those of every update's A)."""
    source, target, normals, gradients, Ip, Iq = (np.asarray(a, np.float64) for a in
                                                  (source, target, normals, gradients, source_intensity, target_intensity))
    ct, s = frame(target)
    tree = cKDTree(target)
    T = np.asarray(init, np.float64).copy()
    fit, rmse, xs, idx, sel = pairs_of(tree, target, source, T, r)
    passes, poses, eig, it = [len(idx)], [T.copy()], [], 0
    for i in range(max_iteration):
        U, lam = reference_update(xs, target[idx], normals[idx], gradients[idx], Iq[idx], Ip[sel], lambda_geometric, ct, s,
                                  return_eig=True)
        eig.append(lam)
        T = U @ T
        pf, pr = fit, rmse
        fit, rmse, xs, idx, sel = pairs_of(tree, target, source, T, r)
        passes.append(len(idx))
        poses.append(T.copy())
        it = i + 1
        if abs(pf - fit) < relative_fitness and abs(pr - rmse) < relative_rmse:
            break
    return {"transformation": T, "fitness": fit, "inlier_rmse": rmse, "iterations": it, "passes": passes, "poses": poses,
            "eigenvalues": eig}
