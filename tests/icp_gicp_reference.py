"""The yardstick of the generalized ICP tests: the rules of include/scorp_gs.h (scorp_icp_generalized) restated in float64
numpy - the cKDTree pair search of tests/icp_reference.py (as icp_plane_reference.correspondence_pass restates it, kept
with the indices of both sides of a pair), the cofactor inverse as the header writes it, np.linalg.eigh for the 6x6 and the
minimum-norm step of tests/icp_plane_reference.py.  Written from the header text, not from the kernels.  No GPU, no
Open3D."""
import numpy as np
from scipy.spatial import cKDTree

from tests import icp_plane_reference as pref

frame = pref.frame
TRIU = ([0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2])          # (row, column) of xx, xy, xz, yy, yz, zz


def unpack(c6):
    """[n, 6] -> symmetric [n, 3, 3] float64."""
    c6 = np.asarray(c6, np.float64)
    C = np.empty((len(c6), 3, 3))
    C[:, TRIU[0], TRIU[1]] = c6
    C[:, TRIU[1], TRIU[0]] = c6
    return C


def pack(C):
    """[n, 3, 3] -> its upper triangle [n, 6]."""
    return np.asarray(C)[:, TRIU[0], TRIU[1]]


def rotate(C, A):
    """A C A^T per covariance, symmetric by construction (built from the six values of C)."""
    M = np.einsum("ab,nbc,dc->nad", A, C, A)
    return unpack(pack(M))


def skew(x):
    S = np.zeros((len(x), 3, 3))
    S[:, 0, 1], S[:, 0, 2], S[:, 1, 0] = -x[:, 2], x[:, 1], x[:, 2]
    S[:, 1, 2], S[:, 2, 0], S[:, 2, 1] = -x[:, 0], -x[:, 1], x[:, 0]
    return S


def positive_definite(M):
    """Sylvester's test on finite symmetric [n, 3, 3]: M00 > 0, M00 M11 - M01^2 > 0, det M > 0 (by cofactors)."""
    K, det = cofactors(M)
    with np.errstate(invalid="ignore"):
        return np.isfinite(M).all(axis=(1, 2)) & (M[:, 0, 0] > 0.0) & (K[:, 2, 2] > 0.0) & (det > 0.0)


def cofactors(M):
    """(the symmetric cofactor matrix K, det M = M00 K00 + M01 K01 + M02 K02)."""
    m00, m01, m02, m11, m12, m22 = (M[:, a, b] for a, b in zip(*TRIU))
    with np.errstate(invalid="ignore", over="ignore"):
        k = np.stack([m11 * m22 - m12 * m12, m02 * m12 - m01 * m22, m01 * m12 - m02 * m11,
                      m00 * m22 - m02 * m02, m01 * m02 - m00 * m12, m00 * m11 - m01 * m01], axis=1)
        det = m00 * k[:, 0] + m01 * k[:, 1] + m02 * k[:, 2]
    return unpack(k), det


def weights(M, inverse="cofactor"):
    """(valid mask, W = M^-1 of the valid pairs)."""
    ok = positive_definite(M)
    Mv = M[ok]
    if inverse == "numpy":
        return ok, (np.linalg.inv(Mv) if len(Mv) else Mv)
    if inverse != "cofactor":
        raise ValueError(inverse)
    K, det = cofactors(Mv)
    return ok, K / det[:, None, None]


def system(xs, qs, Cs_rotated, Cq, ct, s, inverse="cofactor", W=None):
    """A = sum J^T W J and b = sum J^T W u over the pairs whose M = C_q + A_T C_p A_T^T is positive definite (all of them
    when W is injected), J = [ -[x]x / s | I ], u = x - q, relative to c_t."""
    x, q = np.asarray(xs, np.float64) - ct, np.asarray(qs, np.float64) - ct
    if W is None:
        ok, W = weights(np.asarray(Cq, np.float64) + np.asarray(Cs_rotated, np.float64), inverse)
        x, q = x[ok], q[ok]
    J = np.concatenate([-skew(x) / s, np.tile(np.eye(3), (len(x), 1, 1))], axis=2)      # [c, 3, 6]
    WJ = np.einsum("nab,nbc->nac", W, J)
    A = np.einsum("nab,nac->bc", J, WJ)
    b = np.einsum("nab,na->b", WJ, x - q)
    return A, b


def reference_update(xs, qs, Cs_rotated, Cq, ct, s, inverse="cofactor", W=None, return_eig=False):
    """The 4x4 update of one pass's pairs (absolute coordinates): x' -> R x' + tau about c_t; the identity for no pairs
    or when nothing constrains the step."""
    U = np.eye(4)
    lam = np.zeros(6)
    if len(xs):
        A, b = system(xs, qs, Cs_rotated, Cq, ct, s, inverse, W)
        xi, lam = pref.min_norm_step(A, b)
        R = pref.rotation_zyx(xi[:3] / s)
        U[:3, :3] = R
        U[:3, 3] = xi[3:] + ct - R @ ct
    return (U, lam) if return_eig else U


def registration_icp(source, target, source_covariances, target_covariances, r, init, max_iteration=30, relative_fitness=1e-6,
                     relative_rmse=1e-6, inverse="cofactor", rotate_source=True):
    """dict(transformation, fitness, inlier_rmse, iterations, passes = pair count of every pass, poses = T at every pass,
    eigenvalues = those of every update's A).  The covariances are [n, 6]; rotate_source=False leaves C_p unrotated (the
    omission tests/test_icp_gicp_cpu.py makes visible)."""
    source, target = np.asarray(source, np.float64), np.asarray(target, np.float64)
    Cp, Cq = unpack(source_covariances), unpack(target_covariances)
    ct, s = frame(target)
    tree = cKDTree(target)
    T = np.asarray(init, np.float64).copy()

    def one_pass(T):
        x = source @ T[:3, :3].T + T[:3, 3]
        d, idx = tree.query(x, k=1, distance_upper_bound=r * (1.0 + 1e-9))
        ok = np.isfinite(d) & (idx < len(target))
        ok[ok] = ((x[ok] - target[idx[ok]]) ** 2).sum(axis=1) <= r * r
        c = int(ok.sum())
        if c == 0:
            return 0.0, 0.0, x[ok], idx[ok], np.flatnonzero(ok)
        d2 = ((x[ok] - target[idx[ok]]) ** 2).sum(axis=1)
        return c / len(source), float(np.sqrt(d2.sum() / c)), x[ok], idx[ok], np.flatnonzero(ok)

    fit, rmse, xs, idx, sel = one_pass(T)
    passes, poses, eig, it = [len(idx)], [T.copy()], [], 0
    for i in range(max_iteration):
        Cs = rotate(Cp[sel], T[:3, :3]) if rotate_source else Cp[sel]
        U, lam = reference_update(xs, target[idx], Cs, Cq[idx], ct, s, inverse, return_eig=True)
        eig.append(lam)
        T = U @ T
        pf, pr = fit, rmse
        fit, rmse, xs, idx, sel = one_pass(T)
        passes.append(len(idx))
        poses.append(T.copy())
        it = i + 1
        if abs(pf - fit) < relative_fitness and abs(pr - rmse) < relative_rmse:
            break
    return {"transformation": T, "fitness": fit, "inlier_rmse": rmse, "iterations": it, "passes": passes, "poses": poses,
            "eigenvalues": eig}
