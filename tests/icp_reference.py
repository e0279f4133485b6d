"""The yardstick of the ICP tests: Open3D's registration_icp with TransformationEstimationPointToPoint (no scaling) and the
alignment scripts' get_ICP_fitting_transformation_best (align_3dgs_clpe_9dof.py:42-115), restated in float64 numpy with
scipy.spatial.cKDTree for the radius-bounded nearest neighbour.  No GPU, no Open3D."""
import numpy as np
from scipy.spatial import cKDTree


def correspondence_pass(tree, target, source, T, r, workers=1):
    """(fitness, inlier_rmse, x of the pairs, q of the pairs, pair count) of the source under T."""
    x = source @ T[:3, :3].T + T[:3, 3]
    d, idx = tree.query(x, k=1, distance_upper_bound=r, workers=workers)
    ok = np.isfinite(d) & (idx < len(target))
    xs, qs = x[ok], target[idx[ok]]
    c = int(ok.sum())
    if c == 0:
        return 0.0, 0.0, xs, qs, 0
    d2 = ((xs - qs) ** 2).sum(axis=1)
    keep = d2 <= r * r      # cKDTree's bound is on the distance; the spec's pair test is d^2 <= r^2
    xs, qs, d2 = xs[keep], qs[keep], d2[keep]
    c = len(d2)
    if c == 0:
        return 0.0, 0.0, xs, qs, 0
    return c / len(source), float(np.sqrt(d2.sum() / c)), xs, qs, c


def kabsch_update(xs, qs):
    """Umeyama without scale: the rigid 4x4 U minimising sum |U x - q|^2 (the identity for no pairs)."""
    U4 = np.eye(4)
    if len(xs) == 0:
        return U4
    xm, qm = xs.mean(axis=0), qs.mean(axis=0)
    sigma = (qs - qm).T @ (xs - xm) / len(xs)
    U, _, Vt = np.linalg.svd(sigma)
    D = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        D[2, 2] = -1.0
    R = U @ D @ Vt
    U4[:3, :3] = R
    U4[:3, 3] = qm - R @ xm
    return U4


def registration_icp(source, target, r, init, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6, tree=None,
                     workers=1):
    """dict(transformation, fitness, inlier_rmse, iterations, passes=[pair counts of every pass])."""
    source = np.asarray(source, dtype=np.float64)
    target = np.asarray(target, dtype=np.float64)
    if r <= 0:
        raise ValueError("r must be positive")
    if len(source) == 0 or len(target) == 0:
        raise ValueError("empty cloud")
    if max_iteration < 0:
        raise ValueError("max_iteration < 0")
    tree = tree if tree is not None else cKDTree(target)
    T = np.asarray(init, dtype=np.float64).copy()
    fit, rmse, xs, qs, c = correspondence_pass(tree, target, source, T, r, workers)
    passes = [c]
    it = 0
    for i in range(max_iteration):
        T = kabsch_update(xs, qs) @ T
        pf, pr = fit, rmse
        fit, rmse, xs, qs, c = correspondence_pass(tree, target, source, T, r, workers)
        passes.append(c)
        it = i + 1
        if abs(pf - fit) < relative_fitness and abs(pr - rmse) < relative_rmse:
            break
    return {"transformation": T, "fitness": fit, "inlier_rmse": rmse, "iterations": it, "passes": passes}


def downsample_indices(num_original, num_refined):
    if num_refined > 4 * num_original:
        k = int(num_refined / (4 * num_original))
        return np.arange(0, num_refined, k)
    return np.arange(num_refined)


def icp_inits(rotations, center_original, center_refined):
    inits = []
    for rot in rotations:
        T = np.eye(4)
        T[:3, :3] = rot
        T[:3, 3] = center_original - rot @ center_refined
        inits.append(T)
    for _ in range(2):
        T = np.eye(4)
        T[:3, 3] = center_original - center_refined
        inits.append(T)
    inits.append(np.eye(4))
    return np.stack(inits)


def get_ICP_fitting_transformation_best(pc_xyz_original, pc_xyz_refined, rotations, threshold, max_iteration=400,
                                        workers=1, return_all=False):
    if np.any(np.isnan(pc_xyz_original)) or np.any(np.isnan(pc_xyz_refined)):
        raise ValueError("Point clouds contain NaN values")
    if np.any(np.isinf(pc_xyz_original)) or np.any(np.isinf(pc_xyz_refined)):
        raise ValueError("Point clouds contain Inf values")
    center_original = pc_xyz_original.mean(axis=0)
    center_refined = pc_xyz_refined.mean(axis=0)
    src = pc_xyz_refined[downsample_indices(len(pc_xyz_original), len(pc_xyz_refined))]
    tgt = np.asarray(pc_xyz_original, dtype=np.float64)
    tree = cKDTree(tgt)
    best_fitness, best_transform, results = -np.inf, None, []
    for T0 in icp_inits(rotations, center_original, center_refined):
        res = registration_icp(src, tgt, threshold, T0, max_iteration=max_iteration, tree=tree, workers=workers)
        results.append(res)
        if res["fitness"] > best_fitness:
            best_fitness, best_transform = res["fitness"], res["transformation"]
    return (best_transform, results) if return_all else best_transform


def box_surface(lo, hi, n, rng):
    """n points uniformly on the surface of the axis-aligned box [lo, hi]."""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    e = hi - lo
    areas = np.array([e[1] * e[2], e[1] * e[2], e[0] * e[2], e[0] * e[2], e[0] * e[1], e[0] * e[1]])
    face = rng.choice(6, size=n, p=areas / areas.sum())
    p = lo + rng.random((n, 3)) * e
    ax = face // 2
    p[np.arange(n), ax] = np.where(face % 2 == 0, lo[ax], hi[ax])
    return p


def asymmetric_object(n, seed):
    """Surface samples of three boxes of different sizes joined off-centre: no rotational symmetry."""
    rng = np.random.default_rng(seed)
    parts = [((-0.5, -0.3, -0.2), (0.5, 0.3, 0.2), 0.6), ((0.2, 0.3, -0.2), (0.5, 0.7, 0.1), 0.25),
             ((-0.5, -0.3, 0.2), (-0.2, 0.0, 0.6), 0.15)]
    pts = [box_surface(lo, hi, int(n * w), rng) for lo, hi, w in parts]
    p = np.concatenate(pts)
    return p[rng.permutation(len(p))]


def random_rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
