"""The yardstick of the cloud kernels (csrc/cloud_filter.hip): rules R1 - R6 of the cloud block of include/scorp_gs.h as a
float64 brute force in numpy - every pair's d^2, no grid, no pruning - and rules 1 - 3 of the vertex-clustering block for
voxel_down_sample.  Nothing here imports scorp_amd."""
import numpy as np


def d2_rows(P, lo, hi):
    """R1 for the rows lo..hi against every point: (dx dx + dy dy) + dz dz, each product and sum rounded on its own."""
    P = np.asarray(P, dtype=np.float32).astype(np.float64)
    d = P[lo:hi, None, :] - P[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _chunks(n, chunk=256):
    return [(lo, min(lo + chunk, n)) for lo in range(0, n, chunk)]


def radius_count(P, radius):
    """R2: |N_r(i)| [n] int32"""
    r2 = np.float64(radius) * np.float64(radius)
    return np.concatenate([(d2_rows(P, lo, hi) <= r2).sum(1) for lo, hi in _chunks(len(P))]).astype(np.int32)


def knn(P, k_asked):
    """R3: (mean distance [n] float64, neighbours [n, k_asked] int32 padded with -1)"""
    n = len(P)
    k = min(k_asked, n)
    mean = np.zeros(n)
    nb = np.full((n, k_asked), -1, np.int32)
    index = np.arange(n)
    for lo, hi in _chunks(n):
        D = d2_rows(P, lo, hi)
        for i in range(lo, hi):
            row = D[i - lo]
            order = np.lexsort((index, row))[:k]   # ascending (d2, j)
            s = 0.0
            for d2 in row[order]:                  # a sequential sum, not np.sum's pairwise one
                s = s + np.sqrt(d2)
            mean[i] = s / k
            nb[i, :k] = order
    return mean, nb


def dbscan(P, eps, min_points):
    """R4 - R6: (count [n] int32, core [n] bool, labels [n] int32, number of clusters)"""
    n = len(P)
    r2 = np.float64(eps) * np.float64(eps)
    count = radius_count(P, eps)
    core = count >= min_points
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    nearest_core = np.full(n, -1, np.int64)
    for lo, hi in _chunks(n):
        D = d2_rows(P, lo, hi)
        for i in range(lo, hi):
            cand = np.nonzero((D[i - lo] <= r2) & core)[0]
            if core[i]:
                for j in cand:
                    a, b = find(i), find(int(j))
                    if a != b:
                        parent[max(a, b)] = min(a, b)
            elif len(cand):
                nearest_core[i] = cand[np.lexsort((cand, D[i - lo, cand]))[0]]
    labels = np.full(n, -1, np.int32)
    number = {}
    for i in range(n):          # the sequential scan opens the clusters in order of their smallest core index
        if core[i]:
            labels[i] = number.setdefault(find(i), len(number))
    for i in range(n):
        if not core[i] and nearest_core[i] >= 0:
            labels[i] = labels[nearest_core[i]]
    return count, core, labels, len(number)


def statistical_keep(m, std_ratio):
    """(kept indices, threshold, smallest |m_i - threshold| / threshold) from knn means m"""
    n = len(m)
    mu = m.sum() / n
    sd = np.sqrt(((m - mu) ** 2).sum() / (n - 1)) if n > 1 else 0.0
    thr = mu + std_ratio * sd
    return np.nonzero(m <= thr)[0], thr, float(np.abs(m - thr).min() / thr)


def voxel_grid(P, h, colors=None):
    """Rules 1 - 3 of the vertex-clustering block: (cell of every point [n] int64, positions [C, 3] float32, colours [C, 3]
    float32 or None, member counts [C])"""
    P32 = np.asarray(P, dtype=np.float32)
    v = P32.astype(np.float64)
    origin = P32.min(0).astype(np.float64) - 0.5 * h
    ijk = np.floor((v - origin) / h).astype(np.int64)
    assert (ijk >= 0).all() and (ijk < 1 << 21).all()
    _, first, inverse = np.unique(ijk[:, 0] << 42 | ijk[:, 1] << 21 | ijk[:, 2], return_index=True, return_inverse=True)
    order = np.argsort(first)                    # the cells by their smallest point index
    number = np.empty_like(order)
    number[order] = np.arange(order.size)
    cell = number[inverse.reshape(-1)]
    C = order.size
    count = np.bincount(cell, minlength=C)
    total = lambda w: np.stack([np.bincount(cell, weights=w[:, k], minlength=C) for k in range(3)], 1)
    positions = (total(v) / count[:, None]).astype(np.float32)
    colours = None if colors is None else (total(np.asarray(colors, np.float32).astype(np.float64)) / count[:, None]).astype(np.float32)
    return cell, positions, colours, count
