"""The rules O1 - O6 of include/scorp_gs.h (consistent orientation of normals along the minimum spanning forest of the
neighbour graph) restated in float64 numpy: Kruskal over the edges sorted in O3's order, a stack walk from the smallest
index of every component for O4, the votes of O5.  The yardstick of tests/test_orient_cpu.py and tests/test_orient_gpu.py;
nothing here is shared with the kernels."""
import numpy as np

CENTER_LANES, CENTER_RUN = 16384, 64


def edges(neighbors, n):
    """O1: the distinct edges [e, 2] as (lo, hi), lo < hi, sorted by (lo, hi).  Entries < 0 are padding, an entry equal to
    its row is ignored, an entry >= n raises."""
    nb = np.asarray(neighbors, dtype=np.int64)
    assert nb.ndim == 2 and nb.shape[0] == n and 1 <= nb.shape[1] <= 64
    if nb.max(initial=-1) >= n:
        raise ValueError("neighbour index >= n")
    rows = np.repeat(np.arange(n, dtype=np.int64), nb.shape[1])
    cols = nb.reshape(-1)
    keep = (cols >= 0) & (cols != rows)
    rows, cols = rows[keep], cols[keep]
    e = np.stack([np.minimum(rows, cols), np.maximum(rows, cols)], axis=1)
    return np.unique(e, axis=0).reshape(-1, 2) if len(e) else e.reshape(0, 2)


def dot(N, i, j):
    """O2's dot on the float32 normals as given: (x x + y y) + z z, every operation rounded to float64 on its own"""
    a, b = np.asarray(N, np.float32).astype(np.float64)[i], np.asarray(N, np.float32).astype(np.float64)[j]
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def sorted_edges(N, neighbors):
    """(edges in O3's order, their dots, their weights)"""
    n = len(N)
    e = edges(neighbors, n)
    d = dot(N, e[:, 0], e[:, 1])
    w = 1.0 - np.abs(d)
    order = np.lexsort((e[:, 1], e[:, 0], w))
    return e[order], d[order], w[order]


def mean_center(P):
    """O5's default centre: the fixed order of additions of the rule (numpy's cumsum adds one element after the other)."""
    P = np.asarray(P, np.float32).astype(np.float64)
    n = len(P)
    rows = -(-n // CENTER_LANES)
    padded = np.zeros((rows * CENTER_LANES, 3))
    padded[:n] = P                                                           # (x + 0.0 = x: the padding changes no sum)
    S = np.cumsum(padded.reshape(rows, CENTER_LANES, 3), axis=0)[-1]         # S_g
    T = np.cumsum(S.reshape(CENTER_LANES // CENTER_RUN, CENTER_RUN, 3), axis=1)[:, -1]
    return np.cumsum(T, axis=0)[-1] / float(n)


def away_dots(P, N, center):
    """dd of O5 for the normals as given"""
    d = np.asarray(P, np.float32).astype(np.float64) - np.asarray(center, np.float64)
    n = np.asarray(N, np.float32).astype(np.float64)
    return (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]


def away_from(P, N, center=None):
    """orient_normals_away_from: flip where dd < 0 about the centre (default: the plain float64 mean)"""
    c = np.asarray(P, np.float32).astype(np.float64).sum(0) / len(P) if center is None else center
    N = np.asarray(N, np.float32)
    return np.where((away_dots(P, N, c) < 0)[:, None], -N, N)


def forest(N, neighbors):
    """Kruskal in O3's order: (tree edges [t, 2] in the order taken, their dots, every edge sorted, every weight sorted)"""
    n = len(N)
    e, d, w = sorted_edges(N, neighbors)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    take = []
    for idx, (a, b) in enumerate(e.tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
            take.append(idx)
    take = np.asarray(take, dtype=np.int64)
    return e[take], d[take], e, w


def orient(P, N, neighbors, center=None, component_sign="majority_away"):
    """O1 - O6.  dict: normals [n, 3] float32, flip [n] bool, rel [n] bool (O4 alone), label [n] int32, tree [t, 2] int64
    sorted by (lo, hi), n_components, votes {label: votes} (majority_away), center."""
    assert component_sign in ("majority_away", "first")
    N = np.ascontiguousarray(N, dtype=np.float32)
    n = len(N)
    tree, tdot, _, _ = forest(N, neighbors)
    adj = [[] for _ in range(n)]
    for (a, b), d in zip(tree.tolist(), tdot.tolist()):
        adj[a].append((b, d < 0.0))
        adj[b].append((a, d < 0.0))
    label = np.full(n, -1, dtype=np.int32)
    rel = np.zeros(n, dtype=bool)
    for m in range(n):                         # ascending: the first unvisited vertex is its component's smallest
        if label[m] >= 0:
            continue
        label[m] = m
        stack = [m]
        while stack:
            x = stack.pop()
            for y, opposite in adj[x]:
                if label[y] < 0:
                    label[y] = m
                    rel[y] = rel[x] ^ opposite
                    stack.append(y)
    flip = rel.copy()
    votes, c = {}, None
    if component_sign == "majority_away":
        c = mean_center(P) if center is None else np.asarray(center, np.float64)
        dd = away_dots(P, N, c)
        dd = np.where(rel, -dd, dd)
        sign = (dd > 0).astype(np.int64) - (dd < 0).astype(np.int64)
        for m in np.unique(label).tolist():
            member = label == m
            votes[m] = int(sign[member].sum())
            if votes[m] < 0:
                flip[member] = ~flip[member]
    bits = N.view(np.uint32) ^ np.where(flip, np.uint32(0x80000000), np.uint32(0))[:, None]
    tree = tree[np.lexsort((tree[:, 1], tree[:, 0]))] if len(tree) else tree.reshape(0, 2)
    return {"normals": bits.view(np.float32), "flip": flip, "rel": rel, "label": label, "tree": tree.astype(np.int64),
            "n_components": int(len(np.unique(label))), "votes": votes, "center": c}


def knn(P, k):
    """The min(k, n) nearest points of every point, itself included, in ascending (d2, index), padded with -1: [n, k] int32
    (rule R3 of the cloud block)."""
    P = np.asarray(P, np.float32).astype(np.float64)
    n = len(P)
    out = np.full((n, k), -1, dtype=np.int32)
    for lo in range(0, n, 512):
        d = P[lo:lo + 512, None, :] - P[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        order = np.argsort(d2, axis=1, kind="stable")[:, :k]
        out[lo:lo + 512, :order.shape[1]] = order
    return out


def pca_normals(P, k):
    """Normals in the manner of estimate_normals, in numpy: the eigenvector of the smallest eigenvalue of the covariance of
    the k nearest points (itself included), signed so that its largest component is positive.  (normals float32, the list)"""
    nb = knn(P, k)
    P64 = np.asarray(P, np.float32).astype(np.float64)
    Q = P64[nb]                                         # (k <= n in every use)
    Q = Q - Q.mean(1, keepdims=True)
    cov = np.einsum("nki,nkj->nij", Q, Q)
    _, vec = np.linalg.eigh(cov)
    nrm = vec[:, :, 0]
    big = np.abs(nrm).argmax(1)
    nrm = nrm * np.sign(nrm[np.arange(len(nrm)), big])[:, None]
    return nrm.astype(np.float32), nb
