"""The yardstick of scorp_amd/mesh/distance.py: plain numpy float64, brute force over all (query, triangle) pairs, and in
ANOTHER formulation than the kernel's, so that a shared mistake cannot pass.  The kernel classifies the seven regions of a
triangle from six dot products relative to the grid centre; here the point is projected on the triangle's plane and taken
if it falls inside (three signed edge tests against the normal), else the nearest of the three clamped segment projections
is taken, all on the raw float64 values of the float32 inputs (no centre).  A triangle whose normal is exactly zero is its
three segments.  The sampler is restated from the same prefix array with Python integers for the hash."""
import numpy as np

_M64 = (1 << 64) - 1


def _dot(u, w):
    return (u * w).sum(-1)


def _segment(p, a, b):
    """(closest point, d^2) of the segments a..b to p, broadcast"""
    e = b - a
    den = _dot(e, e)
    with np.errstate(all="ignore"):
        t = np.where(den > 0.0, np.clip(_dot(p - a, e) / np.where(den > 0.0, den, 1.0), 0.0, 1.0), 0.0)
    c = a + t[..., None] * e
    return c, _dot(p - c, p - c)


def pair_closest(p, a, b, c):
    """(closest point [..., 3], d^2 [...]) of the triangles (a, b, c) to the points p; every argument broadcasts to [..., 3]"""
    p, a, b, c = np.broadcast_arrays(*(np.asarray(x, np.float64) for x in (p, a, b, c)))
    n = np.cross(b - a, c - a)
    nn = _dot(n, n)
    best_c, best_d = _segment(p, a, b)
    for s, e in ((b, c), (c, a)):
        cc, dd = _segment(p, s, e)
        take = dd < best_d
        best_c, best_d = np.where(take[..., None], cc, best_c), np.where(take, dd, best_d)
    with np.errstate(all="ignore"):
        safe = np.where(nn > 0.0, nn, 1.0)
        off = _dot(n, p - a)
        foot = p - (off / safe)[..., None] * n
        inside = (nn > 0.0) & (_dot(np.cross(b - a, p - a), n) >= 0.0) & (_dot(np.cross(c - b, p - b), n) >= 0.0) & \
            (_dot(np.cross(a - c, p - c), n) >= 0.0)
        plane_d = off * off / safe
    return np.where(inside[..., None], foot, best_c), np.where(inside, plane_d, best_d)


def brute_force(points, verts, faces, chunk_pairs=1 << 20):
    """(best d^2 [Q], its face [Q] (the lowest index of the minimum), the least d^2 over the OTHER faces [Q], +inf if there
    is none).  Non-finite queries give +inf, -1, +inf."""
    p64, v64 = np.asarray(points, np.float64), np.asarray(verts, np.float64)
    Q, F = len(p64), len(faces)
    best, face, second = np.full(Q, np.inf), np.full(Q, -1, np.int64), np.full(Q, np.inf)
    if Q == 0 or F == 0:
        return best, face, second
    a, b, c = (v64[faces[:, k]] for k in range(3))
    step = max(1, chunk_pairs // F)
    for s in range(0, Q, step):
        p = p64[s:s + step]
        ok = np.isfinite(p).all(1)
        _, d2 = pair_closest(np.where(ok[:, None], p, 0.0)[:, None, :], a[None], b[None], c[None])
        f = np.argmin(d2, 1)
        rows = np.arange(len(p))
        b1 = d2[rows, f].copy()
        d2[rows, f] = np.inf
        best[s:s + step] = np.where(ok, b1, np.inf)
        face[s:s + step] = np.where(ok, f, -1)
        second[s:s + step] = np.where(ok, d2.min(1), np.inf)
    return best, face, second


def on_faces(points, verts, faces, index):
    """(closest point [Q, 3], d^2 [Q]) of query i to the ONE face index[i]"""
    v64 = np.asarray(verts, np.float64)
    t = np.asarray(faces)[np.asarray(index, np.int64)]
    return pair_closest(np.asarray(points, np.float64), v64[t[:, 0]], v64[t[:, 1]], v64[t[:, 2]])


def _splitmix(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def variate(seed, i, k):
    return float(_splitmix(_splitmix(_splitmix(seed & _M64) ^ i) ^ k) >> 11) * 2.0 ** -53


def sample(verts, faces, prefix, n, seed):
    """(points float64 [n, 3] before the rounding to float32, faces [n], barycentric float64 [n, 3]) from the prefix array"""
    v64 = np.asarray(verts, np.float64)
    total = float(prefix[-1])
    pts, chosen, bary = np.empty((n, 3)), np.empty(n, np.int64), np.empty((n, 3))
    f = 0                             # (t rises with i, so the walk below never has to go back)
    for i in range(n):
        t = (i + variate(seed, i, 0)) / n * total
        if not t < total:
            t = np.nextafter(total, 0.0)
        while not prefix[f] > t:      # the first face whose inclusive prefix exceeds t (a linear walk where the kernel bisects)
            f += 1
        s, r = np.sqrt(variate(seed, i, 1)), variate(seed, i, 2)
        w = np.array([1.0 - s, s * (1.0 - r), s * r])
        A, B, C = (v64[faces[f, k]] for k in range(3))
        pts[i], chosen[i], bary[i] = w[0] * A + w[1] * B + w[2] * C, f, w
    return pts, chosen, bary
