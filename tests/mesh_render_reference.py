"""The yardstick of the mesh renderer (the mesh-render block of include/scorp_gs.h), independent of both implementations in
scorp_amd/mesh/render.py and csrc/mesh_render.hip.

Rules 1 and 2 are applied as they stand, in float64 numpy: the snapped integers and the float64 1 / w DEFINE the input of
everything after them.  From there on nothing is rounded and nothing is shared with the implementations' formulation:
  * orientation is the usual cross product (b - a) x (p - a) in Python integers, never exchanged corners, no edge tables;
  * a pixel centre belongs to a triangle iff the centre moved by (eps, eps^2), eps = 2^-40 pixel units, lies STRICTLY inside
    (all three cross products have the sign of the area).  The coordinates are integers of at most 2^31 in size, so with
    everything scaled by 2^80 the moved point is an exact integer point and eps |d| < 1 can never change a non-zero sign:
    this is the meaning of the top-left rule, stated without naming an edge "top" or "left";
  * the depth is 1 / sum_k (c_k / S) inv_w_k in fractions.Fraction (inv_w_k is a float64, so a rational), the winner of a
    pixel the least (exact depth, face index), and only then is the depth rounded to fp32, correctly."""
from fractions import Fraction

import numpy as np

SNAP, SNAP_LIMIT = 256, 1 << 29
_N = 1 << 40          # 1 / eps
_N2 = _N * _N


def project(verts, m, H, W, near):
    """rules 1 and 2: (X, Y Python ints, inv_w float64, usable) per vertex"""
    v = np.asarray(verts, np.float32).astype(np.float64)
    m = np.asarray(m, np.float32).astype(np.float64).reshape(4, 4)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    with np.errstate(all="ignore"):
        p = [(z * m[2, j] + (y * m[1, j] + x * m[0, j])) + m[3, j] for j in (0, 1, 3)]
        w = p[2]
        inv_w = 1.0 / w
        sx = ((p[0] * inv_w + 1.0) * W - 1.0) * 0.5
        sy = ((p[1] * inv_w + 1.0) * H - 1.0) * 0.5
        fx, fy = np.floor(sx * 256.0 + 0.5), np.floor(sy * 256.0 + 0.5)
        ok = (w > near) & np.isfinite(w) & (np.abs(fx) <= SNAP_LIMIT) & (np.abs(fy) <= SNAP_LIMIT)
    X = [int(a) if o else 0 for a, o in zip(fx, ok)]
    Y = [int(a) if o else 0 for a, o in zip(fy, ok)]
    return X, Y, inv_w, ok


def _cross(ax, ay, bx, by, px, py):
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax)


def owners_of_view(verts, faces, m, H, W, near=0.01, cull=False):
    """{(j, i): [(exact depth Fraction, face), ...]}: every face that owns pixel centre (i, j), by brute force"""
    X, Y, inv_w, ok = project(verts, m, H, W, near)
    Nv = len(X)
    owners = {}
    for f, (a, b, c) in enumerate(np.asarray(faces).tolist()):
        if not all(0 <= k < Nv for k in (a, b, c)) or not (ok[a] and ok[b] and ok[c]):
            continue
        xs, ys = (X[a], X[b], X[c]), (Y[a], Y[b], Y[c])
        S = _cross(xs[0], ys[0], xs[1], ys[1], xs[2], ys[2])
        if S == 0 or (cull and S > 0):       # S < 0: counter-clockwise on the screen (y down), the front side
            continue
        sign = 1 if S > 0 else -1
        i0, i1 = max(-(-min(xs) // SNAP), 0), min(max(xs) // SNAP, W - 1)
        j0, j1 = max(-(-min(ys) // SNAP), 0), min(max(ys) // SNAP, H - 1)
        if i0 > i1 or j0 > j1:
            continue
        # candidates: the closed triangle, in numpy int64 (the products stay below 2^62)
        px = (SNAP * np.arange(i0, i1 + 1, dtype=np.int64))[None, :]
        py = (SNAP * np.arange(j0, j1 + 1, dtype=np.int64))[:, None]
        cs = [_cross(xs[(k + 1) % 3], ys[(k + 1) % 3], xs[(k + 2) % 3], ys[(k + 2) % 3], px, py) * sign for k in range(3)]
        closed = (cs[0] >= 0) & (cs[1] >= 0) & (cs[2] >= 0)
        iw = [Fraction(float(inv_w[k])) for k in (a, b, c)]
        for dj, di in zip(*np.nonzero(closed)):
            i, j = i0 + int(di), j0 + int(dj)
            c3 = [int(cs[k][dj, di]) * sign for k in range(3)]      # the cross products themselves; they sum to S
            if 0 in c3:                                             # on an edge: decide at the moved point, exactly
                qx, qy = SNAP * i * _N2 + _N, SNAP * j * _N2 + 1
                moved = [_cross(xs[(k + 1) % 3] * _N2, ys[(k + 1) % 3] * _N2, xs[(k + 2) % 3] * _N2, ys[(k + 2) % 3] * _N2, qx, qy)
                         for k in range(3)]
                if not all(mk * sign > 0 for mk in moved):
                    continue
            depth = 1 / sum(Fraction(c3[k], S) * iw[k] for k in range(3))
            owners.setdefault((j, i), []).append((depth, f))
    return owners


def round_f32(fr):
    """the fp32 nearest to a positive Fraction, ties to even"""
    c = np.float32(float(fr))
    best = None
    for cand in (np.nextafter(c, np.float32(0.0)), c, np.nextafter(c, np.float32(np.inf))):
        if not np.isfinite(cand):
            continue
        err = abs(Fraction(float(cand)) - fr)
        even = (int(np.float32(cand).view(np.uint32)) & 1) == 0
        if best is None or err < best[0] or (err == best[0] and even):
            best = (err, np.float32(cand))
    return best[1]


def resolve(owners, H, W, num_faces=None):
    """(face [H, W] int32, depth [H, W] float32 correctly rounded, faces that own a pixel) of the faces below num_faces"""
    face, depth, seen = np.full((H, W), -1, np.int32), np.zeros((H, W), np.float32), set()
    for (j, i), lst in owners.items():
        lst = [e for e in lst if num_faces is None or e[1] < num_faces]
        if not lst:
            continue
        d, f = min(lst)
        face[j, i], depth[j, i] = f, round_f32(d)
        seen.add(f)
    return face, depth, seen


def closest_depth_pair(owners):
    """the least relative gap between the exact depths of two different faces at one pixel (inf when no pixel has two)"""
    worst = float("inf")
    for lst in owners.values():
        ds = sorted(d for d, _ in lst)
        for a, b in zip(ds, ds[1:]):
            worst = min(worst, float((b - a) / b))
    return worst
