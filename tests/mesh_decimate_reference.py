"""Yardstick of the edge-collapse decimator (csrc/mesh_decimate.hip, scorp_amd.mesh.simplify_quadric_decimation): rules
0 - 11 of include/scorp_gs.h in plain Python float64 - dictionaries from edge to faces and from vertex to neighbour set,
lists in ascending index order, sorted() for every ordering.  It does not import scorp_amd.mesh.

Every float of the result is a pure function of the input (nothing is summed in an order that could vary), so the tests
compare bit for bit: exact() below, no ulp.

The meshes of the tests are generated here, each the smallest at which one mechanism can fail."""
import functools
import math

import numpy as np

from tests import mesh_simplify_reference as sref

INF = float("inf")
NO_RANK = 2 ** 31 - 1
DET_FLOOR = 1e-9      # rule 4: the solve is taken iff det > DET_FLOOR ((t t) t), t the trace of A
REACH = 4.0           # ... and |x - mid|^2 <= REACH |P[hi] - P[lo]|^2
M64 = (1 << 64) - 1


def mix(x):
    """the splitmix64 finaliser"""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def _sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _cross(u, w):
    return [u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]]


def _dot(u, w):
    return (u[0] * w[0] + u[1] * w[1]) + u[2] * w[2]


def _add_plane(q, n, d, w):
    """q += w (n n^T, d n, d^2): A as xx xy xz yy yz zz, then b, then c"""
    wn = [w * n[0], w * n[1], w * n[2]]
    q[0] += wn[0] * n[0]
    q[1] += wn[0] * n[1]
    q[2] += wn[0] * n[2]
    q[3] += wn[1] * n[1]
    q[4] += wn[1] * n[2]
    q[5] += wn[2] * n[2]
    wd = w * d
    q[6] += wd * n[0]
    q[7] += wd * n[1]
    q[8] += wd * n[2]
    q[9] += wd * d


def cost_of(q, x):
    s2 = (q[0] * (x[0] * x[0]) + q[3] * (x[1] * x[1])) + q[5] * (x[2] * x[2])
    s1 = (q[1] * (x[0] * x[1]) + q[2] * (x[0] * x[2])) + q[4] * (x[1] * x[2])
    s0 = (q[6] * x[0] + q[7] * x[1]) + q[8] * x[2]
    c = ((s2 + 2.0 * s1) + 2.0 * s0) + q[9]
    return c if c > 0.0 else 0.0


def place(q, plo, phi):
    """rule 4: (x, cost)"""
    a00, a01, a02, a11, a12, a22, b0, b1, b2 = q[:9]
    c00 = a11 * a22 - a12 * a12
    c01 = a02 * a12 - a01 * a22
    c02 = a01 * a12 - a02 * a11
    c11 = a00 * a22 - a02 * a02
    c12 = a01 * a02 - a00 * a12
    c22 = a00 * a11 - a01 * a01
    det = (a00 * c00 + a01 * c01) + a02 * c02
    t = (a00 + a11) + a22
    mid = [0.5 * (plo[k] + phi[k]) for k in range(3)]
    if det > DET_FLOOR * ((t * t) * t):
        x = [-((c00 * b0 + c01 * b1) + c02 * b2) / det, -((c01 * b0 + c11 * b1) + c12 * b2) / det,
             -((c02 * b0 + c12 * b1) + c22 * b2) / det]
        dx, de = _sub(x, mid), _sub(phi, plo)
        if _dot(dx, dx) <= REACH * _dot(de, de):
            return x, cost_of(q, x)
    best, best_cost = plo, cost_of(q, plo)
    for p in (phi, mid):
        c = cost_of(q, p)
        if c < best_cost:
            best, best_cost = p, c
    return list(best), best_cost


def edges_of(faces):
    """{(lo, hi): [face indices, ascending]}"""
    ef = {}
    for t, f in enumerate(faces):
        for k in range(3):
            a, b = f[k], f[(k + 1) % 3]
            ef.setdefault((min(a, b), max(a, b)), []).append(t)
    return ef


def initial_quadrics(P, faces, boundary_weight):
    """rule 1; the loop over the faces in ascending order adds to every vertex in ascending order of ITS faces"""
    ef = edges_of(faces)
    Q = [[0.0] * 10 for _ in P]
    for f in faces:
        p0 = P[f[0]]
        N = _cross(_sub(P[f[1]], p0), _sub(P[f[2]], p0))
        length = math.sqrt(_dot(N, N))
        if not length > 0.0:
            continue
        n = [N[0] / length, N[1] / length, N[2] / length]
        d = -_dot(n, p0)
        a = 0.5 * length
        for v in f:
            _add_plane(Q[v], n, d, a)
        for k in range(3):
            va, vb = f[k], f[(k + 1) % 3]
            if len(ef[(min(va, vb), max(va, vb))]) != 1:
                continue
            e = _sub(P[vb], P[va])
            m = _cross(e, n)
            ml = math.sqrt(_dot(m, m))
            if not ml > 0.0:
                continue
            m = [m[0] / ml, m[1] / ml, m[2] / ml]
            dm = -_dot(m, P[va])
            w = boundary_weight * _dot(e, e)
            _add_plane(Q[va], m, dm, w)
            _add_plane(Q[vb], m, dm, w)
    return Q


def decimate(vertices, colors, faces, target, maximum_error=INF, boundary_weight=1.0):
    """dict: positions [V, 3] float32, colors [V, 3] float32, faces [K, 3] int32, rounds, applied (collapses per round),
    window (window size per round), survivors [V] (input index of every output vertex)"""
    v32 = np.asarray(vertices, np.float32).reshape(-1, 3)
    origin = [float(v32[:, k].min()) for k in range(3)] if len(v32) else [0.0] * 3
    P = [[float(p[k]) - origin[k] for k in range(3)] for p in v32]
    C = [[float(x) for x in c] for c in np.asarray(colors, np.float32).reshape(-1, 3)]
    count = [1] * len(P)
    F = [tuple(int(i) for i in f) for f in np.asarray(faces).reshape(-1, 3)]
    F = [f for f in F if f[0] != f[1] and f[1] != f[2] and f[2] != f[0]]
    Q = initial_quadrics(P, F, float(boundary_weight))
    rnd, applied_log, window_log = 0, [], []
    while True:
        rnd += 1
        K = len(F) - target
        if K <= 0:
            break
        ef = edges_of(F)
        edges = sorted(ef)
        boundary, locked, nbr, vfaces = set(), set(), {}, {}
        for (lo, hi), fs in ef.items():
            nbr.setdefault(lo, set()).add(hi)
            nbr.setdefault(hi, set()).add(lo)
            if len(fs) == 1:
                boundary.update((lo, hi))
            if len(fs) >= 3:
                locked.update((lo, hi))
        for t, f in enumerate(F):
            for v in f:
                vfaces.setdefault(v, []).append(t)
        cands = []
        for eid, (lo, hi) in enumerate(edges):
            fs = ef[(lo, hi)]
            if len(fs) > 2 or lo in locked or hi in locked:
                continue
            if len(fs) == 2 and lo in boundary and hi in boundary:
                continue
            apexes = [next(v for v in F[t] if v != lo and v != hi) for t in fs]
            if nbr[lo] & nbr[hi] != set(apexes) or len(set(apexes)) != len(fs):
                continue
            q = [Q[lo][j] + Q[hi][j] for j in range(10)]
            x, cost = place(q, P[lo], P[hi])
            if not cost <= maximum_error:
                continue
            ok = True
            for moved, other in ((lo, hi), (hi, lo)):
                for t in vfaces[moved]:
                    f = F[t]
                    if other in f:
                        continue
                    p = [P[v] for v in f]
                    old = _cross(_sub(p[1], p[0]), _sub(p[2], p[0]))
                    p = [x if v == moved else P[v] for v in f]
                    new = _cross(_sub(p[1], p[0]), _sub(p[2], p[0]))
                    if not _dot(old, new) > 0.0:
                        ok = False
            if ok:
                cands.append((cost, eid, x))
        if not cands:
            break
        cands.sort(key=lambda c: (c[0], c[1]))
        window = cands[:max(1, K // 2)]
        mr = mix(rnd)
        ranked = sorted(window, key=lambda c: (mix((edges[c[1]][0] << 32 | edges[c[1]][1]) ^ mr) >> 1, c[1]))
        vmin = {}
        for r, (_, eid, _) in enumerate(ranked):
            for v in edges[eid]:
                vmin[v] = min(vmin.get(v, NO_RANK), r)
        vmin2 = {v: min([vmin.get(v, NO_RANK)] + [vmin.get(u, NO_RANK) for u in nbr[v]]) for v in nbr}
        total, vmap, applied = 0, {}, 0
        for r, (_, eid, x) in enumerate(ranked):
            lo, hi = edges[eid]
            if not (r == vmin2[lo] == vmin2[hi]):
                continue
            if not total < K:
                break
            total += len(ef[(lo, hi)])
            P[lo] = x
            Q[lo] = [Q[lo][j] + Q[hi][j] for j in range(10)]
            nl, nh = float(count[lo]), float(count[hi])
            C[lo] = [(nl * C[lo][k] + nh * C[hi][k]) / (nl + nh) for k in range(3)]
            count[lo] += count[hi]
            vmap[hi] = lo
            applied += 1
        applied_log.append(applied)
        window_log.append(len(window))
        F = [tuple(vmap.get(v, v) for v in f) for f in F]
        F = [f for f in F if f[0] != f[1] and f[1] != f[2] and f[2] != f[0]]
    used = sorted({v for f in F for v in f})
    new = {v: i for i, v in enumerate(used)}
    positions = np.array([[origin[k] + P[v][k] for k in range(3)] for v in used], np.float64).reshape(-1, 3).astype(np.float32)
    colours = np.array([C[v] for v in used], np.float64).reshape(-1, 3).astype(np.float32)
    return {"positions": positions, "colors": colours, "faces": np.array([[new[v] for v in f] for f in F], np.int32).reshape(-1, 3),
            "rounds": len(applied_log), "applied": applied_log, "window": window_log, "survivors": np.array(used, np.int64)}


# ---- checks ----

def exact(a, b):
    """equal shapes, dtypes and BITS (so -0.0 differs from 0.0 and a NaN equals the same NaN)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def directed_edges(faces):
    d = {}
    for f in np.asarray(faces).reshape(-1, 3):
        for k in range(3):
            e = (int(f[k]), int(f[(k + 1) % 3]))
            d[e] = d.get(e, 0) + 1
    return d


def is_closed_manifold(faces):
    """every directed edge once, and its reverse once"""
    d = directed_edges(faces)
    return len(d) > 0 and all(c == 1 and d.get((b, a), 0) == 1 for (a, b), c in d.items())


def euler_characteristic(faces):
    faces = np.asarray(faces).reshape(-1, 3)
    return len(np.unique(faces)) - len(edges_of([tuple(int(i) for i in f) for f in faces])) + len(faces)


def edge_face_counts(faces):
    return {e: len(fs) for e, fs in edges_of([tuple(int(i) for i in f) for f in np.asarray(faces).reshape(-1, 3)]).items()}


def boundary_vertices(faces):
    return sorted({v for e, c in edge_face_counts(faces).items() if c == 1 for v in e})


def polyline_distance(points, vertices, faces):
    """distance of each point to the nearest boundary edge (a segment) of the mesh"""
    vertices = np.asarray(vertices, np.float64)
    segs = [(vertices[a], vertices[b]) for (a, b), c in edge_face_counts(faces).items() if c == 1]
    out = []
    for p in np.asarray(points, np.float64).reshape(-1, 3):
        best = INF
        for a, b in segs:
            ab = b - a
            s = min(1.0, max(0.0, float(np.dot(p - a, ab) / np.dot(ab, ab))))
            best = min(best, float(np.linalg.norm(p - (a + s * ab))))
        out.append(best)
    return np.array(out)


# ---- the meshes ----

SHEET = 13   # vertices per side of the sheets


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(vertices [Nv, 3] float32, colors [Nv, 3] float32, faces [F, 3] int32)"""
    if name == "cube8":
        v, f = sref.cube(8)
    elif name == "cube16_scattered":      # cell-mates whole workgroups apart, as mesh("scattered") of the clustering's meshes
        v, f = sref.cube(16)
        perm = np.random.default_rng(41).permutation(len(v))
        inv = np.empty_like(perm)
        inv[perm] = np.arange(len(v))
        v, f = v[perm], inv[f].astype(np.int32)
    elif name == "uv_sphere24":
        v, f = sref.uv_sphere(24)
    elif name == "flat_sheet":            # open, every quadric singular: the fall-back placement and the boundary planes
        xs = np.linspace(0.1, 1.3, SHEET)
        v, f = sref._sheet(xs, xs + 0.2, lambda X, Y: 0.0 * X + 0.05, 0)
    elif name == "wavy_sheet":
        xs = np.linspace(0.1, 1.3, SHEET)
        v, f = sref._sheet(xs, xs + 0.2, lambda X, Y: 0.3 * np.sin(3.0 * X) + 0.2 * Y, 0)
    elif name == "fin":
        # a 9 x 9 sheet at z = 0.05 and a second sheet standing on its row i = 4: the edges along that row carry three faces
        xs = np.linspace(0.1, 0.9, 9)
        v0, f0 = sref._sheet(xs, xs, lambda X, Y: 0.0 * X + 0.05, 0)
        zs = 0.05 + 0.1 * np.arange(1, 5)
        first = len(v0)
        v1 = [[xs[4], y, z] for z in zs for y in xs]
        row = lambda k, j: 4 * 9 + j if k == 0 else first + (k - 1) * 9 + j
        f1 = []
        for k in range(4):
            for j in range(8):
                a, b, c, d = row(k, j), row(k, j + 1), row(k + 1, j + 1), row(k + 1, j)
                f1 += [[a, b, c], [a, c, d]]
        v, f = np.concatenate([v0, np.asarray(v1)]), f0 + f1
    elif name == "degenerate":            # faces with two equal indices and an unreferenced vertex round a small closed mesh
        v, f = sref.cube(2)
        v = np.concatenate([v, [[5.0, 5.0, 5.0]]])
        f = np.concatenate([[[0, 0, 1]], f[:5], [[3, 4, 3], [2, 2, 2]], f[5:]])
    else:
        raise KeyError(name)
    v = np.asarray(v, np.float64).astype(np.float32)
    return v, sref.vertex_colors(len(v)), np.asarray(f, np.int32).reshape(-1, 3)


# name -> (mesh, target, maximum_error, boundary_weight): the cases both test modules run
CASES = {
    "cube8": ("cube8", 12, INF, 1.0),
    "cube8_error_cap": ("cube8", 0, 1e-12, 1.0),
    "cube16_scattered": ("cube16_scattered", 200, INF, 1.0),
    "uv_sphere24": ("uv_sphere24", 300, INF, 1.0),
    "flat_sheet": ("flat_sheet", 2, INF, 1.0),
    "wavy_sheet": ("wavy_sheet", 72, INF, 1.0),
    "fin": ("fin", 60, INF, 1.0),
    "fin_weight": ("fin", 100, INF, 3.5),
    "target_above": ("degenerate", 1000, INF, 1.0),
    "open_within_one": ("flat_sheet", 201, INF, 1.0),
}


@functools.lru_cache(maxsize=None)
def expected(case):
    name, target, max_err, bw = CASES[case]
    v, c, f = mesh(name)
    return decimate(v, c, f, target, max_err, bw)
