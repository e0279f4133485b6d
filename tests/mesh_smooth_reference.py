"""The yardstick of the mesh-smooth tests: the rules of the mesh-smooth block of include/scorp_gs.h restated as per-vertex loops
over Python sets, lists and floats - another formulation than scorp_amd/mesh/smooth.py's sorted 64-bit keys and vectorised
numpy.  A Python float is an IEEE double, `*`, `+`, `-`, `/` and math.sqrt round correctly and CPython fuses nothing, so
every statement below is the rule's own arithmetic; np.float32 rounds where a rule says so and nowhere else."""
import math

import numpy as np


def adjacency(num_vertices, faces):
    """rules 1 - 4: (neighbours: a sorted list per vertex, corners: a list of face indices per vertex, boundary: a bool per
    vertex)"""
    near = [set() for _ in range(num_vertices)]
    corners = [[] for _ in range(num_vertices)]
    seen = {}
    for index, face in enumerate(faces):
        a, b, c = (int(k) for k in face)
        for u, v in ((a, b), (b, c), (c, a)):
            if u == v:
                continue
            near[u].add(v)
            near[v].add(u)
            side = (min(u, v), max(u, v))
            seen[side] = seen.get(side, 0) + 1
        for u in (a, b, c):
            corners[u].append(index)
    boundary = [False] * num_vertices
    for (u, v), times in seen.items():
        if times == 1:
            boundary[u] = boundary[v] = True
    return [sorted(s) for s in near], corners, boundary


def _point(verts, k):
    return float(verts[k][0]), float(verts[k][1]), float(verts[k][2])


def cross(verts, face):
    """rule 5: (b - a) x (c - a)"""
    a, b, c = (_point(verts, int(k)) for k in face)
    e1 = (b[0] - a[0], b[1] - a[1], b[2] - a[2])
    e2 = (c[0] - a[0], c[1] - a[1], c[2] - a[2])
    return (e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0])


def unit(n):
    """rule 5: n over its length, +0 for no length"""
    length = math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
    if length == 0.0:
        return (0.0, 0.0, 0.0)
    return (n[0] / length, n[1] / length, n[2] / length)


def face_normals(verts, faces, normalized=True):
    out = [unit(cross(verts, f)) if normalized else cross(verts, f) for f in faces]
    return np.array(out, np.float64).reshape(-1, 3).astype(np.float32)


def vertex_normals(verts, faces, weighting):
    """rule 6"""
    _, corners, _ = adjacency(len(verts), faces)
    per_face = [cross(verts, f) for f in faces]
    if weighting == "uniform":
        per_face = [unit(n) for n in per_face]
    out = []
    for mine in corners:
        sx = sy = sz = 0.0
        for f in mine:
            sx = sx + per_face[f][0]
            sy = sy + per_face[f][1]
            sz = sz + per_face[f][2]
        out.append(unit((sx, sy, sz)))
    return np.array(out, np.float64).reshape(-1, 3).astype(np.float32)


def half_step(verts, near, fixed, factor, weights):
    """rule 7 on float32 positions: a new float32 array"""
    out = np.array(verts, np.float32)
    for v, mine in enumerate(near):
        if not mine or (fixed is not None and fixed[v]):
            continue
        p = _point(verts, v)
        sx = sy = sz = total = 0.0
        for j in mine:
            q = _point(verts, j)
            w = 1.0
            if weights == "inverse_distance":
                dx, dy, dz = p[0] - q[0], p[1] - q[1], p[2] - q[2]
                w = 1.0 / (math.sqrt((dx * dx + dy * dy) + dz * dz) + 1e-12)
            sx = sx + w * q[0]
            sy = sy + w * q[1]
            sz = sz + w * q[2]
            total = total + w
        out[v] = (np.float32(p[0] + factor * (sx / total - p[0])), np.float32(p[1] + factor * (sy / total - p[1])),
                  np.float32(p[2] + factor * (sz / total - p[2])))
    return out


def half_steps(verts, faces, factors, weights="uniform", fix_boundary=False):
    """rule 8: the positions after each of the half-steps `factors`, a list as long (filter_smooth_laplacian(n) is the entry
    n - 1 of [lambda] * n, filter_smooth_taubin(n) the entry 2 n - 1 of [lambda, mu] * n)"""
    near, _, boundary = adjacency(len(verts), faces)
    out, cur = [], np.array(verts, np.float32)
    for f in factors:
        cur = half_step(cur, near, boundary if fix_boundary else None, float(f), weights)
        out.append(cur)
    return out


def normal_map(verts, faces, normals, face_map, bary):
    """per pixel of face_map [V, H, W]: the face's unit normal (normals None) or the normalised barycentric mix of its corners'
    normals; float32 [V, 3, H, W]"""
    V, H, W = face_map.shape
    out = np.zeros((V, 3, H, W), np.float32)
    flat = {}
    for v, j, i in zip(*np.nonzero(face_map >= 0)):
        f = int(face_map[v, j, i])
        if normals is None:
            if f not in flat:
                flat[f] = unit(cross(verts, faces[f]))
            n = flat[f]
        else:
            b = [float(bary[v, k, j, i]) for k in range(3)]
            N = [_point(normals, int(k)) for k in faces[f]]
            n = unit(tuple((b[0] * N[0][ch] + b[1] * N[1][ch]) + b[2] * N[2][ch] for ch in range(3)))
        out[v, :, j, i] = n
    return out
