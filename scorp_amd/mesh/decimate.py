"""Edge-collapse decimation to a target triangle count: the host loop of rounds over the seven calls of
csrc/mesh_decimate.hip, or over their numpy forms for CPU tensors.  The rules are in include/scorp_gs.h."""
from functools import partial

import numpy as np
import torch

from .. import _C
from ._common import Mesh, check_mesh, drop_unreferenced, empty_mesh
from ._topology import _cross3, _dot3, edge_keys, proper_faces, vertex_face_csr

DECIMATE_DET_FLOOR = 1e-9    # rule 4: the 3x3 solve is taken iff det > this ((t t) t), t the trace
DECIMATE_REACH = 4.0         # ... and |x - mid|^2 <= this |P[hi] - P[lo]|^2
_M64 = (1 << 64) - 1


def _splitmix(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def _plane_quadric(n, d, w):
    wn, wd = w * n, w * d
    return np.array([wn[0] * n[0], wn[0] * n[1], wn[0] * n[2], wn[1] * n[1], wn[1] * n[2], wn[2] * n[2], wd * n[0], wd * n[1], wd * n[2], wd * d])


def _quadric_cost(q, x):
    s2 = (q[..., 0] * (x[..., 0] * x[..., 0]) + q[..., 3] * (x[..., 1] * x[..., 1])) + q[..., 5] * (x[..., 2] * x[..., 2])
    s1 = (q[..., 1] * (x[..., 0] * x[..., 1]) + q[..., 2] * (x[..., 0] * x[..., 2])) + q[..., 4] * (x[..., 1] * x[..., 2])
    s0 = (q[..., 6] * x[..., 0] + q[..., 7] * x[..., 1]) + q[..., 8] * x[..., 2]
    c = ((s2 + 2.0 * s1) + 2.0 * s0) + q[..., 9]
    return np.where(c > 0.0, c, 0.0)


def _quadric_place(q, plo, phi):
    """rule 4 for rows of summed quadrics [E, 10] and their ends' positions [E, 3]: (x [E, 3], cost [E])"""
    a00, a01, a02, a11, a12, a22, b0, b1, b2 = (q[:, k] for k in range(9))
    c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
    c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
    det = (a00 * c00 + a01 * c01) + a02 * c02
    t = (a00 + a11) + a22
    mid = 0.5 * (plo + phi)
    x = np.stack([-((c00 * b0 + c01 * b1) + c02 * b2) / det, -((c01 * b0 + c11 * b1) + c12 * b2) / det,
                  -((c02 * b0 + c12 * b1) + c22 * b2) / det], 1)
    dx, de = x - mid, phi - plo
    solved = (det > DECIMATE_DET_FLOOR * ((t * t) * t)) & (_dot3(dx, dx) <= DECIMATE_REACH * _dot3(de, de))   # (false for NaN)
    best, best_cost = plo, _quadric_cost(q, plo)
    for p in (phi, mid):                                          # ties stay with the earlier of lo, hi, mid
        c = _quadric_cost(q, p)
        better = c < best_cost
        best, best_cost = np.where(better[:, None], p, best), np.where(better, c, best_cost)
    return np.where(solved[:, None], x, best), np.where(solved, _quadric_cost(q, x), best_cost)


class _DecimateNumpy:
    """The seven calls of csrc/mesh_decimate.hip in Python over numpy views of CPU tensors, loop for thread: the same
    arrays go in and come out, so _decimate runs either.  For small meshes; correctness is its only duty."""

    def quadrics(self, P, faces, face_edge, edge_faces, vf_start, vf_face, bw, Q):
        P, f, fe, ef, start, vf, Q = (a.numpy() for a in (P, faces, face_edge, edge_faces, vf_start, vf_face, Q))
        with np.errstate(all="ignore"):
            for v in range(P.shape[0]):
                q = np.zeros(10)
                for t in vf[start[v]:start[v + 1]]:
                    i = f[t]
                    p = P[i]
                    N = _cross3(p[1] - p[0], p[2] - p[0])
                    length = np.sqrt(_dot3(N, N))
                    if not length > 0.0:
                        continue
                    n = N / length
                    q += _plane_quadric(n, -_dot3(n, p[0]), 0.5 * length)
                    for k in range(3):
                        a, b = k, (k + 1) % 3
                        if (i[a] != v and i[b] != v) or ef[fe[t, k]] != 1:
                            continue
                        e = p[b] - p[a]
                        M = _cross3(e, n)
                        ml = np.sqrt(_dot3(M, M))
                        if not ml > 0.0:
                            continue
                        m = M / ml
                        q += _plane_quadric(m, -_dot3(m, p[a]), bw * _dot3(e, e))
                Q[v] = q

    def flags(self, keys, edge_faces, flags):
        k, ef, fl = keys.numpy(), edge_faces.numpy(), flags.numpy()
        fl[:] = 0
        bits = (ef == 1) * 1 + (ef >= 3) * 2
        for ends in (k >> 32, k & 0xFFFFFFFF):
            np.bitwise_or.at(fl, ends, bits.astype(np.int32))

    def candidates(self, P, Q, faces, keys, edge_faces, vf_start, vf_face, flags, max_err, cost, x):
        P, Q, f, k, ef, start, vf, fl, cost, x = (a.numpy() for a in (P, Q, faces, keys, edge_faces, vf_start, vf_face, flags, cost, x))
        cost[:] = np.inf
        with np.errstate(all="ignore"):
            los, his = k >> 32, k & 0xFFFFFFFF
            x[:], costs = _quadric_place(Q[los] + Q[his], P[los], P[his])
            for e in range(k.shape[0]):
                lo, hi, n, xe, c = int(los[e]), int(his[e]), int(ef[e]), x[e], costs[e]
                if n > 2 or (fl[lo] | fl[hi]) & 2 or (n == 2 and fl[lo] & 1 and fl[hi] & 1) or not c <= max_err:
                    continue
                of_lo, of_hi = f[vf[start[lo]:start[lo + 1]]], f[vf[start[hi]:start[hi + 1]]]
                both = (of_lo == hi).any(1)
                apexes = of_lo[both][(of_lo[both] != lo) & (of_lo[both] != hi)]
                if len(apexes) != n or len(set(apexes.tolist())) != n:
                    continue
                ring = of_lo[~both]                                   # the faces with lo alone: no vertex next to hi but an apex
                among = lambda a, b: (a[..., None] == b.reshape(-1)).any(-1)
                if (among(ring, of_hi) & (ring != lo) & ~among(ring, apexes)).any():
                    continue
                tri = np.concatenate([ring, of_hi[~(of_hi == lo).any(1)]])   # rule 5 over the faces with one end
                moved = np.concatenate([np.full(len(ring), lo), np.full(len(tri) - len(ring), hi)])
                p = P[tri]
                q = np.where((tri == moved[:, None])[..., None], xe, p)
                if (_dot3(_cross3(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), _cross3(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0])) > 0.0).all():
                    cost[e] = c

    def hash(self, keys, window, rnd, out):
        k, mr = keys.numpy(), _splitmix(rnd)
        out.numpy()[:] = [_splitmix(int(k[e]) ^ mr) >> 1 for e in window.numpy()]

    def select(self, keys, ranked, vmin, vmin2, selected):
        k, rk, vmin, vmin2, sel = (a.numpy() for a in (keys, ranked, vmin, vmin2, selected))
        lo, hi = k >> 32, k & 0xFFFFFFFF
        vmin[:] = 2 ** 31 - 1
        rank = np.arange(rk.shape[0], dtype=np.int32)
        np.minimum.at(vmin, lo[rk], rank)
        np.minimum.at(vmin, hi[rk], rank)
        vmin2[:] = vmin
        np.minimum.at(vmin2, lo, vmin[hi])
        np.minimum.at(vmin2, hi, vmin[lo])
        sel[:] = (vmin2[lo[rk]] == rank) & (vmin2[hi[rk]] == rank)

    def apply(self, keys, ranked, applied, x, P, Q, C, count, vmap):
        k, rk, ap, x, P, Q, C, count, vmap = (a.numpy() for a in (keys, ranked, applied, x, P, Q, C, count, vmap))
        vmap[:] = np.arange(vmap.shape[0])
        for r in np.flatnonzero(ap):
            e = rk[r]
            lo, hi = int(k[e] >> 32), int(k[e] & 0xFFFFFFFF)
            P[lo] = x[e]
            Q[lo] = Q[lo] + Q[hi]
            nl, nh = float(count[lo]), float(count[hi])
            C[lo] = (nl * C[lo] + nh * C[hi]) / (nl + nh)
            count[lo] += count[hi]
            vmap[hi] = lo

    def faces(self, faces, vmap, out_faces, keep):
        m = vmap.numpy()[faces.numpy()]
        out_faces.numpy()[:] = m
        keep.numpy()[:] = proper_faces(m)


class _DecimateHip:
    """The seven entry points of csrc/mesh_decimate.hip on the current stream"""

    def quadrics(self, P, faces, face_edge, edge_faces, vf_start, vf_face, bw, Q):
        _C.call("scorp_mesh_decimate_quadrics", P, P.shape[0], faces, faces.shape[0], face_edge, edge_faces, edge_faces.shape[0],
                vf_start, vf_face, bw, Q)

    def flags(self, keys, edge_faces, flags):
        _C.call("scorp_mesh_decimate_flags", keys, edge_faces, keys.shape[0], flags.shape[0], flags)

    def candidates(self, P, Q, faces, keys, edge_faces, vf_start, vf_face, flags, max_err, cost, x):
        _C.call("scorp_mesh_decimate_candidates", P, Q, P.shape[0], faces, faces.shape[0], keys, edge_faces, keys.shape[0], vf_start,
                vf_face, flags, max_err, cost, x)

    def hash(self, keys, window, rnd, out):
        _C.call("scorp_mesh_decimate_hash", keys, keys.shape[0], window, window.shape[0], rnd, out)

    def select(self, keys, ranked, vmin, vmin2, selected):
        _C.call("scorp_mesh_decimate_select", keys, keys.shape[0], ranked, ranked.shape[0], vmin.shape[0], vmin, vmin2, selected)

    def apply(self, keys, ranked, applied, x, P, Q, C, count, vmap):
        _C.call("scorp_mesh_decimate_apply", keys, keys.shape[0], ranked, applied, ranked.shape[0], x, P.shape[0], P, Q, C, count, vmap)

    def faces(self, faces, vmap, out_faces, keep):
        _C.call("scorp_mesh_decimate_faces", faces, faces.shape[0], vmap, vmap.shape[0], out_faces, keep)


def _decimate_tables(faces, Nv):
    """One `unique` and one stable sort over the current faces: (edge_keys [E] int64 ascending, face_edge [F, 3] int32,
    edge_faces [E] int32, vf_start [Nv + 1] int32, vf_face [3 F] int32)."""
    keys, inverse, counts = torch.unique(edge_keys(faces).reshape(-1), return_inverse=True, return_counts=True)
    return (keys, inverse.reshape(-1, 3).to(torch.int32).contiguous(), counts.to(torch.int32)) + vertex_face_csr(faces, Nv)


def _decimate(verts, colors, faces, target, max_err, bw, ops, rounds=None):
    """Rules 0 - 11 on tensors of one device; `ops` runs the seven calls.  rounds (a list) receives (faces, edges, window,
    applied faces) of every round."""
    dev, Nv = verts.device, verts.shape[0]
    new = partial(torch.empty, device=dev)
    origin = verts.amin(0).double()
    P = (verts.double() - origin).contiguous()
    C = colors.double().contiguous()
    count = torch.ones(Nv, dtype=torch.int32, device=dev)
    faces = faces[proper_faces(faces)].contiguous()
    Q = new(Nv, 10, dtype=torch.float64)
    flags, vmin, vmin2, vmap = (new(Nv, dtype=torch.int32) for _ in range(4))
    rnd = 0
    while faces.shape[0] > target:
        rnd += 1
        F = faces.shape[0]
        K = F - target
        keys, face_edge, edge_faces, vf_start, vf_face = _decimate_tables(faces, Nv)
        if rnd == 1:
            ops.quadrics(P, faces, face_edge, edge_faces, vf_start, vf_face, bw, Q)
        E = keys.shape[0]
        ops.flags(keys, edge_faces, flags)
        cost, x = new(E, dtype=torch.float64), new(E, 3, dtype=torch.float64)
        ops.candidates(P, Q, faces, keys, edge_faces, vf_start, vf_face, flags, max_err, cost, x)
        by_cost = torch.sort(cost, stable=True)[1]                # (cost, edge number) ascending: +inf, no candidate, last
        candidates = int((cost < float("inf")).sum())             # the one count the host reads per round
        if candidates == 0:
            break
        W = min(max(1, K // 2), candidates)
        window = torch.sort(by_cost[:W])[0].to(torch.int32)
        h = new(W, dtype=torch.int64)
        ops.hash(keys, window, rnd, h)
        ranked = window[torch.sort(h, stable=True)[1]].contiguous()   # (h, edge number) ascending
        selected = new(W, dtype=torch.uint8)
        ops.select(keys, ranked, vmin, vmin2, selected)
        taken = edge_faces[ranked.long()].long() * selected
        applied = (selected.bool() & (torch.cumsum(taken, 0) - taken < K)).to(torch.uint8)
        ops.apply(keys, ranked, applied, x, P, Q, C, count, vmap)
        mapped, keep = new(F, 3, dtype=torch.int32), new(F, dtype=torch.uint8)
        ops.faces(faces, vmap, mapped, keep)
        faces = mapped[keep.bool()].contiguous()
        if rounds is not None:
            rounds.append((F, E, W, F - faces.shape[0]))
    P, faces, C = drop_unreferenced(P, faces, C)
    return Mesh((origin + P).float(), faces, C.float())


def simplify_quadric_decimation(mesh, target_number_of_triangles, maximum_error=float("inf"), boundary_weight=1.0, rounds=None):
    """Reduce a Mesh to `target_number_of_triangles` by edge collapses placed by quadric error (the use of Open3D's
    simplify_quadric_decimation and of the simplify step of TRELLIS post-processing; the rules are this project's own, rules
    0 - 11 of the decimation block of include/scorp_gs.h, and were never compared with Open3D's output).  Every vertex
    carries the quadric of its faces' planes, and `boundary_weight` times a plane through every open edge; an edge collapses
    to the minimiser of its ends' summed quadrics.  Each ROUND evaluates every edge, takes the cheapest half of what is still
    to go as its window, and collapses an independent set of the window at once (no two collapses share or neighbour a
    vertex), chosen by a hash so that it is large; edges whose collapse would cost more than `maximum_error`, flip a
    triangle, pinch the surface (link condition) or touch an edge with three or more faces are never taken.  The result has
    target or target - 1 triangles when the target can be reached, more when the rules stop first, and is a function of the
    input alone: two runs agree bit for bit.  Faces with two equal indices and vertices no face references are dropped.
    `rounds`, a list, receives (faces, edges, window, faces removed) of every round.
    Returns a new Mesh on the mesh's device.  CUDA tensors run csrc/mesh_decimate.hip, with the sorts, `unique` and scans
    in torch between the calls; CPU tensors run a Python / numpy form of the same rules, meant for small meshes.

        mesh = simplify_quadric_decimation(post_process_mesh(ex.extract_mesh_unbounded(resolution=1024)), 200_000)
    """
    target, max_err, bw = int(target_number_of_triangles), float(maximum_error), float(boundary_weight)
    if target < 0:
        raise ValueError(f"target_number_of_triangles must not be negative; got {target_number_of_triangles}")
    if not max_err >= 0.0:
        raise ValueError(f"maximum_error must not be negative or NaN; got {maximum_error}")
    if not (bw >= 0.0 and np.isfinite(bw)):
        raise ValueError(f"boundary_weight must be finite and not negative; got {boundary_weight}")
    checked = check_mesh(mesh)
    dev = mesh.vertices.device
    if checked is None:
        return empty_mesh(dev)
    verts, faces, colors, _ = checked
    if dev.type != "cuda":
        return _decimate(verts, colors, faces, target, max_err, bw, _DecimateNumpy(), rounds)
    with torch.cuda.device(dev):
        return _decimate(verts, colors, faces, target, max_err, bw, _DecimateHip(), rounds)
