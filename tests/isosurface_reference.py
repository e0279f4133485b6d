"""Yardstick of the surface extraction (csrc/isosurface.hip, scorp_amd.mesh.extract_surface): naive surface nets in numpy
float64 with the vertex and face order of include/scorp_gs.h, written as plain loops over the active cells and the
crossed lattice edges, plus the analytic fields of the tests and the mesh invariants they check."""
import numpy as np

SHAPE = (24, 20, 28)   # unequal spacing per axis below


def lattice():
    return (np.linspace(-1.0, 1.0, SHAPE[0]).astype(np.float32), np.linspace(-1.1, 1.1, SHAPE[1]).astype(np.float32),
            np.linspace(-1.2, 1.2, SHAPE[2]).astype(np.float32))


def max_edge(coords):
    return max(float(np.diff(c.astype(np.float64)).max()) for c in coords)


def field(name, coords=None):
    """fp32 grid of an analytic signed distance over the lattice: sphere (r = 0.7, off-centre), torus (R = 0.6, r = 0.25,
    axis z), plane (tilted, leaves the grid through its faces), none (no crossing)."""
    x, y, z = (c.astype(np.float64) for c in (coords or lattice()))
    X, Y, Z = np.meshgrid(x, y, z, indexing="ij")
    if name == "sphere":
        f = np.sqrt((X - 0.03) ** 2 + (Y + 0.02) ** 2 + (Z - 0.05) ** 2) - 0.7
    elif name == "torus":
        f = np.sqrt((np.sqrt(X ** 2 + Y ** 2) - 0.6) ** 2 + Z ** 2) - 0.25
    elif name == "plane":
        f = 0.3 * X + 0.5 * Y + 0.8 * Z - 0.1
    elif name == "none":
        f = np.ones_like(X)
    else:
        raise KeyError(name)
    return f.astype(np.float32)


def surface_nets(f, coords, level=0.0):
    """(vertices [Nv,3] float64, faces [Nf,3] int64).  f [X,Y,Z] (its fp32 values, taken to float64), inside: f < level."""
    f = np.asarray(f).astype(np.float64)
    x, y, z = (np.asarray(c).astype(np.float64) for c in coords)
    X, Y, Z = f.shape
    inside = f < level
    n_in = sum(inside[di:X - 1 + di, dj:Y - 1 + dj, dk:Z - 1 + dk].astype(np.int64)
               for di in (0, 1) for dj in (0, 1) for dk in (0, 1))
    active = (n_in > 0) & (n_in < 8)
    vid = -np.ones(active.shape, np.int64)
    verts = []
    for i, j, k in np.argwhere(active):                      # ascending linear cell index
        acc, n = np.zeros(3), 0
        for axis in range(3):                                # x-edges, then y-edges, then z-edges
            step = 4 >> axis
            for n0 in range(8):                              # by ascending first corner (corner = 4 di + 2 dj + dk)
                if n0 & step:
                    continue
                o = np.array([n0 >> 2, (n0 >> 1) & 1, n0 & 1])
                e = np.zeros(3, np.int64)
                e[axis] = 1
                p0, p1 = (i, j, k) + o, (i, j, k) + o + e
                if inside[tuple(p0)] == inside[tuple(p1)]:
                    continue
                f0, f1 = f[tuple(p0)], f[tuple(p1)]
                pt = o.astype(np.float64)
                pt[axis] = (level - f0) / (f1 - f0)
                acc += pt
                n += 1
        frac = acc / n
        vid[i, j, k] = len(verts)
        verts.append([x[i] + frac[0] * (x[i + 1] - x[i]), y[j] + frac[1] * (y[j + 1] - y[j]), z[k] + frac[2] * (z[k + 1] - z[k])])
    faces = []
    dims = (X, Y, Z)
    for q in np.ndindex(X, Y, Z):                            # ascending linear lattice index
        q = np.array(q)
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            if q[a] + 1 >= dims[a] or not (1 <= q[b] <= dims[b] - 2) or not (1 <= q[c] <= dims[c] - 2):
                continue
            q1 = q.copy()
            q1[a] += 1
            if inside[tuple(q)] == inside[tuple(q1)]:
                continue
            eb, ec = np.zeros(3, np.int64), np.zeros(3, np.int64)
            eb[b], ec[c] = 1, 1
            c00, c10, c11, c01 = (vid[tuple(p)] for p in (q, q - eb, q - eb - ec, q - ec))
            if inside[tuple(q)]:
                faces += [[c00, c10, c11], [c00, c11, c01]]
            else:
                faces += [[c00, c11, c10], [c00, c01, c11]]
    return np.array(verts, np.float64).reshape(-1, 3), np.array(faces, np.int64).reshape(-1, 3)


# ---- invariants ----

def directed_edges(faces):
    return np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])


def is_closed_and_oriented(faces):
    """Every undirected edge lies in exactly two triangles, once in each direction."""
    e = directed_edges(faces)
    fwd = {}
    for a, b in e:
        fwd[(a, b)] = fwd.get((a, b), 0) + 1
    return all(n == 1 and fwd.get((b, a), 0) == 1 for (a, b), n in fwd.items())


def euler_characteristic(verts, faces):
    e = np.sort(directed_edges(faces), axis=1)
    return len(verts) - len(np.unique(e, axis=0)) + len(faces)


def signed_volume(verts, faces):
    a, b, c = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)
