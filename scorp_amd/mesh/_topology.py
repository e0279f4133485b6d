"""The integer tables and the float64 numpy helpers the mesh modules share: undirected edge keys, the vertex -> face CSR, the
size of an open-addressing table, the mask of faces with three distinct indices, and the cross / dot / unit every numpy
form of a csrc/mesh_*.hip kernel computes with (csrc/mesh_common.hpp's, sum for sum)."""
import numpy as np
import torch


def table_slots(entries, factor):
    """the power of two >= factor * entries"""
    return 1 << (factor * entries - 1).bit_length()


def proper_faces(faces):
    """[F] bool: the face's three indices differ (a torch tensor or a numpy array [F, 3])"""
    return (faces[:, 0] != faces[:, 1]) & (faces[:, 1] != faces[:, 2]) & (faces[:, 2] != faces[:, 0])


def edge_keys(faces):
    """[F, 3] int64: min << 32 | max of the ends of the sides (a, b), (b, c), (c, a) of every face, for a torch tensor on
    either device or a numpy array"""
    if isinstance(faces, torch.Tensor):
        a = faces.long()
        b = a.roll(-1, 1)
        return torch.minimum(a, b) << 32 | torch.maximum(a, b)
    a = faces.astype(np.int64)
    b = np.roll(a, -1, 1)
    return np.minimum(a, b) << 32 | np.maximum(a, b)


def vertex_face_csr(faces, Nv):
    """(offsets [Nv + 1] int32, faces [3 F] int32), contiguous: the faces whose corners name vertex v are
    faces[offsets[v]:offsets[v + 1]], one entry per corner, in ascending face index (the sort is stable)."""
    corners = faces.long().reshape(-1)
    offsets = torch.zeros(Nv + 1, dtype=torch.int32, device=faces.device)
    offsets[1:] = torch.cumsum(torch.bincount(corners, minlength=Nv), 0)
    return offsets, (torch.sort(corners, stable=True)[1] // 3).to(torch.int32)


# ---- numpy float64, every product and sum rounded on its own ----

def _dot3(u, w):
    return (u[..., 0] * w[..., 0] + u[..., 1] * w[..., 1]) + u[..., 2] * w[..., 2]


def _cross3(u, w):
    return np.stack([u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1], u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2],
                     u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]], -1)


def _unit(n):
    """n [..., 3] over its length; +0 where the length is zero (or NaN)"""
    with np.errstate(all="ignore"):
        length = np.sqrt(_dot3(n, n))
        ok = length > 0.0
        return np.where(ok[..., None], n / np.where(ok, length, 1.0)[..., None], 0.0)


def _face_cross(verts, faces):
    """(b - a) x (c - a) of every face (a, b, c), float64 [F, 3] from the float32 vertices: twice the face's area long"""
    v = np.asarray(verts, np.float32).astype(np.float64)
    idx = faces.astype(np.int64)
    a = v[idx[:, 0]]
    return _cross3(v[idx[:, 1]] - a, v[idx[:, 2]] - a)
