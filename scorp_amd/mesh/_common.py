"""What the mesh modules share: the Mesh dataclass, the empty mesh, the compaction that drops unreferenced vertices, the
argument checks of the two simplifiers, and the names of the two extraction methods."""
from dataclasses import dataclass

import numpy as np
import torch

MAX_CLUSTER_FACES = 1 << 28       # the C ABI's bound on triangles (include/scorp_gs.h)
MAX_SIMPLIFY_VERTICES = 1 << 30   # the C ABI's bound on the vertices of a mesh to simplify
METHODS = ("surface_nets", "marching_cubes")


@dataclass
class Mesh:
    """vertices [Nv, 3] float32, faces [Nf, 3] int32 (vertex indices), colors [Nv, 3] float32 in [0, 1]."""
    vertices: torch.Tensor
    faces: torch.Tensor
    colors: torch.Tensor


def empty_mesh(dev):
    return Mesh(torch.empty(0, 3, dtype=torch.float32, device=dev), torch.empty(0, 3, dtype=torch.int32, device=dev),
                torch.empty(0, 3, dtype=torch.float32, device=dev))


def _check_method(method):
    if method not in METHODS:
        raise ValueError(f"method must be one of {METHODS}; got {method!r}")


def drop_unreferenced(vertices, faces, colors):
    """Drop the vertices no face references: (vertices[used], faces [F, 3] int32 contiguous re-indexed, colors[used]) on the
    faces' device.  The survivors keep their order and their dtypes, the colours travel with them."""
    faces = faces.long()
    used = torch.zeros(vertices.shape[0], dtype=torch.bool, device=faces.device)
    used[faces.reshape(-1)] = True
    faces = (torch.cumsum(used, 0, dtype=torch.int32) - 1)[faces]
    return vertices[used], faces.contiguous(), colors[used]


def check_mesh(mesh, extent=None):
    """The argument checks cluster_vertices and simplify_quadric_decimation share.  None for an empty mesh (no vertices or no
    faces), else (vertices float32, faces int32, colors float32, lo [3]): contiguous on the vertices' device, lo the
    vertices' minimum per axis.  `extent`, when given, is called with the float64 ends [2, 3] of the bounding box once the
    vertices are known to be finite and before the faces' indices are looked at."""
    verts, faces, colors = mesh.vertices, mesh.faces, mesh.colors
    if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype.is_floating_point:
        raise ValueError("vertices must be [Nv, 3] and faces an integer tensor [F, 3]")
    dev = verts.device
    Nv, F = verts.shape[0], faces.shape[0]
    if colors.dim() != 2 or tuple(colors.shape) != (Nv, 3):
        raise ValueError(f"{colors.shape[0]} colours for {Nv} vertices")
    if Nv > MAX_SIMPLIFY_VERTICES or F > MAX_CLUSTER_FACES:
        raise ValueError(f"more than 2^30 vertices or 2^28 triangles: {Nv}, {F}")
    if F == 0 or Nv == 0:
        return None
    verts = verts.to(torch.float32).contiguous()
    colors = colors.to(device=dev, dtype=torch.float32).contiguous()
    lo, hi = verts.amin(0), verts.amax(0)
    ends = torch.stack([lo, hi]).cpu().numpy().astype(np.float64)
    if not np.isfinite(ends).all():   # (a NaN or an infinity anywhere reaches the minimum or the maximum)
        raise ValueError("the vertices are not all finite")
    if extent is not None:
        extent(ends)
    fmin, fmax = int(faces.min()), int(faces.max())
    if fmin < 0 or fmax >= Nv:
        raise ValueError(f"vertex index {fmin if fmin < 0 else fmax} with {Nv} vertices")
    return verts, faces.to(device=dev, dtype=torch.int32).contiguous(), colors, lo
