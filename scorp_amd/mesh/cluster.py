"""Triangle clustering over shared edges (csrc/mesh_cluster.hip, with a numpy form for CPU tensors) and the floater removal of
post_process_mesh built on it."""
import numpy as np
import torch

from .. import _C
from ._common import MAX_CLUSTER_FACES, Mesh, drop_unreferenced, empty_mesh
from ._topology import _dot3, _face_cross, edge_keys, proper_faces, table_slots

MIN_CLUSTER_TRIANGLES = 50    # mesh_utils.py:36: no cluster below it is ever kept


def _cluster_numpy(f, verts):
    """The rules of include/scorp_gs.h (connected triangles) in numpy: the 3F edge_keys grouped by np.unique, then every
    triangle takes the smallest label on its edges and the labels are pointer-jumped, until nothing changes.  A label is
    always a triangle of the same component, so the fixed point is the component's smallest triangle index."""
    F = f.shape[0]
    _, edge = np.unique(edge_keys(f).reshape(-1), return_inverse=True)   # edge e of triangle t at 3 t + e
    edge = edge.reshape(-1)
    order = np.argsort(edge, kind="stable")
    tri = order // 3                                                        # the triangles edge by edge
    starts = np.flatnonzero(np.diff(edge[order], prepend=-1))
    label = np.arange(F, dtype=np.int64)
    while True:
        edge_min = np.minimum.reduceat(label[tri], starts)
        new = np.minimum(label, edge_min[edge].reshape(F, 3).min(1))
        while True:
            jumped = new[new]
            if np.array_equal(jumped, new):
                break
            new = jumped
        if np.array_equal(new, label):
            break
        label = new
    is_root = label == np.arange(F)
    cluster = (np.cumsum(is_root) - 1)[label].astype(np.int32)
    C = int(is_root.sum())
    counts = np.bincount(cluster, minlength=C).astype(np.int32)
    area = None
    if verts is not None:   # 0.5 |(v1 - v0) x (v2 - v0)| per triangle
        n = _face_cross(verts, f)
        area = np.bincount(cluster, weights=0.5 * np.sqrt(_dot3(n, n)), minlength=C)
    return cluster, counts, area


def cluster_connected_triangles(faces, vertices=None):
    """Open3D's TriangleMesh.cluster_connected_triangles on faces [F, 3] (integer vertex indices): (triangle_clusters [F]
    int32, cluster_n_triangles [C] int32, cluster_area [C] float64 - None without `vertices` [Nv, 3]) on faces' device.
    Triangles are adjacent when they share an edge (a pair of vertex indices); clusters are numbered by their smallest
    triangle index (include/scorp_gs.h).  CUDA tensors run csrc/mesh_cluster.hip, CPU tensors a numpy form of the same rules."""
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype.is_floating_point \
            or faces.dtype.is_complex or faces.dtype == torch.bool:
        raise ValueError("faces must be an integer tensor [F, 3]")
    dev = faces.device
    F = faces.shape[0]
    if F > MAX_CLUSTER_FACES:
        raise ValueError(f"more than 2^28 triangles: {F}")
    if vertices is not None:
        if not isinstance(vertices, torch.Tensor) or vertices.dim() != 2 or vertices.shape[1] != 3:
            raise ValueError("vertices must be [Nv, 3]")
        vertices = vertices.to(device=dev, dtype=torch.float32).contiguous()
    if F == 0:
        return (torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev),
                torch.empty(0, dtype=torch.float64, device=dev) if vertices is not None else None)
    lo, hi = int(faces.min()), int(faces.max())
    if lo < 0:
        raise ValueError(f"negative vertex index {lo}")
    if hi > 2 ** 31 - 1:
        raise ValueError(f"vertex index {hi} above 2^31 - 1")
    if vertices is not None and hi >= vertices.shape[0]:
        raise ValueError(f"vertex index {hi} with {vertices.shape[0]} vertices")
    faces = faces.to(torch.int32).contiguous()
    if dev.type != "cuda":
        cluster, counts, area = _cluster_numpy(faces.numpy(), vertices.numpy() if vertices is not None else None)
        return torch.from_numpy(cluster), torch.from_numpy(counts), torch.from_numpy(area) if area is not None else None
    slots = table_slots(F, 6)
    with torch.cuda.device(dev):
        keys = torch.empty(slots, dtype=torch.int64, device=dev)
        owner = torch.empty(slots, dtype=torch.int32, device=dev)
        parent = torch.empty(F, dtype=torch.int32, device=dev)
        _C.call("scorp_mesh_cluster_link", faces, F, keys, owner, slots, parent)
        del keys, owner
        root = torch.empty(F, dtype=torch.int32, device=dev)
        is_root = torch.empty(F, dtype=torch.uint8, device=dev)
        _C.call("scorp_mesh_cluster_roots", parent, F, root, is_root)
        root_scan = torch.cumsum(is_root, 0, dtype=torch.int32)
        C = int(root_scan[-1])
        cluster = torch.empty(F, dtype=torch.int32, device=dev)
        counts = torch.empty(C, dtype=torch.int32, device=dev)
        area = torch.empty(C, dtype=torch.float64, device=dev) if vertices is not None else None
        _C.call("scorp_mesh_cluster_stats", faces, vertices, vertices.shape[0] if vertices is not None else 0, root, root_scan, F, C,
                cluster, counts, area)
    return cluster, counts, area


def post_process_mesh(mesh, cluster_to_keep=1000):
    """mesh_utils.py:22-43, statement for statement, on the mesh's device: cluster the triangles, n = the size of the
    `cluster_to_keep`-th largest cluster (ties keep every cluster of that size) and at least 50, drop the triangles of
    smaller clusters, drop the vertices no remaining triangle references (survivors keep their order, colours travel with
    them, faces are re-indexed), last drop the triangles with two equal indices.  Returns a new Mesh.

    Departure from the reference: with fewer than `cluster_to_keep` clusters its negative index raises IndexError; here the
    smallest cluster's size stands in, so every cluster of at least 50 triangles is kept."""
    cluster_to_keep = int(cluster_to_keep)
    if cluster_to_keep < 1:
        raise ValueError(f"cluster_to_keep must be at least 1; got {cluster_to_keep}")
    verts, faces, colors = mesh.vertices, mesh.faces, mesh.colors
    dev = faces.device
    Nv = verts.shape[0]
    if colors.shape[0] != Nv:
        raise ValueError(f"{colors.shape[0]} colours for {Nv} vertices")
    if faces.shape[0] == 0:
        return empty_mesh(dev)
    if int(faces.max()) >= Nv:
        raise ValueError(f"vertex index {int(faces.max())} with {Nv} vertices")
    triangle_clusters, cluster_n_triangles, _ = cluster_connected_triangles(faces)
    C = cluster_n_triangles.numel()
    n = torch.sort(cluster_n_triangles)[0][C - min(cluster_to_keep, C)].clamp(min=MIN_CLUSTER_TRIANGLES)
    verts, faces, colors = drop_unreferenced(verts, faces[cluster_n_triangles[triangle_clusters.long()] >= n], colors)
    faces = faces[proper_faces(faces)]
    return Mesh(verts.to(torch.float32), faces.contiguous(), colors.to(torch.float32))
