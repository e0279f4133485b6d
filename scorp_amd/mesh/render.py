"""Looking at a mesh: depth, face, barycentric and colour maps of a triangle mesh from any number of cameras, the number of
views in which each face owns a pixel, and the culling and the image-space comparison built on them (csrc/mesh_render.hip,
or a numpy form of the same statements for CPU tensors).  The rules are the mesh-render block of include/scorp_gs.h; three of
them are this project's own (positions snapped to 1/256 pixel, no clipping against the near plane, equal depths to the lower
face index) and nothing was compared with Open3D's or any other renderer's output."""
from dataclasses import dataclass
from typing import NamedTuple, Optional

import numpy as np
import torch

from .. import _C
from ._common import Mesh, check_mesh, drop_unreferenced

WORKSPACE_CAP = 2 << 30          # bytes of workspace one call may take: the views are rendered in chunks that stay below it
MAX_RENDER_VIEWS = 65535         # the C ABI's bounds on the views of one call and on the image's sides
MAX_RENDER_SIDE = 16384
SNAP = 256                       # rule 2: positions in 1/256 pixel ...
SNAP_LIMIT = 1 << 29             # ... of at most this size
_CHUNK_PAIRS = 1 << 21           # (face, pixel) pairs per trip of the numpy form
_EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


class MeshRender(NamedTuple):
    """depth [V, H, W] float32 (0: no face), face [V, H, W] int32 (-1: no face), color [V, 3, H, W] float32 or None,
    barycentric [V, 3, H, W] float32 (the weights of the face's three corners, in its own order) or None"""
    depth: torch.Tensor
    face: torch.Tensor
    color: Optional[torch.Tensor]
    barycentric: Optional[torch.Tensor]


@dataclass
class DepthDifference:
    """Per view, [V] float64: mean_abs and max_abs of |mesh - reference| over the pixels where both are > 0 (NaN and 0 where
    there is none), reference_covered = the share of the reference's pixels (> 0) where the mesh has one too, mesh_covered
    the share of the mesh's where the reference has.  overall: the same four figures over all views' pixels together."""
    mean_abs: torch.Tensor
    max_abs: torch.Tensor
    reference_covered: torch.Tensor
    mesh_covered: torch.Tensor
    overall: dict


# ---- the numpy form ----

def _project_numpy(verts, m, H, W, near):
    """rules 1 and 2 for one view: (X, Y int64, inv_w float64 - 0 where the vertex is unusable)"""
    x, y, z = (verts[:, k].astype(np.float64) for k in range(3))
    m = m.astype(np.float64).reshape(4, 4)
    p0, p1, w = ((z * m[2, j] + (y * m[1, j] + x * m[0, j])) + m[3, j] for j in (0, 1, 3))
    inv_w = 1.0 / w
    sx = ((p0 * inv_w + 1.0) * float(W) - 1.0) * 0.5
    sy = ((p1 * inv_w + 1.0) * float(H) - 1.0) * 0.5
    fx, fy = np.floor(sx * 256.0 + 0.5), np.floor(sy * 256.0 + 0.5)
    ok = (w > near) & (w < np.inf) & (np.abs(fx) <= float(SNAP_LIMIT)) & (np.abs(fy) <= float(SNAP_LIMIT))
    return np.where(ok, fx, 0.0).astype(np.int64), np.where(ok, fy, 0.0).astype(np.int64), np.where(ok, inv_w, 0.0)


def _edge(ax, ay, bx, by, px, py):
    return (by - ay) * (px - ax) - (bx - ax) * (py - ay)


def _top_left(ax, ay, bx, by):
    return (by - ay > 0) | ((by - ay == 0) & (bx - ax < 0))


def _setup_numpy(faces, Nv, X, Y, inv_w, cull):
    """rule 3 for every face of one view: (usable [F] bool, the corners in local order, A > 0, swapped)"""
    idx = faces.astype(np.int64)
    inside = ((idx >= 0) & (idx < Nv)).all(1)
    idx = np.where(inside[:, None], idx, 0)                      # an index out of range is never followed
    x, y, iw = X[idx], Y[idx], inv_w[idx]                        # [F, 3]
    ok = inside & (iw > 0.0).all(1)
    A = _edge(x[:, 0], y[:, 0], x[:, 1], y[:, 1], x[:, 2], y[:, 2])
    ok &= A != 0
    swapped = A < 0
    if cull:
        ok &= ~swapped
    order = np.where(swapped[:, None], np.array([0, 2, 1]), np.array([0, 1, 2]))
    rows = np.arange(len(faces))[:, None]
    return ok, x[rows, order], y[rows, order], iw[rows, order], np.abs(A), swapped


def _edges_at(x, y, px, py):
    """E_0, E_1, E_2 of triangles (x, y [..., 3]) at the points (px, py), broadcast"""
    return (_edge(x[..., 1], y[..., 1], x[..., 2], y[..., 2], px, py), _edge(x[..., 2], y[..., 2], x[..., 0], y[..., 0], px, py),
            _edge(x[..., 0], y[..., 0], x[..., 1], y[..., 1], px, py))


def _q(e, iw):
    return (e[0].astype(np.float64) * iw[..., 0] + e[1].astype(np.float64) * iw[..., 1]) + e[2].astype(np.float64) * iw[..., 2]


def _render_mesh_numpy(verts, faces, colors, full_proj, H, W, near, cull, want_bary, support=None, tolerance=0.0):
    """Rules 1 - 7 of include/scorp_gs.h statement for statement, in int64 and float64 numpy, over ALL (face, pixel) pairs:
    the box a kernel walks only decides which centres it looks at, never a value.  Returns (depth, face, barycentric or
    None, colour or None, visible_views [F] int32)."""
    V, Nv, F = full_proj.shape[0], verts.shape[0], faces.shape[0]
    depth, face = np.zeros((V, H, W), np.float32), np.full((V, H, W), -1, np.int32)
    bary = np.zeros((V, 3, H, W), np.float32) if want_bary else None
    color = np.zeros((V, 3, H, W), np.float32) if colors is not None else None
    visible = np.zeros(F, np.int32)
    px, py = (SNAP * np.arange(W, dtype=np.int64))[None, None, :], (SNAP * np.arange(H, dtype=np.int64))[None, :, None]
    step = max(1, _CHUNK_PAIRS // (H * W))
    with np.errstate(all="ignore"):
        for v in range(V):
            X, Y, inv_w = _project_numpy(verts, full_proj[v], H, W, near)
            ok, x, y, iw, A, swapped = _setup_numpy(faces, Nv, X, Y, inv_w, cull)
            keys = np.full((H, W), _EMPTY, np.uint64)
            live = np.nonzero(ok)[0]
            for s in range(0, len(live), step):
                f = live[s:s + step]
                xf, yf, iwf = x[f][:, None, None, :], y[f][:, None, None, :], iw[f][:, None, None, :]
                e = _edges_at(xf, yf, px, py)                     # rule 4
                tl = (_top_left(xf[..., 1], yf[..., 1], xf[..., 2], yf[..., 2]), _top_left(xf[..., 2], yf[..., 2], xf[..., 0], yf[..., 0]),
                      _top_left(xf[..., 0], yf[..., 0], xf[..., 1], yf[..., 1]))
                own = np.ones(e[0].shape, bool)
                for ek, tk in zip(e, tl):
                    own &= (ek > 0) | ((ek == 0) & tk)
                d = (A[f][:, None, None].astype(np.float64) / _q(e, iwf)).astype(np.float32)   # rule 5
                key = (d.view(np.uint32).astype(np.uint64) << np.uint64(32)) | f.astype(np.uint64)[:, None, None]
                keys = np.minimum(keys, np.where(own, key, _EMPTY).min(0))
            hit = keys != _EMPTY                                  # rule 6
            jj, ii = np.nonzero(hit)
            fw = (keys[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)
            dw = (keys[hit] >> np.uint64(32)).astype(np.uint32).view(np.float32)
            depth[v][hit], face[v][hit] = dw, fw.astype(np.int32)
            if (want_bary or color is not None) and len(fw):
                e = _edges_at(x[fw], y[fw], SNAP * ii.astype(np.int64), SNAP * jj.astype(np.int64))
                q = _q(e, iw[fw])
                l = [(e[k].astype(np.float64) * iw[fw][:, k]) / q for k in range(3)]
                b = [l[0], np.where(swapped[fw], l[2], l[1]), np.where(swapped[fw], l[1], l[2])]
                if want_bary:
                    for k in range(3):
                        bary[v, k][hit] = b[k].astype(np.float32)
                if color is not None:
                    c = colors.astype(np.float64)[faces[fw].astype(np.int64)]      # [n, 3 corners, 3 channels]
                    for ch in range(3):
                        color[v, ch][hit] = ((b[0] * c[:, 0, ch] + b[1] * c[:, 1, ch]) + b[2] * c[:, 2, ch]).astype(np.float32)
            counts = np.ones(len(fw), bool)                       # rule 7
            if support is not None:
                sd = support[v][hit]
                counts = (sd > np.float32(0.0)) & (np.abs(dw - sd) <= np.float32(tolerance))
            flags = np.zeros(F, np.int32)
            flags[fw[counts]] = 1
            visible += flags
    return depth, face, bary, color, visible


# ---- the public functions ----

def _views(full_proj, height, width, dev):
    """(full_proj [V, 16] float32 contiguous on dev, H, W) from a tensor [V, 4, 4] / [V, 16] or a list of cameras"""
    if isinstance(full_proj, (list, tuple)) and full_proj and hasattr(full_proj[0], "full_proj_transform"):
        sizes = {tuple(cam.resolution) for cam in full_proj}
        if len(sizes) != 1:
            raise ValueError(f"the cameras have different resolutions: {sorted(sizes)}")
        w, h = next(iter(sizes))
        height, width = (h if height is None else height), (w if width is None else width)
        full_proj = torch.stack([cam.full_proj_transform.to(dev) for cam in full_proj])
    if not isinstance(full_proj, torch.Tensor):
        full_proj = torch.as_tensor(np.asarray(full_proj))
    if full_proj.dim() < 2 or full_proj.shape[0] < 1 or full_proj[0].numel() != 16:
        raise ValueError(f"full_proj must be [V, 4, 4] or [V, 16] with V >= 1; got {tuple(full_proj.shape)}")
    if height is None or width is None:
        raise ValueError("height and width are needed unless full_proj is a list of cameras")
    H, W = int(height), int(width)
    if not (1 <= H <= MAX_RENDER_SIDE and 1 <= W <= MAX_RENDER_SIDE):
        raise ValueError(f"height and width must be in [1, {MAX_RENDER_SIDE}]; got {height} x {width}")
    return full_proj.reshape(full_proj.shape[0], 16).to(device=dev, dtype=torch.float32).contiguous(), H, W


def _render(mesh, full_proj, height, width, near, cull_backfaces, want_color, want_bary, want_visible, support_depth=None,
            support_tolerance=None, header=None):
    """The driver of the public functions: (depth, face, colour or None, barycentric or None, visible_views or None)."""
    near = float(near)
    if not (near > 0.0 and np.isfinite(near)):
        raise ValueError(f"near must be positive and finite; got {near}")
    checked = check_mesh(mesh)
    dev = mesh.vertices.device
    fp, H, W = _views(full_proj, height, width, dev)
    V, F = fp.shape[0], mesh.faces.shape[0]
    tol = 0.0
    if support_depth is not None:
        if support_tolerance is None or not float(support_tolerance) >= 0.0:
            raise ValueError(f"support_depth needs a support_tolerance that is not negative or NaN; got {support_tolerance}")
        tol = float(support_tolerance)
        if tuple(support_depth.shape) != (V, H, W):
            raise ValueError(f"support_depth must be [{V}, {H}, {W}]; got {tuple(support_depth.shape)}")
        support_depth = support_depth.to(device=dev, dtype=torch.float32).contiguous()
    depth = torch.zeros(V, H, W, dtype=torch.float32, device=dev)
    face = torch.full((V, H, W), -1, dtype=torch.int32, device=dev)
    color = torch.zeros(V, 3, H, W, dtype=torch.float32, device=dev) if want_color else None
    bary = torch.zeros(V, 3, H, W, dtype=torch.float32, device=dev) if want_bary else None
    visible = torch.zeros(F, dtype=torch.int32, device=dev) if want_visible else None
    if checked is None:   # no vertices or no faces: empty maps
        return depth, face, color, bary, visible
    verts, faces, colors, _ = checked
    flags = _C.MESH_RENDER_CULL_BACKFACES if cull_backfaces else 0
    if dev.type != "cuda":
        d, f, b, c, vis = _render_mesh_numpy(verts.numpy(), faces.numpy(), colors.numpy() if want_color else None, fp.numpy(), H, W, near,
                                             bool(cull_backfaces), want_bary, None if support_depth is None else support_depth.numpy(), tol)
        return (torch.from_numpy(d), torch.from_numpy(f), None if c is None else torch.from_numpy(c),
                None if b is None else torch.from_numpy(b), torch.from_numpy(vis) if want_visible else None)
    Nv = verts.shape[0]
    with torch.cuda.device(dev):
        per_view = _C.lib().scorp_mesh_render_workspace_bytes(Nv, F, 1, H, W)
        chunk = int(min(max(1, WORKSPACE_CAP // max(1, per_view)), MAX_RENDER_VIEWS, V))
        size = _C.lib().scorp_mesh_render_workspace_bytes(Nv, F, chunk, H, W)
        workspace = torch.empty(size, dtype=torch.uint8, device=dev)
        for s in range(0, V, chunk):
            n = min(chunk, V - s)
            _C.call("scorp_mesh_render", verts, Nv, faces, F, colors if want_color else None, fp[s:s + n], n, H, W, near, flags,
                    None if support_depth is None else support_depth[s:s + n], tol, depth[s:s + n], face[s:s + n],
                    None if bary is None else bary[s:s + n], None if color is None else color[s:s + n], visible, workspace, size)
            if header is not None:   # the workspace opens with the length of each view's large list
                header.append(workspace[:4 * n].view(torch.int32).clone())
    return depth, face, color, bary, visible


def render_mesh(mesh, full_proj, height=None, width=None, near=0.01, cull_backfaces=False, colors=True, barycentric=False, header=None):
    """The mesh as every camera sees it: a MeshRender of depth [V, H, W] (view-space depth of the nearest face at each pixel
    centre, 0 where there is none), face [V, H, W] int32 (-1 where there is none), color [V, 3, H, W] (the vertex colours,
    perspective-correct; None with colors=False) and, with barycentric=True, the weights [V, 3, H, W] of the face's three
    corners.  `full_proj` is [V, 4, 4] or [V, 16] (each camera's full_proj_transform as stored) or a list of cameras, whose
    full_proj_transform is taken and whose common `resolution` gives height and width when those are None; cameras of
    different resolutions raise.  Pixel (i, j) has its centre at (i, j) as in the splat rasterizers, so the depth lines up
    with a render's `render_depth` pixel for pixel.  The rules (include/scorp_gs.h): positions are snapped to 1/256 pixel and
    coverage is decided exactly, by the top-left rule, so faces that share an edge own each centre on it once; of two faces
    with the same fp32 depth the lower index wins; there is NO clipping against the near plane - a triangle with a vertex at
    w <= near is dropped whole for that view; cull_backfaces drops the faces whose corners run clockwise in the image (x
    right, y down), those whose right-hand normal points away from the camera.  The maps are a function of the inputs
    alone: the same bits from two calls, from any split of the views, and for the faces in any order (up to the face
    numbers, and to which of two coplanar duplicates is named).  An empty mesh renders empty maps.  `header`, a list,
    receives on a CUDA device one int32 tensor per chunk of views: how many triangles of each view were walked by a
    workgroup instead of a thread (a box of more than 64 pixel centres), a figure for measurements.
    CUDA tensors run csrc/mesh_render.hip on the current stream, the views in chunks whose workspace stays under
    WORKSPACE_CAP; CPU tensors run the same statements in numpy over ALL (face, pixel) pairs, meant for small inputs."""
    depth, face, color, bary, _ = _render(mesh, full_proj, height, width, near, cull_backfaces, bool(colors), bool(barycentric), False,
                                          header=header)
    return MeshRender(depth, face, color, bary)


def face_visibility(mesh, full_proj, height=None, width=None, near=0.01, cull_backfaces=False, support_depth=None,
                    support_tolerance=None):
    """int32 [F]: in how many of the views each face owns at least one pixel of render_mesh's face map.  With support_depth
    [V, H, W] (say the depth maps the mesh was fused from) a pixel counts only where support_depth > 0 and the mesh's depth
    is within support_tolerance of it."""
    return _render(mesh, full_proj, height, width, near, cull_backfaces, False, False, True, support_depth, support_tolerance)[4]


def cull_unseen_faces(mesh, full_proj, height=None, width=None, near=0.01, cull_backfaces=False, support_depth=None,
                      support_tolerance=None, min_views=1):
    """A new Mesh of the faces that face_visibility counts in at least `min_views` views, without the vertices nothing
    references any more: view-based culling of the back shells and interior sheets a TSDF leaves behind."""
    if int(min_views) < 1:
        raise ValueError(f"min_views must be at least 1; got {min_views}")
    seen = face_visibility(mesh, full_proj, height, width, near, cull_backfaces, support_depth, support_tolerance)
    dev = mesh.vertices.device
    faces = mesh.faces.to(dev)[seen >= int(min_views)]
    return Mesh(*drop_unreferenced(mesh.vertices, faces, mesh.colors.to(dev)))


def depth_difference(mesh_depth, reference_depth):
    """How a mesh's depth maps [V, H, W] (render_mesh(...).depth) differ from reference maps of the same shape (the surfel
    render's depthmaps): a DepthDifference over the pixels where both are > 0.  Plain torch; nothing leaves the device but
    the four overall figures."""
    if mesh_depth.shape != reference_depth.shape or mesh_depth.dim() != 3:
        raise ValueError(f"two depth stacks [V, H, W] of one shape are needed; got {tuple(mesh_depth.shape)} and {tuple(reference_depth.shape)}")
    m, r = mesh_depth.to(torch.float64), reference_depth.to(device=mesh_depth.device, dtype=torch.float64)
    has_m, has_r = m > 0, r > 0
    both = has_m & has_r
    diff = torch.where(both, (m - r).abs(), torch.zeros((), dtype=torch.float64, device=m.device))
    n_both, n_m, n_r = (t.sum((1, 2)).to(torch.float64) for t in (both, has_m, has_r))
    sums, maxima = diff.sum((1, 2)), diff.amax((1, 2))
    total = torch.stack([sums.sum(), maxima.max(), n_both.sum(), n_m.sum(), n_r.sum()]).cpu().tolist()
    share = lambda a, b: a / b if b > 0 else float("nan")
    overall = dict(mean_abs=share(total[0], total[2]), max_abs=total[1], reference_covered=share(total[2], total[4]),
                   mesh_covered=share(total[2], total[3]))
    return DepthDifference(sums / n_both, maxima, n_both / n_r, n_both / n_m, overall)
