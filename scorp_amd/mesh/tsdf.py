"""Dense TSDF fusion: every sample, or every point of a lattice, over all views in one launch (csrc/tsdf.hip), and the torch
form of the same statements for CPU tensors."""
import numpy as np
import torch

from .. import _C

MAX_RANGE = 32.0            # mcube_utils.py:26,93: the un-contracted vertices are clipped to +-max_range
LAUNCH_SAMPLES = 1 << 30    # samples per scorp_tsdf_fuse call (the C ABI takes up to (2^31 - 1) * 256)


def uncontract(y):
    """Contracted space back to the normalised one: a point of norm n >= 1 goes to norm 1 / (2 - n) on its ray, the unit
    ball stays (the inverse of the contraction n -> 2 - 1 / n that the reference's unbounded route works in)."""
    n = torch.linalg.vector_norm(y, dim=-1, keepdim=True)
    return y * torch.where(n < 1, torch.ones_like(n), 1 / ((2 - n) * n))


def _maps(depth, rgb, full_proj):
    if not isinstance(depth, torch.Tensor) or not isinstance(full_proj, torch.Tensor):
        raise ValueError("depth and full_proj must be torch tensors")
    if depth.dim() == 4 and depth.shape[1] == 1:
        depth = depth[:, 0]
    if depth.dim() != 3:
        raise ValueError(f"depth must be [V, H, W] or [V, 1, H, W]; got {tuple(depth.shape)}")
    V, H, W = depth.shape
    if V < 1:
        raise ValueError("no views")
    if H < 2 or W < 2:
        raise ValueError(f"the maps must be at least 2 x 2; got {H} x {W}")
    dev = depth.device
    depth = depth.to(torch.float32).contiguous()
    if rgb is not None:
        if tuple(rgb.shape) != (V, 3, H, W):
            raise ValueError(f"rgb must be [{V}, 3, {H}, {W}] like depth; got {tuple(rgb.shape)}")
        rgb = rgb.to(device=dev, dtype=torch.float32).contiguous()
    if tuple(full_proj.shape) not in ((V, 4, 4), (V, 16)):
        raise ValueError(f"full_proj must be [{V}, 4, 4] or [{V}, 16]; got {tuple(full_proj.shape)}")
    return depth, rgb, full_proj.to(device=dev, dtype=torch.float32).reshape(V, 16).contiguous()


def _bilinear(img, fx, fy, x0, y0):
    """img [C, H, W] at (fx, fy) with (x0, y0) = floor: grid_sample's four corners in its order; a corner past the last
    row / column has weight 0 and is not read."""
    H, W = img.shape[-2:]
    x1, y1 = x0 + 1, y0 + 1
    ex, ey, dx, dy = (x0 + 1).to(fx.dtype) - fx, (y0 + 1).to(fx.dtype) - fy, fx - x0.to(fx.dtype), fy - y0.to(fx.dtype)
    zero = torch.zeros((), dtype=img.dtype)

    def at(x, y):
        ok = (x < W) & (y < H)
        return torch.where(ok, img[:, y.clamp(max=H - 1), x.clamp(max=W - 1)], zero)
    return at(x0, y0) * (ex * ey) + at(x1, y0) * (dx * ey) + at(x0, y1) * (ex * dy) + at(x1, y1) * (dx * dy)


def _tsdf_fuse_torch(depth, rgb, full_proj, pts, voxel_size, contracted, center, radius):
    """scorp_tsdf_fuse's statements on CPU tensors (include/scorp_gs.h), every view over all samples at once."""
    V, H, W = depth.shape
    trunc = torch.full((pts.shape[0],), float(np.float32(5.0 * voxel_size)), dtype=torch.float32)
    if contracted:
        n = torch.sqrt((pts * pts).sum(-1))
        trunc = torch.where(n > 1, trunc * (1.0 / (2.0 - n.clamp(max=1.9))), trunc)
        k = (1.0 / (2.0 - n))[:, None]
        pts = torch.where((n < 1)[:, None], pts, k * (pts / n[:, None]))
        pts = pts * float(radius) + center
    tsdf = torch.ones(pts.shape[0])
    w = torch.ones(pts.shape[0])
    col = torch.zeros(pts.shape[0], 3)
    M = full_proj.reshape(V, 4, 4)
    for v in range(V):
        m = M[v]
        p = [pts[:, 2] * m[2, j] + (pts[:, 1] * m[1, j] + pts[:, 0] * m[0, j]) + m[3, j] for j in (0, 1, 3)]
        zc = p[2]
        u, t = p[0] / zc, p[1] / zc
        inside = (u > -1) & (u < 1) & (t > -1) & (t < 1) & (zc > 0)
        idx = torch.nonzero(inside)[:, 0]
        if idx.numel() == 0:
            continue
        fx = ((u[idx] + 1) / 2 * (W - 1)).clamp(0, W - 1)
        fy = ((t[idx] + 1) / 2 * (H - 1)).clamp(0, H - 1)
        x0, y0 = fx.floor().long(), fy.floor().long()
        sdf = _bilinear(depth[v][None], fx, fy, x0, y0)[0] - zc[idx]
        hit = sdf > -trunc[idx]
        idx, s = idx[hit], (sdf[hit] / trunc[idx[hit]]).clamp(-1.0, 1.0)
        wp = w[idx] + 1
        tsdf[idx] = (tsdf[idx] * w[idx] + s) / wp
        if rgb is not None:
            c = _bilinear(rgb[v], fx[hit], fy[hit], x0[hit], y0[hit]).T
            col[idx] = (col[idx] * w[idx][:, None] + c) / wp[:, None]
        w[idx] = wp
    return tsdf, (col if rgb is not None else None)


def tsdf_fuse(depth, rgb, full_proj, samples, voxel_size, contracted=False, center=None, radius=None):
    """compute_unbounded_tsdf (mesh_utils.py:209-247) over the views depth [V, H, W] (or [V, 1, H, W]), rgb [V, 3, H, W]
    or None, full_proj [V, 4, 4] (each camera's full_proj_transform as stored).  `samples` is [M, 3], or a tuple (x, y, z)
    of 1-D coordinate tensors: the lattice of their product in C order, never materialised on the GPU path.  With
    `contracted` the samples lie in the contracted space of the sphere (center [3], radius).  Returns the TSDF - [M], or
    [X, Y, Z] for a lattice - and, when rgb is given, (tsdf, colours [..., 3])."""
    depth, rgb, full_proj = _maps(depth, rgb, full_proj)
    dev = depth.device
    voxel_size = float(voxel_size)
    if not voxel_size > 0.0:
        raise ValueError(f"voxel_size must be positive; got {voxel_size}")
    if contracted:
        if center is None or radius is None:
            raise ValueError("contracted samples need center and radius")
        if not float(radius) > 0.0:
            raise ValueError(f"radius must be positive; got {radius}")
        center = torch.as_tensor(center, dtype=torch.float32, device="cpu").reshape(3)
    lattice = isinstance(samples, (tuple, list))
    if lattice:
        if len(samples) != 3 or any(not isinstance(c, torch.Tensor) or c.dim() != 1 or c.numel() < 1 for c in samples):
            raise ValueError("a lattice is a tuple of three non-empty 1-D coordinate tensors")
        coords = [c.to(device=dev, dtype=torch.float32).contiguous() for c in samples]
        shape = tuple(c.numel() for c in coords)
        M = shape[0] * shape[1] * shape[2]
        if max(shape) >= 2 ** 31:
            raise ValueError("a lattice axis has more than 2^31 - 1 points")
    else:
        if not isinstance(samples, torch.Tensor) or samples.dim() != 2 or samples.shape[1] != 3:
            raise ValueError("samples must be [M, 3] or a tuple (x, y, z)")
        pts = samples.to(device=dev, dtype=torch.float32).contiguous()
        M, shape = pts.shape[0], (pts.shape[0],)
    if M < 1:
        raise ValueError("no samples")
    V, H, W = depth.shape
    if not dev.type == "cuda":
        if lattice:
            pts = torch.stack(torch.meshgrid(*coords, indexing="ij"), dim=-1).reshape(-1, 3)
        tsdf, col = _tsdf_fuse_torch(depth, rgb, full_proj, pts, voxel_size, contracted, center, radius)
    else:
        tsdf = torch.empty(M, dtype=torch.float32, device=dev)
        col = torch.empty(M, 3, dtype=torch.float32, device=dev) if rgb is not None else None
        views = _C.ScorpTsdfViews(depth=depth.data_ptr(), rgb=rgb.data_ptr() if rgb is not None else None,
                                  full_proj=full_proj.data_ptr(), num_views=V, width=W, height=H)
        params = _C.ScorpTsdfParams(voxel_size=voxel_size, contracted=1 if contracted else 0, radius=float(radius or 0.0))
        if contracted:
            params.center[:] = center.tolist()
        smp = _C.ScorpTsdfSamples()
        if lattice:
            smp.x, smp.y, smp.z = (c.data_ptr() for c in coords)
            smp.nx, smp.ny, smp.nz = shape
        else:
            smp.xyz = pts.data_ptr()
        with torch.cuda.device(dev):
            for first in range(0, M, LAUNCH_SAMPLES):
                smp.first, smp.count = first, min(LAUNCH_SAMPLES, M - first)
                _C.call("scorp_tsdf_fuse", views, smp, params, tsdf, col)
    tsdf = tsdf.reshape(shape)
    return (tsdf, col.reshape(*shape, 3)) if rgb is not None else tsdf
