"""The bounded route: a sparse TSDF volume of 16^3-voxel blocks (csrc/tsdf_blocks.hip) and its surface through the block
borders by surface nets (csrc/isosurface_blocks.hip) or marching cubes (csrc/marching_cubes_blocks.hip), each with a numpy form
for CPU tensors.  The rules are in include/scorp_gs.h."""
from dataclasses import dataclass

import numpy as np
import torch

from .. import _C, mc_table
from ._common import Mesh, _check_method, empty_mesh
from .surface import _mc_faces_numpy, _scan_counts

BLOCK_SIDE, BLOCK_VOXELS = 16, 4096
KEY_BIAS = 1 << 20          # block coordinates lie in [-2^20, 2^20)
MAX_TABLE_SLOTS = 1 << 32   # the C ABI's bound on the touch table


@dataclass
class BlockVolume:
    """A fused sparse volume.  keys [B] int64 ascending (the block keys; they are below 2^63), coords [B, 3] int32 (bx, by, bz),
    view_mask [B, ceil(V / 32)] int32 (the bits of uint32 words), tsdf / weight [B, 4096] float32, colour [B, 4096, 3] float32
    in [0, 255] or None, voxel_length."""
    keys: torch.Tensor
    coords: torch.Tensor
    view_mask: torch.Tensor
    tsdf: torch.Tensor
    weight: torch.Tensor
    colour: object
    voxel_length: float


def block_coords(keys):
    """[B] int64 keys -> [B, 3] int32 block coordinates."""
    return torch.stack([((keys >> s) & 0x1FFFFF) - KEY_BIAS for s in (42, 21, 0)], -1).to(torch.int32)


def _block_views(depth, rgb, world_to_cam, intrinsics):
    if not isinstance(depth, torch.Tensor) or not isinstance(world_to_cam, torch.Tensor):
        raise ValueError("depth and world_to_cam must be torch tensors")
    if depth.dim() == 4 and depth.shape[1] == 1:
        depth = depth[:, 0]
    if depth.dim() != 3:
        raise ValueError(f"depth must be [V, H, W] or [V, 1, H, W]; got {tuple(depth.shape)}")
    V, H, W = depth.shape
    if V < 1:
        raise ValueError("no views")
    if V > 65535:
        raise ValueError(f"more than 65535 views: {V}")
    if H < 1 or W < 1:
        raise ValueError(f"empty maps: {H} x {W}")
    dev = depth.device
    depth = depth.to(torch.float32).contiguous()
    if rgb is not None:
        if tuple(rgb.shape) != (V, H, W, 3) or rgb.dtype != torch.uint8:
            raise ValueError(f"rgb must be uint8 [{V}, {H}, {W}, 3]; got {rgb.dtype} {tuple(rgb.shape)}")
        rgb = rgb.to(dev).contiguous()
    if tuple(world_to_cam.shape) not in ((V, 3, 4), (V, 4, 4)):
        raise ValueError(f"world_to_cam must be [{V}, 3, 4] or [{V}, 4, 4]; got {tuple(world_to_cam.shape)}")
    intrinsics = torch.as_tensor(intrinsics, dtype=torch.float32)   # (a device tensor stays where it is)
    if tuple(intrinsics.shape) == (4,):
        intrinsics = intrinsics[None].expand(V, 4)
    if tuple(intrinsics.shape) != (V, 4):
        raise ValueError(f"intrinsics must be (fx, fy, cx, cy) as [4] or [{V}, 4]; got {tuple(intrinsics.shape)}")
    cam = torch.cat([world_to_cam[:, :3].to(device=dev, dtype=torch.float32).reshape(V, 12), intrinsics.to(dev)], 1).contiguous()
    return depth, rgb, cam


def _check_lengths(voxel_length, sdf_trunc, stride):
    voxel_length, sdf_trunc, stride = float(np.float32(voxel_length)), float(np.float32(sdf_trunc)), int(stride)
    if not voxel_length > 0.0:
        raise ValueError(f"voxel_length must be positive; got {voxel_length}")
    if not sdf_trunc > 0.0 or not np.float32(sdf_trunc) <= np.float32(16) * np.float32(voxel_length):
        raise ValueError(f"sdf_trunc must be in (0, 16 voxel_length]; got {sdf_trunc} with voxel_length {voxel_length}")
    if stride < 1:
        raise ValueError(f"stride must be at least 1; got {stride}")
    return voxel_length, sdf_trunc, stride


def _block_coords_numpy(keys):
    """block_coords on a numpy array of keys, in int64."""
    return np.stack([((keys >> s) & 0x1FFFFF) - KEY_BIAS for s in (42, 21, 0)], -1)


def _pack_keys_numpy(b):
    b = b.astype(np.int64) + KEY_BIAS
    return b[..., 0] << 42 | b[..., 1] << 21 | b[..., 2]


def _blocks_touch_numpy(depth, cam, voxel_length, sdf_trunc, stride):
    """The touch rule in vectorised numpy float32: (keys [B] int64 ascending, view_mask [B, words] uint32)."""
    f = np.float32
    V, H, W = depth.shape
    words = (V + 31) // 32
    block_len, trunc = f(16) * f(voxel_length), f(sdf_trunc)
    uu, vv = np.meshgrid(np.arange(0, W, stride), np.arange(0, H, stride))
    per_view = []
    with np.errstate(all="ignore"):
        for i in range(V):
            C = cam[i]
            d = depth[i][::stride, ::stride]
            ok = d > 0
            d, u, v = d[ok], uu[ok].astype(f), vv[ok].astype(f)
            q = ((u - C[14]) * d / C[12] - C[3], (v - C[15]) * d / C[13] - C[7], d - C[11])
            pw = np.stack([(C[k] * q[0] + C[4 + k] * q[1]) + C[8 + k] * q[2] for k in range(3)], -1)
            lo, hi = np.floor((pw - trunc) / block_len), np.floor((pw + trunc) / block_len)
            if not bool(((lo >= -KEY_BIAS) & (hi < KEY_BIAS)).all()):
                raise ValueError("a depth point lies outside the volume's range of 2^20 blocks per axis (or is not finite)")
            lo, hi = lo.astype(np.int64), hi.astype(np.int64)
            keys = [np.empty(0, np.int64)]
            for o in np.ndindex(3, 3, 3):
                b = lo + np.asarray(o)
                keys.append(_pack_keys_numpy(b[(b <= hi).all(-1)]))
            per_view.append(np.unique(np.concatenate(keys)))
    keys = np.unique(np.concatenate(per_view))
    mask = np.zeros((keys.size, words), np.uint32)
    for i, k in enumerate(per_view):
        mask[np.searchsorted(keys, k), i >> 5] |= np.uint32(1 << (i & 31))
    return keys, mask


def _blocks_integrate_numpy(depth, rgb, cam, keys, mask, voxel_length, sdf_trunc):
    """The integrate rule in vectorised numpy float32, one view at a time over the blocks that carry its bit."""
    f = np.float32
    V, H, W = depth.shape
    B = keys.size
    vl, trunc = f(voxel_length), f(sdf_trunc)
    coords = _block_coords_numpy(keys)
    local = np.stack(np.unravel_index(np.arange(BLOCK_VOXELS), (16, 16, 16)), -1)
    tsdf, w = np.zeros(B * BLOCK_VOXELS, f), np.zeros(B * BLOCK_VOXELS, f)
    col = np.zeros((B * BLOCK_VOXELS, 3), f) if rgb is not None else None
    u_max, v_max = f(W) - f(1e-4), f(H) - f(1e-4)
    with np.errstate(all="ignore"):
        for i in range(V):
            blocks = np.flatnonzero((mask[:, i >> 5] >> np.uint32(i & 31)) & np.uint32(1))
            if blocks.size == 0:
                continue
            C = cam[i]
            g = coords[blocks][:, None, :] * 16 + local[None]
            c = vl * (g.astype(f) + f(0.5))
            x, y, z = c[..., 0].ravel(), c[..., 1].ravel(), c[..., 2].ravel()
            at = (blocks[:, None] * BLOCK_VOXELS + np.arange(BLOCK_VOXELS)[None]).ravel()
            px, py, pz = (((C[4 * r] * x + C[4 * r + 1] * y) + C[4 * r + 2] * z) + C[4 * r + 3] for r in range(3))
            uf, vf = (px * C[12] / pz + C[14]) + f(0.5), (py * C[13] / pz + C[15]) + f(0.5)
            ok = (pz > 0) & (uf >= f(1e-4)) & (uf < u_max) & (vf >= f(1e-4)) & (vf < v_max)
            at, pz, u, v = at[ok], pz[ok], uf[ok].astype(np.int64), vf[ok].astype(np.int64)
            d = depth[i][v, u]
            rx, ry = (u.astype(f) - C[14]) / C[12], (v.astype(f) - C[15]) / C[13]
            sdf = (d - pz) * np.sqrt((rx * rx + ry * ry) + f(1))
            hit = (d > 0) & (sdf > -trunc)
            at, s, u, v = at[hit], np.minimum(f(1), sdf[hit] / trunc), u[hit], v[hit]
            wo = w[at]
            wp = wo + f(1)
            tsdf[at] = (tsdf[at] * wo + s) / wp
            if col is not None:
                col[at] = (col[at] * wo[:, None] + rgb[i][v, u].astype(f)) / wp[:, None]
            w[at] = wp
    return (tsdf.reshape(B, BLOCK_VOXELS), w.reshape(B, BLOCK_VOXELS), col.reshape(B, BLOCK_VOXELS, 3) if col is not None else None)


def _blocks_touch(views, depth, voxel_length, sdf_trunc, stride, num_slots):
    """One scorp_tsdf_blocks_touch call on a table of num_slots: (keys [B] int64 ascending, view_mask [B, words] int32,
    overflow word).  With an overflow bit set the blocks are incomplete."""
    dev = depth.device
    words = (views.num_views + 31) // 32
    keys = torch.empty(num_slots, dtype=torch.int64, device=dev)
    mask = torch.empty(num_slots, words, dtype=torch.int32, device=dev)
    overflow = torch.empty(1, dtype=torch.int32, device=dev)
    _C.call("scorp_tsdf_blocks_touch", views, voxel_length, sdf_trunc, stride, keys, mask, num_slots, overflow)
    taken = keys != -1   # the empty key is all ones
    keys, order = torch.sort(keys[taken])
    return keys, mask[taken][order].contiguous(), int(overflow)


def tsdf_blocks_fuse(depth, rgb, world_to_cam, intrinsics, voxel_length, sdf_trunc, stride=4, num_slots=None):
    """Fuse the views depth [V, H, W] (0 = no measurement), rgb uint8 [V, H, W, 3] or None, world_to_cam [V, 3, 4] (p_cam =
    R p_w + t; [V, 4, 4] is cut), intrinsics (fx, fy, cx, cy) as [4] or [V, 4] into a BlockVolume by the rules of
    include/scorp_gs.h: every `stride`-th pixel of a view touches the blocks within sdf_trunc of its point, then every voxel of a
    touched block runs over the views that touched it.  sdf_trunc <= 16 voxel_length.  `num_slots` (a power of two) is the
    first size of the touch table; a table that turns out too small is doubled and the call repeated."""
    depth, rgb, cam = _block_views(depth, rgb, world_to_cam, intrinsics)
    voxel_length, sdf_trunc, stride = _check_lengths(voxel_length, sdf_trunc, stride)
    dev = depth.device
    V, H, W = depth.shape
    words = (V + 31) // 32
    if dev.type != "cuda":
        d, c = depth.numpy(), cam.numpy()
        keys, mask = _blocks_touch_numpy(d, c, voxel_length, sdf_trunc, stride)
        tsdf, weight, col = _blocks_integrate_numpy(d, rgb.numpy() if rgb is not None else None, c, keys, mask, voxel_length, sdf_trunc)
        keys = torch.from_numpy(keys)
        return BlockVolume(keys, block_coords(keys), torch.from_numpy(mask.view(np.int32)), torch.from_numpy(tsdf), torch.from_numpy(weight),
                           torch.from_numpy(col) if col is not None else None, voxel_length)
    views = _C.ScorpTsdfBlockViews(depth=depth.data_ptr(), rgb=rgb.data_ptr() if rgb is not None else None, cam=cam.data_ptr(),
                                   num_views=V, width=W, height=H)
    if num_slots is None:   # a first guess: a block per 16 sampled pixels, at load 1/2
        pixels = V * -(-W // stride) * -(-H // stride)
        num_slots = 1 << max(10, (pixels // 8).bit_length())
    num_slots = int(num_slots)
    if num_slots < 1 or num_slots & (num_slots - 1):
        raise ValueError(f"num_slots must be a power of two; got {num_slots}")
    with torch.cuda.device(dev):
        while True:
            keys, mask, overflow = _blocks_touch(views, depth, voxel_length, sdf_trunc, stride, num_slots)
            if overflow & 2:
                raise ValueError("a depth point lies outside the volume's range of 2^20 blocks per axis (or is not finite)")
            if not overflow:
                break
            if num_slots >= MAX_TABLE_SLOTS:
                raise ValueError("the touch table overflows at 2^32 slots")
            num_slots *= 2
        B = keys.numel()
        tsdf = torch.empty(B, BLOCK_VOXELS, dtype=torch.float32, device=dev)
        weight = torch.empty(B, BLOCK_VOXELS, dtype=torch.float32, device=dev)
        col = torch.empty(B, BLOCK_VOXELS, 3, dtype=torch.float32, device=dev) if rgb is not None else None
        if B:
            _C.call("scorp_tsdf_blocks_integrate", views, voxel_length, sdf_trunc, keys, mask, B, tsdf, weight, col)
    return BlockVolume(keys, block_coords(keys), mask, tsdf, weight, col, voxel_length)


def block_neighbors(keys):
    """nbr [B, 27] int32 for the ascending keys [B] int64: entry (dx + 1) 9 + (dy + 1) 3 + (dz + 1) is the rank of block
    b + (dx, dy, dz), or -1."""
    B = keys.numel()
    if keys.device.type == "cuda":
        nbr = torch.empty(B, 27, dtype=torch.int32, device=keys.device)
        if B:
            with torch.cuda.device(keys.device):
                _C.call("scorp_tsdf_blocks_neighbors", keys, B, nbr)
        return nbr
    k = keys.numpy()
    coords = _block_coords_numpy(k)
    nbr = np.full((B, 27), -1, np.int32)
    for n, o in enumerate(np.ndindex(3, 3, 3)):
        c = coords + (np.asarray(o) - 1)
        ok = ((c >= -KEY_BIAS) & (c < KEY_BIAS)).all(-1)
        want = _pack_keys_numpy(np.where(ok[:, None], c, 0))
        pos = np.minimum(np.searchsorted(k, want), max(B - 1, 0))
        nbr[:, n] = np.where(ok & (k[pos] == want), pos, -1)
    return torch.from_numpy(nbr)


def _pad_blocks(a, nbr, lo, hi, fill):
    """a [B, 16, 16, 16, ...] -> [B, n, n, n, ...] over the local range lo .. hi - 1 per axis (lo in (-1, 0), hi in (16, 17)),
    the entries outside 0 .. 15 fetched from the neighbouring blocks, `fill` where there is none."""
    B, n = a.shape[0], hi - lo
    out = np.full((B, n, n, n) + a.shape[4:], fill, a.dtype)
    segs = [(1, slice(0, 16), slice(-lo, 16 - lo))]
    if lo < 0:
        segs.append((0, slice(15, 16), slice(0, 1)))
    if hi > 16:
        segs.append((2, slice(0, 1), slice(16 - lo, 17 - lo)))
    for ox, sx, dx in segs:
        for oy, sy, dy in segs:
            for oz, sz, dz in segs:
                r = nbr[:, ox * 9 + oy * 3 + oz]
                have = np.flatnonzero(r >= 0)
                out[have[:, None, None, None], np.arange(n)[dx][None, :, None, None], np.arange(n)[dy][None, None, :, None],
                    np.arange(n)[dz][None, None, None, :]] = a[r[have]][:, sx, sy, sz]
    return out


def _surface_blocks_numpy(keys, nbr, tsdf, weight, colour, voxel_length):
    """The surface rule of include/scorp_gs.h in vectorised numpy float32: (vertices, faces, colours or None)."""
    f = np.float32
    B = keys.size
    coords = _block_coords_numpy(keys)
    nbr = nbr.copy()
    nbr[:, 13] = np.arange(B)
    shape = (B, 16, 16, 16)
    T = _pad_blocks(tsdf.reshape(shape), nbr, -1, 17, f(0))
    valid = _pad_blocks(weight.reshape(shape), nbr, -1, 17, f(0)) > 0
    inside = T < 0
    Cc = _pad_blocks(colour.reshape(shape + (3,)), nbr, 0, 17, f(0)) if colour is not None else None

    def corner(a, n, base=1):   # the values at corner n of the block's own cells (a padded from local -1: base 1)
        di, dj, dk = base + (n >> 2), base + ((n >> 1) & 1), base + (n & 1)
        return a[:, di:di + 16, dj:dj + 16, dk:dk + 16]
    cell_valid = np.ones((B, 17, 17, 17), bool)   # cells -1 .. 15 at index 0 .. 16
    for n in range(8):
        di, dj, dk = n >> 2, (n >> 1) & 1, n & 1
        cell_valid &= valid[:, di:di + 17, dj:dj + 17, dk:dk + 17]
    s = [np.zeros(shape, f) for _ in range(3)]
    csum = np.zeros(shape + (3,), f) if Cc is not None else None
    cnt = np.zeros(shape, np.int32)
    with np.errstate(all="ignore"):
        for axis in range(3):
            step = 4 >> axis
            for n0 in range(8):
                if n0 & step:
                    continue
                v0, v1 = corner(T, n0), corner(T, n0 + step)
                cross = corner(inside, n0) != corner(inside, n0 + step)
                t = (f(0) - v0) / (v1 - v0)
                fixed = (f(n0 >> 2), f((n0 >> 1) & 1), f(n0 & 1))
                for d in range(3):
                    s[d] += np.where(cross, t if d == axis else fixed[d], f(0)).astype(f)
                if csum is not None:
                    c0, c1 = corner(Cc, n0, 0), corner(Cc, n0 + step, 0)
                    csum += np.where(cross[..., None], c0 + t[..., None] * (c1 - c0), f(0)).astype(f)
                cnt += cross
    active = (cnt > 0) & cell_valid[:, 1:, 1:, 1:]
    ids = (np.cumsum(active.ravel(), dtype=np.int64) - 1).reshape(shape)
    bi, ci, cj, ck = np.nonzero(active)
    n = cnt[active].astype(f)
    verts = np.empty((bi.size, 3), f)
    for d, l in enumerate((ci, cj, ck)):
        g = coords[bi, d] * 16 + l
        verts[:, d] = f(voxel_length) * ((g.astype(f) + f(0.5)) + s[d][active] / n)
    cols = (csum[active] / n[:, None] / f(255)).astype(f) if csum is not None else None
    ids = _pad_blocks(np.where(active, ids, -1), nbr, -1, 16, -1)   # cells -1 .. 15 at index 0 .. 16
    E = np.zeros(shape + (3,), bool)
    own = lambda a, off=(0, 0, 0): a[:, 1 + off[0]:17 + off[0], 1 + off[1]:17 + off[1], 1 + off[2]:17 + off[2]]
    eye = np.eye(3, dtype=np.int64)
    for a in range(3):
        b, c = eye[(a + 1) % 3], eye[(a + 2) % 3]
        ok = own(inside) != own(inside, eye[a])
        for off in (0 * b, -b, -b - c, -c):
            ok = ok & own(cell_valid, off)
        E[..., a] = ok
    qb, qi, qj, qk, qa = np.nonzero(E)
    q = np.stack([qi, qj, qk], 1) + 1   # into the arrays padded from -1
    b, c = eye[(qa + 1) % 3], eye[(qa + 2) % 3]
    cell = lambda p: ids[qb, p[:, 0], p[:, 1], p[:, 2]]
    c00, c10, c11, c01 = cell(q), cell(q - b), cell(q - b - c), cell(q - c)
    qin = inside[qb, q[:, 0], q[:, 1], q[:, 2]]
    faces = np.stack([c00, np.where(qin, c10, c11), np.where(qin, c11, c10),
                      c00, np.where(qin, c11, c01), np.where(qin, c01, c11)], 1).reshape(-1, 3).astype(np.int32)
    return verts, faces, cols


def _marching_cubes_blocks_numpy(keys, nbr, tsdf, weight, colour, voxel_length):
    """The marching-cubes surface rule of include/scorp_gs.h in vectorised numpy float32: (vertices, faces, colours or None)."""
    f = np.float32
    B = keys.size
    coords = _block_coords_numpy(keys)
    nbr = nbr.copy()
    nbr[:, 13] = np.arange(B)
    shape = (B, 16, 16, 16)
    T = _pad_blocks(tsdf.reshape(shape), nbr, -1, 17, f(0))          # local -1 .. 16 at index 0 .. 17
    valid = _pad_blocks(weight.reshape(shape), nbr, -1, 17, f(0)) > 0
    inside = (T < 0) & valid
    cell_valid = np.ones((B, 17, 17, 17), bool)                      # cells -1 .. 15 at index 0 .. 16
    for n in range(8):
        di, dj, dk = n >> 2, (n >> 1) & 1, n & 1
        cell_valid &= valid[:, di:di + 17, dj:dj + 17, dk:dk + 17]
    own = lambda a, off=(0, 0, 0): a[:, 1 + off[0]:17 + off[0], 1 + off[1]:17 + off[1], 1 + off[2]:17 + off[2]]
    eye = np.eye(3, dtype=np.int64)
    E = np.zeros(shape + (3,), bool)
    for a in range(3):
        b, c = eye[(a + 1) % 3], eye[(a + 2) % 3]
        some = np.zeros(shape, bool)
        for off in (0 * b, -b, -b - c, -c):
            some |= own(cell_valid, off)
        E[..., a] = (own(inside) != own(inside, eye[a])) & some
    vid = (np.cumsum(E.ravel(), dtype=np.int64) - 1).reshape(E.shape)   # ascending (block rank, local q, axis)
    qb, qi, qj, qk, qa = np.nonzero(E)
    q = np.stack([qi, qj, qk], 1)
    q1 = q + eye[qa]
    f0, f1 = T[qb, q[:, 0] + 1, q[:, 1] + 1, q[:, 2] + 1], T[qb, q1[:, 0] + 1, q1[:, 1] + 1, q1[:, 2] + 1]
    with np.errstate(all="ignore"):
        t = (f(0) - f0) / (f1 - f0)
    verts = np.empty((qb.size, 3), f)
    for d in range(3):
        g = (coords[qb, d] * 16 + q[:, d]).astype(f) + f(0.5)
        verts[:, d] = f(voxel_length) * np.where(qa == d, g + t, g)
    cols = None
    if colour is not None:
        Cc = _pad_blocks(colour.reshape(shape + (3,)), nbr, 0, 17, f(0))
        c0, c1 = Cc[qb, q[:, 0], q[:, 1], q[:, 2]], Cc[qb, q1[:, 0], q1[:, 1], q1[:, 2]]
        cols = ((c0 + t[:, None] * (c1 - c0)) / f(255)).astype(f)
    case = np.zeros(shape, np.int64)
    for n in range(8):
        case |= own(inside, (n >> 2, (n >> 1) & 1, n & 1)).astype(np.int64) << n
    vid = _pad_blocks(np.where(E, vid, -1), nbr, 0, 17, -1)          # local 0 .. 16: the edges of the cells' far corners
    return verts, _mc_faces_numpy(case, cell_valid[:, 1:, 1:, 1:], vid, mc_table.cached_table()), cols


def _marching_cubes_blocks_gpu(keys, nbr, tsdf, weight, colour, voxel_length):
    dev = tsdf.device
    B = keys.numel()
    with torch.cuda.device(dev):
        masks = torch.empty(B * BLOCK_VOXELS, dtype=torch.uint8, device=dev)
        counts = torch.empty(B * BLOCK_VOXELS, dtype=torch.uint8, device=dev)
        _C.call("scorp_marching_cubes_blocks_count_edges", tsdf, weight, nbr, B, masks, counts)
        nv, edge_scan = _scan_counts(counts, 2 ** 31, "vertices")
        if nv == 0:
            return empty_mesh(dev)
        verts = torch.empty(nv, 3, dtype=torch.float32, device=dev)
        cols = torch.empty(nv, 3, dtype=torch.float32, device=dev) if colour is not None else None
        _C.call("scorp_marching_cubes_blocks_emit_vertices", tsdf, weight, colour, keys, nbr, B, voxel_length, masks, edge_scan, nv,
                verts, cols)
        if cols is None:
            cols = torch.zeros(nv, 3, dtype=torch.float32, device=dev)
        _C.call("scorp_marching_cubes_blocks_count_faces", tsdf, weight, nbr, B, counts)
        nf, face_scan = _scan_counts(counts, 2 ** 31, "triangles")
        faces = torch.empty(nf, 3, dtype=torch.int32, device=dev)
        if nf:
            _C.call("scorp_marching_cubes_blocks_emit_faces", tsdf, weight, nbr, B, masks, edge_scan, face_scan, nf, faces)
    return Mesh(verts, faces, cols)


def _surface_nets_blocks_gpu(keys, nbr, tsdf, weight, colour, voxel_length):
    dev = tsdf.device
    B = keys.numel()
    with torch.cuda.device(dev):
        flags = torch.empty(B * BLOCK_VOXELS, dtype=torch.uint8, device=dev)
        _C.call("scorp_isosurface_blocks_count_cells", tsdf, weight, nbr, B, flags)
        nv, cell_scan = _scan_counts(flags, 2 ** 31, "vertices")
        if nv == 0:
            return empty_mesh(dev)
        verts = torch.empty(nv, 3, dtype=torch.float32, device=dev)
        cols = torch.empty(nv, 3, dtype=torch.float32, device=dev) if colour is not None else None
        _C.call("scorp_isosurface_blocks_emit_vertices", tsdf, weight, colour, keys, nbr, B, voxel_length, cell_scan, nv, verts, cols)
        if cols is None:
            cols = torch.zeros(nv, 3, dtype=torch.float32, device=dev)
        counts = torch.empty(B * BLOCK_VOXELS, dtype=torch.uint8, device=dev)
        _C.call("scorp_isosurface_blocks_count_faces", tsdf, weight, nbr, B, counts)
        nq, edge_scan = _scan_counts(counts, 2 ** 30, "triangles")   # (two triangles per quad)
        faces = torch.empty(2 * nq, 3, dtype=torch.int32, device=dev)
        if nq:
            _C.call("scorp_isosurface_blocks_emit_faces", tsdf, weight, nbr, B, cell_scan, edge_scan, nq, faces)
    return Mesh(verts, faces, cols)


def extract_surface_blocks(volume, method="surface_nets"):
    """The zero surface of a BlockVolume through the block borders (include/scorp_gs.h): a Mesh on the volume's device, colours
    in [0, 1] (zeros for a volume without colour).  method "surface_nets": vertices in ascending (block, local cell index);
    cells with a corner no view has written, or in a block that does not exist, carry no vertex and no face.
    "marching_cubes": one vertex per crossed lattice edge that has a valid cell round it, in ascending (block, local index of
    the edge's first point, axis); only valid cells emit triangles."""
    _check_method(method)
    keys, tsdf, weight, colour = volume.keys, volume.tsdf, volume.weight, volume.colour
    dev = tsdf.device
    B = keys.numel()
    if B == 0:
        return empty_mesh(dev)
    if tuple(tsdf.shape) != (B, BLOCK_VOXELS) or tuple(weight.shape) != (B, BLOCK_VOXELS) or \
            (colour is not None and tuple(colour.shape) != (B, BLOCK_VOXELS, 3)):
        raise ValueError(f"tsdf and weight must be [{B}, 4096] and colour [{B}, 4096, 3]")
    keys = keys.to(torch.int64).contiguous()
    tsdf, weight = tsdf.to(torch.float32).contiguous(), weight.to(torch.float32).contiguous()
    colour = colour.to(torch.float32).contiguous() if colour is not None else None
    voxel_length = float(np.float32(volume.voxel_length))
    nbr = block_neighbors(keys)
    if dev.type != "cuda":
        form = _marching_cubes_blocks_numpy if method == "marching_cubes" else _surface_blocks_numpy
        v, t, c = form(keys.numpy(), nbr.numpy(), tsdf.numpy(), weight.numpy(), colour.numpy() if colour is not None else None, voxel_length)
        return Mesh(torch.from_numpy(v), torch.from_numpy(t), torch.from_numpy(c) if c is not None else torch.zeros(v.shape[0], 3))
    form = _marching_cubes_blocks_gpu if method == "marching_cubes" else _surface_nets_blocks_gpu
    return form(keys, nbr, tsdf, weight, colour, voxel_length)
