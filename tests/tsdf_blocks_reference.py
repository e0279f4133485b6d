"""Yardstick of the bounded TSDF route (csrc/tsdf_blocks.hip, csrc/isosurface_blocks.hip, scorp_amd.mesh.tsdf_blocks_fuse /
extract_surface_blocks): the rules of include/scorp_gs.h restated in plain numpy with a dtype argument (float64 is the
reference, float32 measures what the statements' own rounding costs), written independently of scorp_amd/mesh/blocks.py - touch
as loops over the pixels into a dictionary, integration block by block, the surface as surface nets over the dense box
gathered from a dictionary of blocks - plus the analytic scene the tests fuse and the rule that leaves out the voxels
whose decisions are too close to call."""
import functools

import numpy as np

W, H = 48, 40
FX = FY = 44.0
CX, CY = 23.5, 19.5
VOXEL, TRUNC, STRIDE = 0.05, 0.2, 4
PLANE_Z = -0.6
DEPTH_MAX = 6.0        # the range of the analytic depth (twice the cameras' distance): a ray that hits nothing nearer measures nothing
MARGIN = 1e-5          # a decision closer than this to its threshold (float64) is too close to call
VIEWS = ((0.0, 0.5), (1.3, 1.0), (2.6, -0.4), (3.9, 1.5), (5.2, 0.2))   # azimuth, height; distance 3 from the origin
BIAS = 1 << 20


def key_of(b):
    return (int(b[0]) + BIAS) << 42 | (int(b[1]) + BIAS) << 21 | (int(b[2]) + BIAS)


def coords_of(key):
    return ((key >> 42) & 0x1FFFFF) - BIAS, ((key >> 21) & 0x1FFFFF) - BIAS, (key & 0x1FFFFF) - BIAS


# ---- the scene: a unit sphere at the origin over the plane z = -0.6 ----

def camera(azimuth, height, distance=3.0, shift=(0.0, 0.0, 0.0)):
    """E [3, 4] float64 of a camera at `distance` from the origin (+ shift), at the given height, looking at the origin
    (+ shift): +x right, +y down, +z forward."""
    r = np.sqrt(distance ** 2 - height ** 2)
    pos = np.array([r * np.cos(azimuth), r * np.sin(azimuth), height])
    fwd = -pos / np.linalg.norm(pos)
    right = np.cross(fwd, (0.0, 0.0, 1.0))
    right /= np.linalg.norm(right)
    R = np.stack([right, np.cross(fwd, right), fwd])
    pos = pos + np.asarray(shift, np.float64)
    return np.concatenate([R, (-R @ pos)[:, None]], 1)


def analytic_depth(E, shift=(0.0, 0.0, 0.0)):
    """Camera-space z of every pixel's ray through (u, v) at the unit sphere or the plane (both moved by shift); 0 where the
    ray hits neither within DEPTH_MAX.  (Without a range the rays near the horizon meet the plane a thousand units away,
    where one ulp of a float32 coordinate is 6e-5: no float32 statement can hold a margin of 1e-5 there.)"""
    R, t = E[:, :3], E[:, 3]
    o = -R.T @ t - np.asarray(shift, np.float64)
    u, v = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    d = np.stack([(u - CX) / FX, (v - CY) / FY, np.ones_like(u)], -1) @ R     # rows of R^T applied: world directions
    depth = np.full((H, W), np.inf)
    a, b, c = (d * d).sum(-1), (d * o).sum(-1), (o * o).sum() - 1.0
    disc = b * b - a * c
    with np.errstate(invalid="ignore", divide="ignore"):
        s = (-b - np.sqrt(disc)) / a
        ok = (disc >= 0) & (s > 1e-6)
        depth[ok] = s[ok]
        s = (PLANE_Z - o[2]) / d[..., 2]
        ok = np.isfinite(s) & (s > 1e-6) & (s < depth)
        depth[ok] = s[ok]
    depth[~(depth <= DEPTH_MAX)] = 0.0
    return depth.astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene(num_views=5, shift=(0.0, 0.0, 0.0)):
    """(depth [V, H, W] float32, rgb [V, H, W, 3] uint8 seeded noise, cam [V, 16] float32: E row-major, fx, fy, cx, cy).  More
    than five views repeat the five."""
    E = [camera(*VIEWS[i % 5], shift=shift) for i in range(num_views)]
    depth = np.stack([analytic_depth(e, shift) for e in E])
    rgb = np.random.default_rng(7).integers(0, 256, (5, H, W, 3), dtype=np.uint8)[np.arange(num_views) % 5]
    cam = np.stack([np.concatenate([e.reshape(-1), [FX, FY, CX, CY]]) for e in E]).astype(np.float32)
    return depth, np.ascontiguousarray(rgb), cam


# ---- the rules ----

def touch(depth, cam, voxel_length, sdf_trunc, stride, dtype=np.float64, grow=0.0):
    """{block key: set of views}: a loop over the sampled pixels of every view.  `grow` widens (or, negative, narrows) every
    pixel's box by grow * max(1, d) per side: with +-MARGIN the two runs bracket every block whose existence is too close to
    call - a box face within MARGIN of a block face.  (The points of the plane z = -0.6 put the face p.z - 0.2 of their boxes
    ON the block face z = -0.8 = -16 voxel_length: whether the blocks below exist hangs on the last bits of p.z.  The float32
    error of p_w is a few 2^-24 d; MARGIN max(1, d) is some forty times that.)"""
    f = dtype
    block_len, trunc = f(16) * f(np.float32(voxel_length)), f(np.float32(sdf_trunc))
    blocks = {}
    V, Hh, Ww = depth.shape
    for i in range(V):
        C = cam[i].astype(f)
        R, t = C[:12].reshape(3, 4)[:, :3], C[:12].reshape(3, 4)[:, 3]
        fx, fy, cx, cy = C[12:]
        for v in range(0, Hh, stride):
            for u in range(0, Ww, stride):
                d = f(depth[i, v, u])
                if not d > 0:
                    continue
                q = (f(u) - cx) * d / fx - t[0], (f(v) - cy) * d / fy - t[1], d - t[2]
                pw = [(R[0, k] * q[0] + R[1, k] * q[1]) + R[2, k] * q[2] for k in range(3)]
                g = f(grow) * max(f(1), d)
                lo = [int(np.floor((p - trunc - g) / block_len)) for p in pw]
                hi = [int(np.floor((p + trunc + g) / block_len)) for p in pw]
                for bx in range(lo[0], hi[0] + 1):
                    for by in range(lo[1], hi[1] + 1):
                        for bz in range(lo[2], hi[2] + 1):
                            blocks.setdefault(key_of((bx, by, bz)), set()).add(i)
    return blocks


def masks_of(blocks, num_views, keys=None):
    """(keys [B] int64 ascending, view_mask [B, words] uint32) of a touch() dictionary (over the given keys, if any)."""
    keys = np.array(sorted(blocks), np.int64) if keys is None else keys
    mask = np.zeros((keys.size, (num_views + 31) // 32), np.uint32)
    for r, k in enumerate(keys):
        for i in blocks.get(int(k), ()):
            mask[r, i >> 5] |= np.uint32(1 << (i & 31))
    return keys, mask


LOCAL = np.stack(np.unravel_index(np.arange(4096), (16, 16, 16)), -1)   # (lx, ly, lz) of the linear index (lx 16 + ly) 16 + lz


def integrate(depth, rgb, cam, keys, mask, voxel_length, sdf_trunc, dtype=np.float64, undecided=None):
    """(tsdf [B, 4096], weight, colour [B, 4096, 3], near [B, 4096]) in `dtype`, block by block and view by view; near marks a
    voxel one of whose decisions, in a view that may write it, is too close to call (the leave-out rule of the tests): |z| <
    1e-5, u_f or v_f within 1e-4 of an integer (in front of the camera: behind it nothing is decided by them), |sdf +
    sdf_trunc| < 1e-5 - and a voxel written by a view whose bit in the block's mask is `undecided`."""
    f = dtype
    V, Hh, Ww = depth.shape
    B = keys.size
    vl, trunc = f(np.float32(voxel_length)), f(np.float32(sdf_trunc))
    tsdf, w, col = np.zeros((B, 4096), f), np.zeros((B, 4096), f), np.zeros((B, 4096, 3), f)
    near = np.zeros((B, 4096), bool)
    u_max, v_max = f(Ww) - f(np.float32(1e-4)), f(Hh) - f(np.float32(1e-4))
    with np.errstate(all="ignore"):
        for r in range(B):
            g = np.asarray(coords_of(int(keys[r])))[None] * 16 + LOCAL
            c = vl * (g.astype(f) + f(0.5))
            x, y, z = c[:, 0], c[:, 1], c[:, 2]
            for i in range(V):
                if not (int(mask[r, i >> 5]) >> (i & 31)) & 1:
                    continue
                C = cam[i].astype(f)
                px = ((C[0] * x + C[1] * y) + C[2] * z) + C[3]
                py = ((C[4] * x + C[5] * y) + C[6] * z) + C[7]
                pz = ((C[8] * x + C[9] * y) + C[10] * z) + C[11]
                fx, fy, cx, cy = C[12:]
                uf, vf = (px * fx / pz + cx) + f(0.5), (py * fy / pz + cy) + f(0.5)
                ok = (pz > 0) & (uf >= f(np.float32(1e-4))) & (uf < u_max) & (vf >= f(np.float32(1e-4))) & (vf < v_max)
                near[r] |= np.abs(pz) < 1e-5
                front = pz > 0
                near[r] |= front & ((np.abs(uf - np.rint(uf)) < 1e-4) | (np.abs(vf - np.rint(vf)) < 1e-4))
                at = np.flatnonzero(ok)
                u, v = uf[at].astype(np.int64), vf[at].astype(np.int64)
                d = depth[i][v, u].astype(f)
                rx, ry = (u.astype(f) - cx) / fx, (v.astype(f) - cy) / fy
                sdf = (d - pz[at]) * np.sqrt((rx * rx + ry * ry) + f(1))
                seen = d > 0
                near[r, at[seen]] |= np.abs(sdf[seen] + trunc) < 1e-5
                hit = seen & (sdf > -trunc)
                if undecided is not None and (int(undecided[r, i >> 5]) >> (i & 31)) & 1:
                    near[r, at[hit]] = True
                at, s, u, v = at[hit], np.minimum(f(1), sdf[hit] / trunc), u[hit], v[hit]
                wo = w[r, at]
                tsdf[r, at] = (tsdf[r, at] * wo + s) / (wo + f(1))
                col[r, at] = (col[r, at] * wo[:, None] + rgb[i][v, u].astype(f)) / (wo + f(1))[:, None]
                w[r, at] = wo + f(1)
    return tsdf, w, col, near


def fuse_case(depth, rgb, cam, voxel_length, sdf_trunc, stride):
    """The views fused in float64 and float32.  keys / mask: every block and view bit that MAY exist (boxes widened by
    MARGIN); sure: the bits that MUST (boxes narrowed); a bit in between is too close to call.  The volumes tsdf64 ... col32 are
    fused over keys / mask; keep leaves out the voxels too close to call; keys32 / mask32: the float32 touch."""
    num_views = depth.shape[0]
    keys, mask = masks_of(touch(depth, cam, voxel_length, sdf_trunc, stride, np.float64, MARGIN), num_views)
    _, sure = masks_of(touch(depth, cam, voxel_length, sdf_trunc, stride, np.float64, -MARGIN), num_views, keys)
    keys32, mask32 = masks_of(touch(depth, cam, voxel_length, sdf_trunc, stride, np.float32), num_views)
    t64, w64, c64, near = integrate(depth, rgb, cam, keys, mask, voxel_length, sdf_trunc, np.float64, mask & ~sure)
    t32, w32, c32, _ = integrate(depth, rgb, cam, keys, mask, voxel_length, sdf_trunc, np.float32)
    keep = ~near
    return dict(keys=keys, mask=mask, sure=sure, keys32=keys32, mask32=mask32, tsdf64=t64, w64=w64, col64=c64, tsdf32=t32, w32=w32,
                col32=c32, keep=keep, e_ref=float(np.abs(t32.astype(np.float64) - t64)[keep].max(initial=0.0)),
                e_ref_colour=float(np.abs(c32.astype(np.float64) - c64)[keep].max(initial=0.0)))


def inputs(num_views=5, shift=(0.0, 0.0, 0.0), blank_view=None):
    """scene() with, optionally, one view that sees nothing (all-zero depth)."""
    depth, rgb, cam = scene(num_views, shift)
    if blank_view is not None:
        depth = depth.copy()
        depth[blank_view] = 0.0
    return depth, rgb, cam


@functools.lru_cache(maxsize=None)
def case(num_views=5, shift=(0.0, 0.0, 0.0), blank_view=None):
    """fuse_case of the scene at VOXEL / TRUNC / STRIDE, evaluated once."""
    return fuse_case(*inputs(num_views, shift, blank_view), VOXEL, TRUNC, STRIDE)


def one_block_inputs():
    """One view whose every sampled pixel lands in block (0, 0, 0): a fronto-parallel plane at depth 8 seen from (8.5, 8.5, 0)
    along +z, voxel_length 1 (a block is 16 wide), sdf_trunc 0.5.  -> (depth, rgb, cam, voxel_length, sdf_trunc, stride)"""
    depth = np.full((1, H, W), 8.0, np.float32)
    rgb = np.random.default_rng(3).integers(0, 256, (1, H, W, 3), dtype=np.uint8)
    E = np.concatenate([np.eye(3), [[-8.5], [-8.5], [0.0]]], 1)
    cam = np.concatenate([E.reshape(-1), [FX, FY, CX, CY]]).astype(np.float32)[None]
    return depth, rgb, cam, 1.0, 0.5, STRIDE


def compare_volume(c, keys, mask, tsdf, weight, colour):
    """Holds a fused volume (numpy arrays) to the yardstick of case c: blocks and masks EQUAL to the float32 touch and, by
    match_blocks, to float64 in every bit float64 can call; weights EQUAL
    on the kept voxels, tsdf within 4 e_ref and colour within 4 e_ref_colour there (both carry the float32 statements' own
    rounding), and nothing written in a kept voxel of a block that was free not to exist.  Returns the two measured errors."""
    rows, absent = match_blocks(c, keys, mask)
    # float64 cannot call the bits inside the bracket; the float32 statements can, and the forms under test ARE those
    # statements (no contraction, correctly rounded division): their keys and masks are the float32 yardstick's, bit for bit
    assert np.array_equal(np.asarray(keys, np.int64), c["keys32"]), "block keys differ from the float32 yardstick's"
    assert np.array_equal(np.asarray(mask).view(np.uint32).reshape(len(c["keys32"]), -1), c["mask32"]), "view masks differ from the float32 yardstick's"
    keep = c["keep"][rows]
    assert np.array_equal(weight[keep].astype(np.float64), c["w64"][rows][keep])
    assert not c["w64"][absent][c["keep"][absent]].any()
    err = float(np.abs(tsdf.astype(np.float64) - c["tsdf64"][rows])[keep].max(initial=0.0))
    err_colour = float(np.abs(colour.astype(np.float64) - c["col64"][rows])[keep].max(initial=0.0)) if colour is not None else 0.0
    assert err <= 4 * c["e_ref"], (err, c["e_ref"])
    assert err_colour <= 4 * c["e_ref_colour"], (err_colour, c["e_ref_colour"])
    return err, err_colour


def match_blocks(c, keys, mask):
    """Holds a block set (keys [B] int64 ascending, mask [B, words] uint32) to the case's: EQUAL in every bit that is not too
    close to call - no block or view bit beyond those that may exist, none missing of those that must.  Returns the rows of
    c's arrays the blocks correspond to and the rows of c's blocks that are absent."""
    keys, mask = np.asarray(keys, np.int64), np.asarray(mask).view(np.uint32).reshape(len(keys), -1)
    assert np.array_equal(keys, np.unique(keys)), "block keys not strictly ascending"
    rows = np.searchsorted(c["keys"], keys)
    assert rows.max(initial=0) < c["keys"].size and np.array_equal(c["keys"][rows], keys), "a block that cannot exist"
    assert not (mask & ~c["mask"][rows]).any(), "a view bit that cannot be set"
    assert not (c["sure"][rows] & ~mask).any(), "a view bit that must be set is missing"
    absent = np.setdiff1d(np.arange(c["keys"].size), rows)
    assert not c["sure"][absent].any(), "a block that must exist is missing"
    return rows, absent


# ---- the surface: surface nets over the dense box gathered from a dictionary of blocks ----

CORNERS = [np.array([n >> 2, (n >> 1) & 1, n & 1]) for n in range(8)]


def surface_blocks(blocks, voxel_length, return_cells=False):
    """blocks: {(bx, by, bz): (tsdf [4096], weight [4096], colour [4096, 3] or None)} -> (vertices [Nv, 3] float64, faces
    [Nf, 3] int64, colours [Nv, 3] float64 in [0, 1]), in the order of include/scorp_gs.h.  Plain loops over the active cells
    and the crossed lattice edges of the blocks' bounding box; a voxel of a missing block has weight 0.  With return_cells also
    the global cell coordinates g [Nv, 3] of the vertices."""
    bs = sorted(blocks)
    rank = {b: r for r, b in enumerate(bs)}
    lo = np.min(np.array(bs), 0)
    dims = (np.max(np.array(bs), 0) - lo + 1) * 16
    T, Wt, C = np.zeros(dims), np.zeros(dims), np.zeros(tuple(dims) + (3,))
    for b in bs:
        o = (np.array(b) - lo) * 16
        sl = tuple(slice(o[k], o[k] + 16) for k in range(3))
        t, w, c = blocks[b]
        T[sl], Wt[sl] = np.asarray(t, np.float64).reshape(16, 16, 16), np.asarray(w, np.float64).reshape(16, 16, 16)
        if c is not None:
            C[sl] = np.asarray(c, np.float64).reshape(16, 16, 16, 3)
    valid, inside = Wt > 0, T < 0
    X, Y, Z = dims

    def cell_valid(p):
        if min(p) < 0 or p[0] > X - 2 or p[1] > Y - 2 or p[2] > Z - 2:
            return False
        return all(valid[tuple(p + o)] for o in CORNERS)

    def order(p):   # (block rank, local linear index) of lattice point / cell p
        b = tuple(int(x) for x in (p // 16 + lo))
        l = p % 16
        return rank.get(b, -1), int((l[0] * 16 + l[1]) * 16 + l[2])

    n_in = sum(inside[o[0]:X - 1 + o[0], o[1]:Y - 1 + o[1], o[2]:Z - 1 + o[2]].astype(np.int64) for o in CORNERS)
    cand = [p for p in np.argwhere((n_in > 0) & (n_in < 8)) if cell_valid(p)]
    cand.sort(key=order)
    vid, verts, cols = {}, [], []
    for p in cand:
        acc, cacc, n = np.zeros(3), np.zeros(3), 0
        for axis in range(3):
            step = 4 >> axis
            for n0 in range(8):
                if n0 & step:
                    continue
                p0, p1 = tuple(p + CORNERS[n0]), tuple(p + CORNERS[n0 + step])
                if inside[p0] == inside[p1]:
                    continue
                t = (0.0 - T[p0]) / (T[p1] - T[p0])
                pt = CORNERS[n0].astype(np.float64)
                pt[axis] = t
                acc += pt
                cacc += C[p0] + t * (C[p1] - C[p0])
                n += 1
        vid[tuple(p)] = len(verts)
        g = p + lo * 16
        verts.append(np.float64(np.float32(voxel_length)) * ((g + 0.5) + acc / n))
        cols.append(cacc / n / 255.0)
    quads = []
    eye = np.eye(3, dtype=np.int64)
    for a in range(3):
        b, c = eye[(a + 1) % 3], eye[(a + 2) % 3]
        sl0 = tuple(slice(0, dims[k] - (k == a)) for k in range(3))
        sl1 = tuple(slice(int(k == a), dims[k]) for k in range(3))
        for q in np.argwhere(inside[sl0] != inside[sl1]):
            cells = (q, q - b, q - b - c, q - c)
            if all(cell_valid(p) for p in cells):
                quads.append((order(q) + (a,), [vid[tuple(p)] for p in cells], bool(inside[tuple(q)])))
    quads.sort(key=lambda x: x[0])
    faces = []
    for _, (c00, c10, c11, c01), qin in quads:
        faces += [[c00, c10, c11], [c00, c11, c01]] if qin else [[c00, c11, c10], [c00, c01, c11]]
    out = (np.array(verts, np.float64).reshape(-1, 3), np.array(faces, np.int64).reshape(-1, 3),
           np.array(cols, np.float64).reshape(-1, 3))
    return out + (np.array([p + lo * 16 for p in cand], np.int64).reshape(-1, 3),) if return_cells else out


# ---- hand-made volumes ----

def make_blocks(block_list, field, voxel_length, weight=None):
    """{(bx, by, bz): (tsdf float32 [4096], weight float32 [4096], colour float32 [4096, 3])}: tsdf = field(x, y, z) at the voxel
    centres (float64, rounded to float32), weight 1 (or weight(gx, gy, gz)), colour a fixed function of the voxel coordinates."""
    out = {}
    for b in block_list:
        g = np.asarray(b)[None] * 16 + LOCAL
        c = voxel_length * (g + 0.5)
        t = field(c[:, 0], c[:, 1], c[:, 2]).astype(np.float32)
        w = np.ones(4096, np.float32) if weight is None else weight(g[:, 0], g[:, 1], g[:, 2]).astype(np.float32)
        col = np.stack([(37 * g[:, 0] + 11 * g[:, 1]) % 256, (53 * g[:, 1] + 7 * g[:, 2]) % 256, (29 * g[:, 2] + 13 * g[:, 0]) % 256], -1)
        out[tuple(int(x) for x in b)] = (t, w, col.astype(np.float32))
    return out


def volume_arrays(blocks):
    """(keys [B] int64 ascending, tsdf [B, 4096], weight [B, 4096], colour [B, 4096, 3]) of a block dictionary."""
    bs = sorted(blocks)
    return (np.array([key_of(b) for b in bs], np.int64), np.stack([blocks[b][0] for b in bs]), np.stack([blocks[b][1] for b in bs]),
            np.stack([blocks[b][2] for b in bs]))


def gather_dense(blocks):
    """The dense grid [X, Y, Z] float32 over the blocks' bounding box (which they must fill) and the coordinates of its first
    voxel."""
    bs = sorted(blocks)
    lo = np.min(np.array(bs), 0)
    dims = (np.max(np.array(bs), 0) - lo + 1) * 16
    assert len(bs) == int(np.prod(dims // 16))
    T = np.zeros(dims, np.float32)
    for b in bs:
        o = (np.array(b) - lo) * 16
        T[o[0]:o[0] + 16, o[1]:o[1] + 16, o[2]:o[2] + 16] = blocks[b][0].reshape(16, 16, 16)
    return T, lo * 16


SURFACE_VOXEL = 0.0625   # a power of two: voxel_length (g + 0.5 + frac) and x[i] + frac (x[i + 1] - x[i]) round alike


def surface_cases():
    """name -> (blocks, voxel_length): the hand-made volumes of the surface tests."""
    vl = SURFACE_VOXEL
    eight = [(x, y, z) for x in (-1, 0) for y in (-1, 0) for z in (-1, 0)]
    r = 0.9 * vl * 16
    sphere = lambda x, y, z: np.sqrt(x * x + y * y + z * z) - r
    cases = {
        "sphere_8_blocks": make_blocks(eight, sphere, vl),
        "sphere_hole": make_blocks([b for b in eight if b != (0, -1, 0)], sphere, vl),
        "sphere_unseen_layer": make_blocks(eight, sphere, vl, weight=lambda gx, gy, gz: (gy != 3).astype(np.float32)),
        # the plane x = 16 voxel_length is the face between blocks 0 and 1: the voxel centres lie half a voxel off it
        "plane_in_block_face": make_blocks([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)], lambda x, y, z: x - 16 * vl, vl),
        "single_block": make_blocks([(2, -3, 5)], lambda x, y, z: sphere(x - (2 * 16 + 8) * vl, y - (-3 * 16 + 8) * vl, z - (5 * 16 + 8) * vl) + 0.5 * r, vl),
        "tilted_plane_3x1x1": make_blocks([(-1, 4, 4), (0, 4, 4), (1, 4, 4)],
                                          lambda x, y, z: 0.31 * x + 0.52 * (y - 72.3 * vl) + 0.8 * (z - 71.6 * vl), vl),
    }
    return {k: (v, vl) for k, v in cases.items()}
