"""Yardstick of the TSDF fusion (scorp_tsdf_fuse, scorp_amd.mesh.tsdf_fuse): a torch-CPU restatement of the reference's
compute_sdf_perframe / compute_unbounded_tsdf (gs2dgs/utils/mesh_utils.py:196-247) with a dtype argument, the analytic
scene the tests fuse (a unit sphere over a ground plane, ray-cast in numpy), its sample sets, and the rule that leaves out
the samples whose decisions are too close to call.  Restated, not copied: F.grid_sample itself and the same masked
read-modify-write statements, one view at a time."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

W, H = 48, 40          # W != H, neither a multiple of 16
CENTER = (0.1, -0.05, 0.2)
RADIUS = 1.5
VOXEL = 0.04
MARGIN = 1e-5          # a decision closer than this to its threshold (float64) leaves the sample out


def uncontract(y):
    """The inverse contraction (what mesh_utils.py:192-194 computes): the unit ball stays, a point of norm n >= 1 goes to
    (y / n) / (2 - n), rounded in that order."""
    n = torch.linalg.vector_norm(y, dim=-1, keepdim=True)
    stretched = (y / n) * (1 / (2 - n))
    return torch.where(n < 1, y, stretched)


def sdf_per_frame(points, depthmap, rgbmap, full_proj):
    """mesh_utils.py:196-207: points [M,3], depthmap [1,H,W], rgbmap [3,H,W] -> (sdf [M,1], rgb [M,3], mask [M])."""
    proj = torch.cat([points, torch.ones_like(points[..., :1])], dim=-1) @ full_proj          # :200
    z = proj[..., -1:]                                                                          # :201
    pix = proj[..., :2] / proj[..., -1:]                                                        # :202
    mask = ((pix > -1.) & (pix < 1.) & (z > 0)).all(dim=-1)                                     # :203
    depth = F.grid_sample(depthmap[None], pix[None, None], mode="bilinear", padding_mode="border",
                          align_corners=True).reshape(-1, 1)                                    # :204
    rgb = F.grid_sample(rgbmap[None], pix[None, None], mode="bilinear", padding_mode="border",
                        align_corners=True).reshape(3, -1).T                                    # :205
    return depth - z, rgb, mask                                                                 # :206-207


def unbounded_tsdf(samples, depth, rgb, full_proj, voxel_size, contracted, center=None, radius=None, dtype=torch.float32,
                   return_hits=False):
    """mesh_utils.py:209-247 in `dtype`: samples [M,3], depth [V,H,W], rgb [V,3,H,W], full_proj [V,4,4] (the inputs are
    cast, so the float64 run starts from the same fp32 numbers).  -> (tsdfs [M], rgbs [M,3]) and, with return_hits, the
    per-view update masks [V,M]."""
    samples, depth, rgb, full_proj = (t.to(dtype) for t in (samples, depth, rgb, full_proj))
    if contracted:
        mask = torch.linalg.norm(samples, dim=-1) > 1                                           # :214
        trunc = 5 * voxel_size * torch.ones_like(samples[:, 0])                                 # :216
        trunc[mask] *= 1 / (2 - torch.linalg.norm(samples, dim=-1)[mask].clamp(max=1.9))        # :217
        samples = uncontract(samples) * radius + torch.as_tensor(center, dtype=dtype, device=samples.device)   # :218, 250-251
    else:
        trunc = 5 * voxel_size                                                                  # :220
    tsdfs = torch.ones_like(samples[:, 0]) * 1                                                  # :222
    rgbs = torch.zeros((samples.shape[0], 3), dtype=dtype, device=samples.device)               # :223
    weights = torch.ones_like(samples[:, 0])                                                    # :225
    hits = []
    for i in range(depth.shape[0]):                                                             # :226
        sdf, c, mask_proj = sdf_per_frame(samples, depth[i][None], rgb[i], full_proj[i])        # :227-231
        sdf = sdf.flatten()                                                                     # :234
        mask_proj = mask_proj & (sdf > -trunc)                                                  # :235
        sdf = torch.clamp(sdf / trunc, min=-1.0, max=1.0)[mask_proj]                            # :236
        w = weights[mask_proj]                                                                  # :237
        wp = w + 1                                                                              # :238
        tsdfs[mask_proj] = (tsdfs[mask_proj] * w + sdf) / wp                                    # :239
        rgbs[mask_proj] = (rgbs[mask_proj] * w[:, None] + c[mask_proj]) / wp[:, None]           # :240
        weights[mask_proj] = wp                                                                 # :242
        if return_hits:
            hits.append(mask_proj.clone())
    return (tsdfs, rgbs, torch.stack(hits)) if return_hits else (tsdfs, rgbs)


def kept_mask(samples, depth, full_proj, voxel_size, contracted, center=None, radius=None):
    """False for a sample one of whose decisions, in any view, lies within MARGIN of its threshold in float64: pix
    against +-1 (the threshold's scale is 1), zc against 0 (absolute), sdf against -trunc (relative to trunc)."""
    dt = torch.float64
    samples, depth, full_proj = samples.to(dt), depth.to(dt), full_proj.to(dt)
    if contracted:
        n = torch.linalg.norm(samples, dim=-1)
        trunc = 5 * voxel_size * torch.ones_like(n)
        trunc[n > 1] *= 1 / (2 - n[n > 1].clamp(max=1.9))
        samples = uncontract(samples) * radius + torch.as_tensor(center, dtype=dt)
    else:
        trunc = torch.full_like(samples[:, 0], 5 * voxel_size)
    keep = torch.ones(samples.shape[0], dtype=torch.bool)
    dummy = torch.zeros(3, *depth.shape[1:], dtype=dt)
    for i in range(depth.shape[0]):
        proj = torch.cat([samples, torch.ones_like(samples[:, :1])], -1) @ full_proj[i]
        zc, pix = proj[:, 3], proj[:, :2] / proj[:, 3:]
        sdf = sdf_per_frame(samples, depth[i][None], dummy, full_proj[i])[0].flatten()
        near = ((pix.abs() - 1).abs() < MARGIN).any(-1) | (zc.abs() < MARGIN) | ((sdf + trunc).abs() < MARGIN * trunc)
        keep &= ~near
    return keep


# ---- the scene: a unit sphere at the origin over the plane z = -1, seen by five cameras ----

def cameras():
    """Three cameras round the object, one INSIDE the sample cloud looking outwards (part of the samples have zc <= 0), one
    looking past the object (its frustum misses part of the samples)."""
    from scorp_amd.camera import look_at_camera
    fov, up = math.radians(60.0), (0, 0, 1)
    return [look_at_camera((4.0, 0.0, 1.0), (0, 0, 0), up, fov, (W, H)),
            look_at_camera((-2.0, 3.4, 1.8), (0, 0, 0), up, fov, (W, H)),
            look_at_camera((-1.5, -3.2, 0.4), (0, 0, 0), up, fov, (W, H)),
            look_at_camera((0.6, 0.3, 1.4), (3.0, 1.0, 0.0), up, fov, (W, H)),
            look_at_camera((3.0, -3.0, 2.0), (0.0, 2.5, 0.0), up, math.radians(35.0), (W, H))]


def raycast_depth(cam, far=12.0, size=None):
    """Camera-space z of the nearest hit of every pixel's ray with the unit sphere or the plane z = -1 (numpy float64; the
    pixel centres are where grid_sample with align_corners puts them), `far` where the ray hits nothing."""
    w, h = size or (W, H)
    wv = cam.world_view_transform.numpy().astype(np.float64)          # row-vector convention: p_cam = [p 1] @ wv
    c2w = np.linalg.inv(wv)
    ndc_x, ndc_y = np.linspace(-1, 1, w), np.linspace(-1, 1, h)
    d_cam = np.stack(np.broadcast_arrays(ndc_x[None, :] * math.tan(cam.FoVx / 2), ndc_y[:, None] * math.tan(cam.FoVy / 2),
                                         np.ones((h, w))), -1)        # z component 1: the ray parameter is the depth
    d = d_cam @ c2w[:3, :3]
    o = c2w[3, :3]
    depth = np.full((h, w), far)
    b, c = (d * o).sum(-1), (o * o).sum() - 1.0
    a = (d * d).sum(-1)
    disc = b * b - a * c
    for sign in (-1.0, 1.0):
        with np.errstate(invalid="ignore"):
            t = (-b + sign * np.sqrt(disc)) / a
        ok = (disc >= 0) & (t > 1e-6) & (t < depth)
        depth[ok] = t[ok]
    with np.errstate(divide="ignore"):
        t = (-1.0 - o[2]) / d[..., 2]
    ok = np.isfinite(t) & (t > 1e-6) & (t < depth)
    depth[ok] = t[ok]
    return depth.astype(np.float32)


@functools.lru_cache(maxsize=None)
def scene(num_views=5):
    """(depth [V,H,W], rgb [V,3,H,W], full_proj [V,4,4]) fp32 CPU tensors; rgb is seeded noise."""
    cams = cameras()[:num_views]
    depth = torch.from_numpy(np.stack([raycast_depth(c) for c in cams]))
    rgb = torch.from_numpy(np.random.default_rng(11).random((len(cams), 3, H, W), dtype=np.float32))
    return depth, rgb, torch.stack([c.full_proj_transform for c in cams]).contiguous()


SEED = 5   # tests/test_tsdf_cpu.py checks that with it the fp32 restatement flips no decision among the kept samples


def point_samples(m=3 * 64 * 64 + 17, seed=SEED):
    """Contracted-space points: uniform directions, norms uniform in [0, 1.97]."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(m, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return torch.from_numpy((d * rng.uniform(0.0, 1.97, (m, 1))).astype(np.float32))


def lattice_coords(scale=1.0):
    """33 x 17 x 9, unequal extents (contracted space at scale 1: the corners reach norm 1.8)."""
    return (torch.linspace(-1.2 * scale, 1.2 * scale, 33), torch.linspace(-1.0 * scale, 1.0 * scale, 17),
            torch.linspace(-0.8 * scale, 0.9 * scale, 9))


def lattice_points(coords):
    return torch.stack(torch.meshgrid(*coords, indexing="ij"), dim=-1).reshape(-1, 3).contiguous()


def colour_samples(m=1000, seed=SEED + 1):
    """World-space points within 0.3 of the sphere's surface (where mesh vertices would lie)."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(m, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return torch.from_numpy((d * rng.uniform(0.7, 1.3, (m, 1))).astype(np.float32))


@functools.lru_cache(maxsize=None)
def case(name, num_views=5):
    """One named sample set against the scene, evaluated once: dict(samples, contracted, kw, ref32, rgb32, ref64, rgb64,
    hits32, hits64, keep, e_ref, e_ref_rgb).  name: points | lattice_contracted | lattice_plain | colour."""
    depth, rgb, fp = scene(num_views)
    coords = None
    if name == "points":
        samples, contracted = point_samples(), True
    elif name == "lattice_contracted":
        coords, contracted = lattice_coords(1.0), True
        samples = lattice_points(coords)
    elif name == "lattice_plain":
        coords, contracted = lattice_coords(1.6), False
        samples = lattice_points(coords)
    elif name == "colour":
        samples, contracted = colour_samples(), False
    else:
        raise KeyError(name)
    kw = dict(center=CENTER, radius=RADIUS) if contracted else {}
    t32, c32, h32 = unbounded_tsdf(samples, depth, rgb, fp, VOXEL, contracted, dtype=torch.float32, return_hits=True, **kw)
    t64, c64, h64 = unbounded_tsdf(samples, depth, rgb, fp, VOXEL, contracted, dtype=torch.float64, return_hits=True, **kw)
    keep = kept_mask(samples, depth, fp, VOXEL, contracted, **kw)
    return dict(samples=samples, coords=coords, contracted=contracted, kw=kw, ref32=t32, rgb32=c32, ref64=t64, rgb64=c64,
                hits32=h32, hits64=h64, keep=keep, e_ref=float((t32.double() - t64)[keep].abs().max()),
                e_ref_rgb=float((c32.double() - c64)[keep].abs().max()))
