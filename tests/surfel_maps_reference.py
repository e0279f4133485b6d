"""float64 torch yardstick for the per-pixel tail of the 2DGS render() (gs2d_maps.hip: the five render maps from the
rasterizer's allmap[7,H,W], forward and backward) and for the two regularisers of train_2dgs.py:142-150 on it, over
oracle/surfel_maps_ref.py (its depth_to_normal and camera_rays).  Not a test module: tests/test_surfel_maps_cpu.py and
tests/test_surfel_maps_edges_gpu.py import it.

Every decision is taken on the float32 data, as the kernel and the restatement take it: where the float32 quotient
allmap[0] / allmap[1] is NaN or infinite the expected depth is 0 and passes no gradient, where allmap[5] is NaN or +inf the
median depth is 0 and passes no gradient.  The arithmetic after the decisions is float64 (or, for e_ref, the same functions
in float32 on the CPU: |float32 - float64| is the measure every tolerance of the GPU tests is taken from, and it never
involves the kernel).
"""
import math

import torch

from oracle.surfel_maps_ref import camera_rays, depth_to_normal

MAPS = ("render_alpha", "render_normal", "render_dist", "surf_depth", "surf_normal")
INF = float("inf")


def decisions(allmap):
    """(expected depth is kept, median depth is kept), [1,H,W] bool each, from the float32 data."""
    a = allmap.detach().float()
    m = a[5:6]
    return torch.isfinite(a[0:1] / a[1:2]), ~(torch.isnan(m) | (m == INF))


def maps_from_allmap(a, e_ok, m_ok, view, rays_d, rays_o, depth_ratio, alpha_weight=None):
    """The five maps as oracle.surfel_maps_ref.surfel_maps_ref forms them, in the dtype of `a`, nan_to_num replaced by the
    decisions handed in.  alpha_weight: the alpha that weights surf_normal (default: this allmap's, detached - a finite
    difference hands in the unperturbed one, which is what detaching means for a difference quotient)."""
    alpha = a[1:2]
    rn = (a[2:5].permute(1, 2, 0) @ (view[:3, :3].T)).permute(2, 0, 1)
    zero = torch.zeros_like(alpha)
    expected = torch.where(e_ok, a[0:1] / alpha, zero)
    median = torch.where(m_ok, a[5:6], zero)
    sd = expected * (1 - depth_ratio) + depth_ratio * median
    sn = depth_to_normal(rays_d, rays_o, sd).permute(2, 0, 1) * (alpha.detach() if alpha_weight is None else alpha_weight)
    return alpha, rn, a[6:7], sd, sn


def frame_lengths(sd, rays_d, rays_o):
    """|dv x dh| of every interior centre, [H-2,W-2] (empty for an image without one), in the dtype of sd."""
    pts = (sd.reshape(-1, 1) * rays_d + rays_o).reshape(*sd.shape[1:], 3)
    dx = pts[2:, 1:-1] - pts[:-2, 1:-1]
    dy = pts[1:-1, 2:] - pts[1:-1, :-2]
    return torch.linalg.cross(dx, dy, dim=-1).norm(dim=-1)


def _zero_the_documented_entries(g, allmap, g_alpha=None):
    """include/scorp_gs.h: 'where PyTorch's chain yields 0/0 = NaN (empty pixels) it writes 0' - channels 0 and 1 at
    allmap[1] == 0 only.  The zero stands for the chain through the quotient allmap[0] / allmap[1], which is all that reaches
    channel 0; channel 1 also carries the weight of render_alpha itself, which stays (tests/test_gs2d_gpu.py pins the same).
    The float32 run (e_ref) also has 0 * inf = NaN where a subnormal alpha overflows 1 / alpha: the float32 quotient is not
    finite there, no gradient passes, and float64 has an exact 0 - so the entries are those where the quotient is not kept,
    which in float64 are the ones with allmap[1] == 0."""
    empty = ~decisions(allmap)[0].expand_as(g[:2]) if g.dtype == torch.float32 else (allmap[1] == 0).expand_as(g[:2])
    direct = torch.zeros_like(g[:2])
    if g_alpha is not None:
        direct[1] = g_alpha.detach().to(g.dtype).reshape(g.shape[1:])
    g[:2] = torch.where(empty & torch.isnan(g[:2]), direct, g[:2])
    return g


def _setup(allmap, view, rays_d, rays_o, dtype):
    e_ok, m_ok = decisions(allmap)
    a = allmap.detach().float().to(dtype).requires_grad_(True)
    return a, e_ok, m_ok, view.detach().to(dtype), rays_d.detach().to(dtype), rays_o.detach().to(dtype)


def maps_autograd(allmap, view, rays_d, rays_o, depth_ratio, ws, dtype=torch.float64):
    """([render_alpha, render_normal, render_dist, surf_depth, surf_normal], g_allmap) for the loss sum_k (map_k * w_k).sum();
    any w_k may be None (all of them: a zero gradient)."""
    a, e_ok, m_ok, v, rd, ro = _setup(allmap, view, rays_d, rays_o, dtype)
    maps = maps_from_allmap(a, e_ok, m_ok, v, rd, ro, depth_ratio)
    terms = [(m * w.detach().to(dtype)).sum() for m, w in zip(maps, ws) if w is not None]
    g = torch.autograd.grad(sum(terms), a)[0] if terms else torch.zeros_like(a)
    return [m.detach() for m in maps], _zero_the_documented_entries(g.detach(), allmap, ws[0])


def regularizers_autograd(allmap, view, rays_d, rays_o, depth_ratio, lambda_normal, lambda_dist, g_out2=None, dtype=torch.float64):
    """{"values": (lambda_normal mean(1 - render_normal . surf_normal), lambda_dist mean(render_dist)), "term_n", "term_d":
    the per-pixel terms [H,W], "g_allmap": the gradient of g_out2 . values (g_out2 None: (1, 1))}."""
    a, e_ok, m_ok, v, rd, ro = _setup(allmap, view, rays_d, rays_o, dtype)
    _, rn, dist, _, sn = maps_from_allmap(a, e_ok, m_ok, v, rd, ro, depth_ratio)
    term_n, term_d = 1 - (rn * sn).sum(dim=0), dist[0]
    values = torch.stack([lambda_normal * term_n.mean(), lambda_dist * term_d.mean()])
    g0, g1 = (1.0, 1.0) if g_out2 is None else g_out2
    g = torch.autograd.grad(g0 * values[0] + g1 * values[1], a)[0]
    return {"values": values.detach(), "term_n": term_n.detach(), "term_d": term_d.detach(),
            "g_allmap": _zero_the_documented_entries(g.detach(), allmap)}


def maps_e_ref(allmap, view, rays_d, rays_o, depth_ratio, ws):
    """(maps64, g64, |maps32 - maps64| per map, |g32 - g64|): the float32 CPU run of maps_autograd against the float64 one,
    per element; channel figures are the maxima the callers take of these."""
    m64, g64 = maps_autograd(allmap, view, rays_d, rays_o, depth_ratio, ws)
    m32, g32 = maps_autograd(allmap, view, rays_d, rays_o, depth_ratio, ws, dtype=torch.float32)
    return m64, g64, [(x.double() - y).abs() for x, y in zip(m32, m64)], (g32.double() - g64).abs()


def regularizers_e_ref(allmap, view, rays_d, rays_o, depth_ratio, lambda_normal, lambda_dist, g_out2=None):
    """(the float64 result, {"term_n", "term_d", "g_allmap"}: |float32 - float64| per element)."""
    r64 = regularizers_autograd(allmap, view, rays_d, rays_o, depth_ratio, lambda_normal, lambda_dist, g_out2)
    r32 = regularizers_autograd(allmap, view, rays_d, rays_o, depth_ratio, lambda_normal, lambda_dist, g_out2, dtype=torch.float32)
    return r64, {k: (r32[k].double() - r64[k]).abs() for k in ("term_n", "term_d", "g_allmap")}


def per_channel(x):
    """max over the pixels of each channel of [C,H,W] (0 for an empty selection)."""
    return x.reshape(x.shape[0], -1).amax(dim=1) if x.numel() else torch.zeros(x.shape[0], dtype=x.dtype)


# ---- the cases: shared by the CPU and the GPU tests, seeded, built on the CPU in float32 ----
CASES = ("smooth", "disc", "lines", "lines_camera", "threshold", "nonfinite")
SHAPES = ((1, 1), (1, 7), (7, 1), (2, 2), (3, 3), (4, 64), (5, 65), (6, 66), (9, 63), (8, 128), (13, 130), (12, 129), (3, 321))
RATIOS = (0.0, 1.0, 0.5)
SUBNORMAL_ALPHA = 1e-42      # 1 / 1e-42 overflows float32 and not float64


class Case:
    """allmap [7,H,W], view [4,4], rays_d [H*W,3], rays_o [3] (float32, CPU); planted: [H,W] bool, the pixels whose g_allmap
    channels 0, 1 and 5 are compared per element, planted_normals: those whose surf_normal is (both listed by coordinate
    here, never taken from a kernel's output); centres / sites: the planted coordinates by name."""

    def __init__(self, allmap, view, rays_d, rays_o, planted, centres=None, sites=None, planted_normals=None):
        self.allmap, self.view, self.rays_d, self.rays_o, self.planted = allmap, view, rays_d, rays_o, planted
        self.planted_normals = torch.zeros_like(planted) if planted_normals is None else planted_normals
        self.centres, self.sites = centres or {}, sites or {}


def _grid(H, W):
    return torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")


def _smooth_allmap(H, W, g, covered=None):
    ys, xs = _grid(H, W)
    depth = 2.5 + 0.5 * torch.sin(xs / 7.0) + 0.3 * torch.cos(ys / 5.0)
    alpha = 0.3 + 0.6 * torch.rand(H, W, generator=g)
    n = torch.nn.functional.normalize(torch.randn(3, H, W, generator=g), dim=0) * alpha
    allmap = torch.stack([depth * alpha, alpha, n[0], n[1], n[2], depth + 0.02, 0.01 * torch.rand(H, W, generator=g)])
    if covered is not None:
        allmap = allmap * covered      # an empty pixel is all zeros, as the rasterizer leaves it
    return allmap


def _neighbours(mask, count=False):
    """The pixels with a 4-neighbour in mask (count: how many of the four are)."""
    m = torch.zeros(mask.shape[0] + 2, mask.shape[1] + 2, dtype=torch.int64)
    m[1:-1, 1:-1] = mask
    n = m[:-2, 1:-1] + m[2:, 1:-1] + m[1:-1, :-2] + m[1:-1, 2:]
    return n if count else n > 0


def _shifted(mask, dy, dx):
    """mask moved by (dy, dx), False moving in."""
    H, W = mask.shape
    m = torch.zeros(H + 2, W + 2, dtype=torch.bool)
    m[1:-1, 1:-1] = mask
    return m[1 - dy:1 - dy + H, 1 - dx:1 - dx + W]


def threshold_centres(H, W):
    """{"clamp": (y, x), "normalise": (y, x)}: two interior centres four columns apart, the first one on a tile seam where the
    image has one (its lower neighbour in the next tile row, its right neighbour in the next tile column); a centre that
    does not fit in the image is left out."""
    out = {}
    if H >= 3 and W >= 3:
        y, x = min(3, H - 2), min(63, W - 2)
        out["clamp"] = (y, x)
        if x - 4 >= 1:
            out["normalise"] = (y, x - 4)
        elif x + 4 <= W - 2:
            out["normalise"] = (y, x + 4)
    return out


def nonfinite_sites(H, W):
    """{"subnormal_alpha" | "nan_median" | "inf_median": [(y, x), ...]}: on the image border, on both sides of the first tile
    seam (rows 3 | 4, columns 63 | 64) and clipped into the image; a subnormal alpha may share its pixel with a planted
    median (different channels); a pixel both medians claim is NaN."""
    cl = lambda y, x: (min(y, H - 1), min(x, W - 1))
    nan = {(H - 1, W - 1), cl(3, 64), cl(5, 62), cl(1, 2)}
    return {"subnormal_alpha": sorted({(0, 0), cl(3, 63), cl(4, 64), cl(2, W - 1)}), "nan_median": sorted(nan),
            "inf_median": sorted({(H - 1, 0), cl(4, 63), cl(2, 65), cl(1, 4)} - nan)}


def make_case(name, H, W, seed=0):
    from scorp_amd.synthetic import ring_cameras
    g = torch.Generator().manual_seed(1000 * H + W + 7919 * seed)
    cam = ring_cameras(3, W, H, 11)[1]
    view = cam.world_view_transform.float().contiguous()
    rays_d, rays_o = camera_rays(cam.world_view_transform, cam.full_proj_transform, W, H)
    rays_d, rays_o = rays_d.float().contiguous(), rays_o.float().contiguous()
    ys, xs = _grid(H, W)
    none = torch.zeros(H, W, dtype=torch.bool)
    if name == "smooth":
        return Case(_smooth_allmap(H, W, g), view, rays_d, rays_o, none)
    if name == "disc":
        covered = (xs - (W - 1) / 2) ** 2 + (ys - (H - 1) / 2) ** 2 >= (min(H, W) / 4) ** 2
        return Case(_smooth_allmap(H, W, g, covered), view, rays_d, rays_o, none)
    if name == "lines_camera":
        # the lines on the smooth surface under the ring camera.  Its clamp-branch entries are ill-conditioned - a frame's one
        # vector is the float32 difference of two points three units from the origin and a fiftieth apart, and (G / eps) x dv
        # then meets a ray it is nearly perpendicular to: the float32 run of the yardstick itself is off by 2e-4 of such an
        # element at 9 x 63 and by 14 % of one at 3 x 321 - so nothing is planted here (every channel is held by its maximum)
        # and the per-element comparison runs on "lines" below, which has the same lines on exactly representable points
        yl, xl = H // 2, W // 2
        return Case(_smooth_allmap(H, W, g, (xs == xl) | (ys == yl)), view, rays_d, rays_o, none, centres={"cross": (yl, xl)})
    if name == "lines":
        # depth 2 and alpha of three bits on the lines, rays (0, 0, 1) tilted by 2^-4 per pixel ALONG a line on that line's own
        # pixels only, rays_o = 0: a line centre's one vector is exactly (0, 1/4, 0) or (1/4, 0, 0), the other exactly zero;
        # (G / eps) x dv is an exact scaling of G / eps and reaches the empty neighbour through the ray (0, 0, 1) as one term
        yl, xl = H // 2, W // 2
        covered = (xs == xl) | (ys == yl)
        alpha = (4 + torch.randint(0, 4, (H, W), generator=g)) / 8.0
        n = torch.nn.functional.normalize(torch.randn(3, H, W, generator=g), dim=0) * alpha
        allmap = torch.stack([2.0 * alpha, alpha, n[0], n[1], n[2], torch.full((H, W), 2.0), 0.01 * torch.rand(H, W, generator=g)]) * covered
        rays = torch.zeros(H, W, 3)
        rays[..., 2] = 1.0
        rays[yl, :, 0] = (torch.arange(W) - xl) * 2.0 ** -4
        rays[:, xl, 1] = (torch.arange(H) - yl) * 2.0 ** -4
        # planted: the empty pixels next to exactly one line pixel - where the clamp branch of that one centre writes.  (The
        # four empty pixels diagonal to the crossing take the sum of two such entries, which may cancel; they stay with
        # their channel.)
        planted = ~covered & (_neighbours(covered, count=True) == 1)
        return Case(allmap, torch.eye(4), rays.reshape(-1, 3).contiguous(), torch.zeros(3), planted, centres={"cross": (yl, xl)})
    if name == "threshold":
        alpha = 0.3 + 0.6 * torch.rand(H, W, generator=g)
        n = torch.nn.functional.normalize(torch.randn(3, H, W, generator=g), dim=0) * alpha
        one = torch.ones(H, W)
        allmap = torch.stack([alpha, alpha, n[0], n[1], n[2], one, 0.01 * torch.rand(H, W, generator=g)])   # depth 1 everywhere
        rays = torch.zeros(H, W, 3)
        rays[..., 2] = 1.0
        centres, tilted = threshold_centres(H, W), none.clone()
        for kind, (y, x) in centres.items():
            rays[y + 1, x, 0] = 2.0 ** -20                                        # dv = (2^-20, 0, 0)
            rays[y, x + 1, 1] = 2.0 ** -20 if kind == "clamp" else 2.0 ** -19     # dh = (0, 2^-20 | 2^-19, 0)
            tilted[y + 1, x] = tilted[y, x + 1] = True
        # planted: a tilted ray above or below an interior centre makes its dv non-zero, one to its left or right its dh
        # (every other vector is exactly zero); g_dh = gc x dv reaches the centre's horizontal neighbours, g_dv = dh x gc its
        # vertical ones, 1e4 to 1e7 - those pixels.  Every other pixel has no frame gradient at all.
        interior = none.clone()
        interior[1:-1, 1:-1] = True
        has_dv = (_shifted(tilted, 1, 0) | _shifted(tilted, -1, 0)) & interior
        has_dh = (_shifted(tilted, 0, 1) | _shifted(tilted, 0, -1)) & interior
        planted = _shifted(has_dv, 0, 1) | _shifted(has_dv, 0, -1) | _shifted(has_dh, 1, 0) | _shifted(has_dh, -1, 0)
        return Case(allmap, torch.eye(4), rays.reshape(-1, 3).contiguous(), torch.zeros(3), planted, centres=centres,
                    planted_normals=has_dv & has_dh)
    if name == "nonfinite":
        allmap, sites = _smooth_allmap(H, W, g), nonfinite_sites(H, W)
        for y, x in sites["subnormal_alpha"]:
            allmap[1, y, x] = SUBNORMAL_ALPHA
        for y, x in sites["nan_median"]:
            allmap[5, y, x] = math.nan
        for y, x in sites["inf_median"]:
            allmap[5, y, x] = INF
        return Case(allmap, view, rays_d, rays_o, none, sites=sites)
    raise ValueError(name)


def upstream_weights(H, W, seed=0):
    """The five upstream gradient maps of the maps' backward, N(0, 1)."""
    g = torch.Generator().manual_seed(31 * H + W + 104729 * (seed + 1))
    return [torch.randn(c, H, W, generator=g) for c in (1, 3, 1, 1, 3)]
