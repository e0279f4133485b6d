"""V views of ONE Gaussian or surfel set in one launch set (`ScorpGs3dInputs.num_views`, include/scorp_gs.h), forward only.

The align loop renders an object from ~15 cameras per pose hypothesis (align_3dgs_clpe_9dof.py:157-169,336-368).  A
100 k-Gaussian object at 800x800 cannot fill an MI355X: one such render is a chain of seven launch-latency-bound kernels
(147 us for ~25 MB of traffic).  Stacked, the V views are ONE image of V x H rows and V x N virtual Gaussians - the size
of the training benchmark's frame - and go through the same preprocess -> bin -> sort -> blend kernels once.

Both model kinds: a `GaussianModel` goes through the 3DGS entry points, a `GaussianModel2D` (the objects of
align_2dgs_clpe_9dof.py) through the 2DGS ones; the kind is read off the model (`segment._model_kind`).
"""
import ctypes
import math

import torch

from . import _C
from .rasterizer3d import _GS2D, GaussianRasterizationSettings, PairPolicy, _preprocess, _ptr, _raw_inputs, _stream
from .segment import _model_kind


class ViewStack:
    """The cameras of a stacked render: matrices as [V,4,4] / [V,3] device tensors (row-vector convention, as
    `Camera.world_view_transform` / `full_proj_transform` / `camera_center`), one resolution and field of view."""

    def __init__(self, cameras, device=None):
        c0 = cameras[0]
        for c in cameras:
            if tuple(c.resolution) != tuple(c0.resolution) or abs(c.FoVx - c0.FoVx) > 1e-12 or abs(c.FoVy - c0.FoVy) > 1e-12:
                raise ValueError("a ViewStack needs cameras of one resolution and field of view")
        dev = device or c0.world_view_transform.device
        self.W, self.H = int(c0.resolution[0]), int(c0.resolution[1])
        if self.H % 16:
            raise ValueError("stacked views need an image height that is a multiple of 16")
        self.tanfovx, self.tanfovy = math.tan(c0.FoVx * 0.5), math.tan(c0.FoVy * 0.5)
        self.view = torch.stack([c.world_view_transform.to(dev) for c in cameras]).float().contiguous()
        self.proj = torch.stack([c.full_proj_transform.to(dev) for c in cameras]).float().contiguous()
        self.campos = torch.stack([c.camera_center.to(dev) for c in cameras]).float().contiguous()
        self.V = len(cameras)

    def moved(self, R, d):
        """The same cameras as seen from an object that was moved by x -> R x + d (R [...,3,3], d [...,3]; leading
        hypothesis dimensions broadcast): rendering the MOVED object from these cameras equals rendering the object as
        it is from the returned ones.  In the row-vector convention x_row -> x_row R^T + d, so every matrix is
        multiplied from the left by M = [[R^T, 0], [d, 1]]; the camera centre goes to (c - d) R.  Returns
        (view [...,V,4,4], proj [...,V,4,4], campos [...,V,3])."""
        R, d = R.to(self.view), d.to(self.view)
        lead = R.shape[:-2]
        M = torch.zeros(lead + (4, 4), dtype=self.view.dtype, device=self.view.device)
        M[..., :3, :3] = R.transpose(-1, -2)
        M[..., 3, :3] = d
        M[..., 3, 3] = 1.0
        view = M.unsqueeze(-3) @ self.view
        proj = M.unsqueeze(-3) @ self.proj
        campos = (self.campos - d.unsqueeze(-2)) @ R
        return view.contiguous(), proj.contiguous(), campos.contiguous()


def _stacked_inputs(pc, stack, bg, view, proj, campos, scaling_modifier, keep):
    """ScorpGs3dInputs of the model's raw leaves seen from the V cameras of `stack` (num_views = V)."""
    settings = GaussianRasterizationSettings(
        image_height=stack.H, image_width=stack.W, tanfovx=stack.tanfovx, tanfovy=stack.tanfovy, bg=bg,
        scale_modifier=scaling_modifier, viewmatrix=view, projmatrix=proj, sh_degree=pc.active_sh_degree, campos=campos,
        prefiltered=False, debug=False)
    _, _, args = _raw_inputs(settings, pc, keep)
    args.num_views = stack.V
    return args


@torch.no_grad()
def render_stacked(pc, stack, bg, view=None, proj=None, campos=None, scaling_modifier=1.0):
    """Forward-only render of `pc` from the V cameras of `stack` (optionally with replaced matrices, e.g. from
    `stack.moved`).  Returns {"render": [3, V*H, W], "render_depth_raw": [V*H, W] (sum z alpha T, not normalised),
    "render_alpha": [V*H, W], "radii": [V, N], "num_pairs": the (tile, splat) pair count in PairPolicy's "exact" mode, else
    None}; view v is rows [v*H, (v+1)*H).  For a surfel model (GaussianModel2D): {"render": [3, V*H, W], "allmap":
    [7, V*H, W] (the rasterizer's seven maps, see `surfel_alpha_depth`), "radii": [V, N], "num_pairs"}."""
    kind = _model_kind(pc)
    xyz = pc.get_xyz
    if not xyz.is_cuda:
        raise RuntimeError(f"render_stacked needs GPU tensors (scorp_amd has no CPU path for {kind.render_image})")
    L = _C.lib()
    dev = xyz.device
    V, W, H, N = stack.V, stack.W, stack.H, xyz.shape[0]
    keep = []
    args = _stacked_inputs(pc, stack, bg, stack.view if view is None else view, stack.proj if proj is None else proj,
                           stack.campos if campos is None else campos, scaling_modifier, keep)
    Nt, Ht = V * N, V * H
    stream = _stream()
    exact = PairPolicy.mode == "exact"
    new = lambda shape: torch.empty(shape, dtype=torch.float32, device=dev)
    color, maps = new((3, Ht, W)), [new((c, Ht, W)) for c in kind.maps]   # before _preprocess, which may wait
    radii, state, pairs, capacity, num_pairs = _preprocess(kind, args, Nt, Ht, W, dev, stream, exact)
    _C.check(getattr(L, kind.render_image)(ctypes.byref(args), _ptr(state), _ptr(pairs), capacity, _ptr(color), *map(_ptr, maps),
                                           stream), kind.render_image)
    if not exact:
        PairPolicy.pend(state, Nt, Ht, W)
    if kind is _GS2D:
        return {"render": color, "allmap": maps[0], "radii": radii.view(V, N), "num_pairs": num_pairs}
    return {"render": color, "render_depth_raw": maps[0][0], "render_alpha": maps[1][0], "radii": radii.view(V, N),
            "num_pairs": num_pairs}


def surfel_alpha_depth(allmap, depth_ratio=1.0):
    """(render_alpha, render_depth) [..., H, W] of a surfel render's allmap [7, ..., H, W] as renderer2d.render forms them
    (gs2dgs/gaussian_renderer/__init__.py:139-154): alpha = allmap[1], depth = (1 - depth_ratio) * nan_to_num(allmap[0] /
    alpha, 0, 0) + depth_ratio * nan_to_num(allmap[5], 0, 0).  Per pixel, so a stacked allmap gives every band's maps."""
    alpha = allmap[1]
    expected = torch.nan_to_num(allmap[0] / alpha, 0, 0)
    median = torch.nan_to_num(allmap[5], 0, 0)
    return alpha, expected * (1 - depth_ratio) + depth_ratio * median


@torch.no_grad()
def score_stacked(pc, stack, bg, view, proj, campos, tgt_depth, tgt_alpha, acc, rows_per_score, scale, scaling_modifier=1.0,
                  depth_ratio=1.0):
    """`render_stacked` for a caller that only wants the mismatch with a target (the rotation sweep): preprocess + bin + sort
    + the scoring form of the blend (scorp_gs3d_render_score / scorp_gs2d_render_score) - no images, no colour, depth and
    alpha compared with tgt_depth / tgt_alpha [rows_per_score, W] where they are formed.  acc[j] += scale * (mismatch of rows
    [j, j + 1) * rows_per_score of the stacked image); `acc`: float32 device tensor with V * H / rows_per_score entries.
    `depth_ratio` (surfel models only): the mix of expected and median depth, as `surfel_alpha_depth`.
    Reserve-mode sizing only (the sweep verifies its launch sets with one PairPolicy.drain())."""
    kind = _model_kind(pc)
    L = _C.lib()
    xyz = pc.get_xyz
    V, W, H, N = stack.V, stack.W, stack.H, xyz.shape[0]
    keep = []
    args = _stacked_inputs(pc, stack, bg, view, proj, campos, scaling_modifier, keep)
    Nt, Ht = V * N, V * H
    assert acc.dtype == torch.float32 and acc.is_contiguous() and acc.numel() * rows_per_score == Ht
    assert tgt_depth.is_contiguous() and tgt_alpha.is_contiguous() and tgt_depth.numel() == rows_per_score * W == tgt_alpha.numel()
    stream = _stream()
    radii, state, pairs, capacity, _ = _preprocess(kind, args, Nt, Ht, W, xyz.device, stream, exact=False)
    if kind is _GS2D:
        _C.check(L.scorp_gs2d_render_score(ctypes.byref(args), _ptr(state), _ptr(pairs), capacity, _ptr(tgt_depth), _ptr(tgt_alpha),
                                           int(rows_per_score), float(depth_ratio), float(scale), _ptr(acc), stream),
                 "scorp_gs2d_render_score")
    else:
        _C.check(L.scorp_gs3d_render_score(ctypes.byref(args), _ptr(state), _ptr(pairs), capacity, _ptr(tgt_depth), _ptr(tgt_alpha),
                                           int(rows_per_score), float(scale), _ptr(acc), stream), "scorp_gs3d_render_score")
    PairPolicy.pend(state, Nt, Ht, W)
