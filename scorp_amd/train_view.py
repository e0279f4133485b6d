"""One training view in one library call: `render()` + `0.8 L1 + 0.2 (1 - SSIM)` + `loss.backward()`.

`train_view(camera, pc, pipe, bg, gt_image)` does what lines 88-150 of the reference's train_3dgs.py do for the plain
photometric loss (render -> l1_loss / ssim -> loss.backward()), with the same kernels as `renderer.render` +
`fused_loss.fused_l1_ssim_loss` + autograd, but enqueued by a single C call (`scorp_gs3d_train_view`): at ~1 ms of
device work per view the Python glue, autograd bookkeeping and a dozen ctypes calls cost about as much host time as
the GPU needs, and any hiccup of the host shows up as idle GPU.  No autograd graph is built; the gradients land in the
`.grad` of the model's six raw leaves (accumulating, like backward()), the screen-space gradient in
`out["viewspace_points"].grad` (what add_densification_stats reads, gaussian_model.py:603-605).

The pair buffer is always "reserved" (no host synchronisation): sized by `PairPolicy.capacity()` for this (model size,
resolution, stream), verified by `PairPolicy.drain()`.  The view's overflow word comes back as a device tensor
(`out["overflow"]`): `train()` hands it to `FusedAdam` (the step is skipped on the device if it is set) and masks the
densification statistics with it, so a view that overflowed its reservation changes nothing.
"""
import ctypes

import torch

from . import _C
# GaussianRasterizationSettings: kept as a name of this module (re-exported)
from .rasterizer3d import (_GS2D, _GS3D, _RAW_FIELDS, GaussianRasterizationSettings, PairPolicy,  # noqa: F401
                           _backward_flags, _camera_settings, _grads_struct, _prep, _raw_inputs, _stream)


class _View:
    """What train_view and train_view2d share: the model's raw leaves as the library reads them, the rasterizer's
    buffers (pair buffer sized by PairPolicy's reservation, no host synchronisation), the loss and backward workspaces,
    the fused optimizer step if it can be taken, and the gradient buffers.  `fill(v)` enters them into the caller's
    Scorp*TrainView, which the caller completes and issues."""

    def __init__(self, kind, name, camera, pc, bg_color, gt_image, mask, scaling_modifier, optimizer, stats,
                 grad_out=None, debug=False):
        L = _C.lib()
        xyz = pc.get_xyz
        if not xyz.is_cuda:
            raise RuntimeError(f"{name} needs GPU tensors (scorp_amd has no CPU path)")
        settings = _camera_settings(camera, bg_color, scaling_modifier, pc.active_sh_degree, debug)
        self.keep = []
        self.leaves, t, self.args = _raw_inputs(settings, pc, self.keep)
        dev, W, H, N = xyz.device, settings.image_width, settings.image_height, xyz.shape[0]
        self.dev, self.W, self.H, self.N = dev, W, H, N
        self.gt = _prep(gt_image, "gt_image")
        self.mask = None if mask is None else _prep(mask.expand(1, H, W), "mask")
        new = self.new = lambda shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)
        self.color, self.grad_color = new((3, H, W)), new((3, H, W))
        self.radii = new((N,), torch.int32)
        state_bytes = getattr(L, kind.state_bytes)(N, W, H)
        self.state = new((state_bytes,), torch.uint8)
        capacity = PairPolicy.capacity(N, H, W)
        self.pairs = new((L.scorp_gs3d_pairs_bytes(capacity),), torch.uint8)
        ws_bytes = L.scorp_loss_workspace_bytes(3, H, W)
        self.ws = new((ws_bytes,), torch.uint8)
        # rasterizer3d.backward_precision(...) / SCORP_BACKWARD_DETERMINISTIC reach the one-call views too
        flags = _backward_flags() & kind.flags_mask
        scratch_bytes = getattr(L, kind.backward_scratch_bytes_ex)(N, W, H, capacity, flags)
        self.scratch = new((scratch_bytes,), torch.uint8)
        need = [p.requires_grad for p in self.leaves]   # frozen leaves (post-refine) get no gradient buffer: NULL = not wanted
        need[1] = need[2] = need[1] or need[2]          # the SH gradient is written as a whole
        self.pack = None
        if (optimizer is not None and hasattr(optimizer, "fused_view_pack") and t[2].numel() > 0
                and all(x.data_ptr() == p.data_ptr() for x, p in zip(t, self.leaves))):
            st = None
            if stats is not None and xyz.requires_grad:
                st = tuple(s_ if (s_.dtype == torch.float32 and s_.is_contiguous()) else None for s_ in stats)
                st = None if any(s_ is None for s_ in st) else st
            self.pack = optimizer.fused_view_pack(self.leaves, st)
            stats = st
        self.fused_step = self.pack is not None
        self.stats_accumulated = self.fused_step and stats is not None
        self.g = [torch.empty_like(x) if (n and not self.fused_step) else None for x, n in zip(t, need)]
        self.grad_out = None if self.fused_step else grad_out
        if self.grad_out is not None:
            for k, (x, n, go) in enumerate(zip(t, need, grad_out)):
                if n and go is not None:
                    assert go.shape == x.shape and go.dtype == torch.float32 and go.is_contiguous() and go.device == x.device
                    self.g[k] = go
        # the screen-space gradient feeds the densification statistics: not produced when the positions are frozen
        # (renderer.render does the same), which leaves the backward with colour gradients only -> its colour-only path
        self.g_means2D = new((N, 3)) if (xyz.requires_grad and not self.stats_accumulated) else None
        self.grads = _grads_struct(_RAW_FIELDS, self.g, self.g_means2D)
        self.sizes = (state_bytes, capacity, ws_bytes, scratch_bytes, flags)

    def fill(self, v):
        """The shared fields of `v` (a ScorpGs3dTrainView or ScorpGs2dTrainView)."""
        state_bytes, capacity, ws_bytes, scratch_bytes, flags = self.sizes
        v.inputs = ctypes.addressof(self.args)
        v.out_radii, v.state, v.state_bytes, v.pairs, v.capacity = (self.radii.data_ptr(), self.state.data_ptr(), state_bytes,
                                                                    self.pairs.data_ptr(), capacity)
        v.out_color, v.grad_color = self.color.data_ptr(), self.grad_color.data_ptr()
        v.gt, v.mask = self.gt.data_ptr(), (None if self.mask is None else self.mask.data_ptr())
        v.loss_workspace, v.loss_workspace_bytes = self.ws.data_ptr(), ws_bytes
        v.grads, v.backward_scratch, v.backward_scratch_bytes = ctypes.addressof(self.grads), self.scratch.data_ptr(), scratch_bytes
        v.backward_flags = flags
        if self.fused_step:
            v.adam = ctypes.addressof(self.pack[0])

    def accumulate(self):
        """The gradients into the leaves' .grad (unless the fused step consumed them): accumulated like backward(), or
        the grad_out tensors made the .grad."""
        if self.fused_step:
            return
        for k, (p, gp) in enumerate(zip(self.leaves, self.g)):
            if p.requires_grad:
                if self.grad_out is not None and self.grad_out[k] is not None:
                    p.grad = gp.view_as(p)      # written in place of whatever was there: the arena is the gradient
                elif p.grad is None:
                    p.grad = gp.view_as(p)
                else:
                    p.grad += gp.view_as(p)

    def result(self, loss3, total, header, **own):
        """What both views return, then the view's `own` keys."""
        # "overflow": != 0 if this view needed more pairs than were reserved (its images and gradients then come from truncated
        # tile lists): a device word, so the caller can make the optimizer step conditional without a host sync
        return {"optimizer_stepped": self.fused_step, "stats_accumulated": self.stats_accumulated, "render": self.color,
                "viewspace_points": _ViewspaceGrad(self.g_means2D), "radii": self.radii, "loss": total, "l1": loss3[1],
                "ssim": loss3[2], "overflow": header.view(torch.int32)[1:2], **own}


def _any_term(depth_sensor, depth_est, *weights):
    """Was any term of ScorpGs3dViewTerms / ScorpGs2dViewTerms asked for?  (With none the plain entry point is called.)"""
    return depth_sensor is not None or depth_est is not None or any(weights)


def _depth_maps(c, depth_sensor, depth_est):
    """The two optional depth maps of a view's terms, checked against the view's size and laid out as the library reads them."""
    maps = []
    for t, name in ((depth_sensor, "depth_sensor"), (depth_est, "depth_est")):
        if t is not None:
            if t.numel() != c.H * c.W:
                raise ValueError(f"{name}: {tuple(t.shape)} is not a depth map of the view ({c.H} x {c.W})")
            t = _prep(t, name)
        maps.append(t)
    return maps


def train_view(viewpoint_camera, pc, pipe, bg_color, gt_image, lambda_dssim=0.2, mask=None, scaling_modifier=1.0,
               optimizer=None, stats=None, grad_out=None, depth_sensor=None, depth_est=None, lambda_depth_sensor=0.0,
               weight_depth_est=0.0, lambda_isotropic=0.0):
    """Returns the dict of `renderer.render` plus "loss", "l1", "ssim" (0-d views of one device tensor); parameter
    gradients are accumulated into `pc`'s leaves.  Needs the model's raw leaves (fused activations).

    `optimizer` (a FusedAdam holding the model's leaves): the optimizer step of this iteration is applied INSIDE the view, by
    the per-Gaussian backward kernel (ScorpFusedAdam, include/scorp_gs.h) - same update as optimizer.step() on the view's
    gradients, bit for bit, but the gradient rows never go to HBM: the leaves get NO .grad, the result carries
    "optimizer_stepped": True and the caller must not call optimizer.step() for this iteration.  Skipped on the device if
    the view overflowed its pair reservation (counted in optimizer.take_skipped()).  `stats` = (max_radii2D,
    xyz_gradient_accum, denom): the view's share of the densification statistics (GaussianModel.accumulate_view_stats) by
    the same kernel; then "viewspace_points".grad is None.  If the step cannot be fused (pending gradients, a leaf the
    optimizer does not hold) the view runs as without `optimizer` and says "optimizer_stepped": False.

    `grad_out` (six tensors or None entries, the leaves' order xyz, features_dc, features_rest, opacity, scaling, rotation; e.g.
    parallel.GradArena.views): the gradients are WRITTEN there (not accumulated) and become the leaves' .grad - the
    data-parallel loop's collective then reads them where the kernel left them.

    `depth_sensor` / `depth_est` ([1,H,W] or [H,W]), `lambda_depth_sensor`, `weight_depth_est` (= 10 * dn_l1_weight(iteration),
    formed by the caller as loss.depth_losses forms it) and `lambda_isotropic`: the terms train_3dgs.py:109-150 adds after
    depth_from_iter, inside the same call (scorp_gs3d_train_view_ex, ScorpGs3dViewTerms in include/scorp_gs.h: the two depth
    passes between the loss and the backward, the isotropic gradient in the per-Gaussian backward kernel - with `optimizer`
    the invisible Gaussians then take the step with that gradient alone).  The result gains "depth_sensor_loss",
    "depth_est_loss", "isotropic_loss" (unweighted, 0-d views of one device tensor) and "loss" is the total.  A term whose mask
    is empty or whose range is zero reads NaN and moves nothing.  With all five at their defaults nothing changes."""
    L = _C.lib()
    c = _View(_GS3D, "train_view", viewpoint_camera, pc, bg_color, gt_image, mask, scaling_modifier, optimizer, stats,
              grad_out, debug=bool(getattr(pipe, "debug", False)))
    H, W, N = c.H, c.W, c.N
    depth_raw, alpha, depth = c.new((1, H, W)), c.new((1, H, W)), c.new((1, H, W))
    visible, loss3 = c.new((N,), torch.uint8), c.new((3,))
    header = c.new((64,), torch.uint8)                # {pairs needed, overflow, capacity, 0}: written by the scatter kernel
    v = _C.ScorpGs3dTrainView()
    c.fill(v)
    v.lambda_dssim = float(lambda_dssim)
    v.out_depth_raw, v.out_alpha, v.out_depth, v.out_visible = depth_raw.data_ptr(), alpha.data_ptr(), depth.data_ptr(), visible.data_ptr()
    v.out_loss3, v.out_header = loss3.data_ptr(), header.data_ptr()
    terms = None
    if _any_term(depth_sensor, depth_est, lambda_depth_sensor, weight_depth_est, lambda_isotropic):
        terms, keep = _view_terms(L, c, depth_sensor, depth_est, lambda_depth_sensor, weight_depth_est, lambda_isotropic)
        _C.check(L.scorp_gs3d_train_view_ex(ctypes.byref(v), ctypes.byref(terms), _stream()), "scorp_gs3d_train_view_ex")
    else:
        _C.check(L.scorp_gs3d_train_view(ctypes.byref(v), _stream()), "scorp_gs3d_train_view")
    PairPolicy.pend(c.state, N, H, W, header=header)    # queued for drain(): no copy launch, the state blob is not pinned
    c.accumulate()
    extra, total = {}, loss3[0]
    if terms is not None:
        terms4 = keep[0]
        extra = {"photometric_loss": loss3[0], "depth_sensor_loss": terms4[1], "depth_est_loss": terms4[2], "isotropic_loss": terms4[3]}
        total = loss3[0] + terms4[0]      # the convention of the 2DGS twin: out_loss3[0] + out_terms4[0]
    return c.result(loss3, total, header, visibility_filter=visible.view(torch.bool), render_depth=depth, render_alpha=alpha, **extra)


def _view_terms(L, c, depth_sensor, depth_est, lambda_depth_sensor, weight_depth_est, lambda_isotropic):
    """The ScorpGs3dViewTerms of one view and the tensors it points to (out_terms4 first)."""
    H, W, N = c.H, c.W, c.N
    maps = _depth_maps(c, depth_sensor, depth_est)
    ws_bytes = L.scorp_gs3d_view_terms_workspace_bytes(W, H, N)
    keep = [c.new((4,)), c.new((ws_bytes,), torch.uint8), *maps]
    t = _C.ScorpGs3dViewTerms()
    t.depth_sensor, t.depth_est = (None if m is None else m.data_ptr() for m in maps)
    t.lambda_depth_sensor, t.weight_depth_est = float(lambda_depth_sensor), float(weight_depth_est)
    t.lambda_isotropic = float(lambda_isotropic)
    t.out_terms4, t.workspace, t.workspace_bytes = keep[0].data_ptr(), keep[1].data_ptr(), ws_bytes
    if maps[0] is not None or maps[1] is not None:
        keep += [c.new((H, W)), c.new((H, W))]
        t.grad_depth_raw, t.grad_alpha = keep[-2].data_ptr(), keep[-1].data_ptr()
    return t, keep


class _ViewspaceGrad:
    """What the training loop uses of `viewspace_points`: its `.grad` ([N,3], gaussian_model.py:603-605)."""
    __slots__ = ("grad",)

    def __init__(self, grad):
        self.grad = grad


def train_view2d(viewpoint_camera, pc, pipe, bg_color, gt_image, lambda_dssim=0.2, lambda_normal=0.0, lambda_dist=0.0,
                 mask=None, scaling_modifier=1.0, optimizer=None, stats=None, depth_sensor=None, depth_est=None,
                 lambda_depth_sensor=0.0, weight_depth_est=0.0, weight_depth_normal=0.0, lambda_isotropic=0.0):
    """The 2DGS twin of `train_view`: one iteration of train_2dgs.py:95-150 for the plain photometric loss plus the
    normal-consistency / depth-distortion regularisers (train_2dgs.py:142-150), enqueued by ONE library call
    (`scorp_gs2d_train_view`).  Returns "render", "allmap", "radii", "visibility_filter", "viewspace_points",
    "loss" (= photometric + normal + distortion, a 0-d device tensor), "l1", "ssim", "normal_loss", "dist_loss",
    "overflow"; parameter gradients are accumulated into the surfel model's leaves.  `optimizer` / `stats`: the optimizer
    step and the view's densification statistics inside the view, as for `train_view` (ScorpGs2dTrainView.adam).

    `depth_sensor` / `depth_est` ([1,H,W] or [H,W]), `lambda_depth_sensor`, `weight_depth_est` (= 10 * dn_l1_weight(iteration)),
    `weight_depth_normal` (= dn_l1_weight(iteration) once iteration > depth_from_iter + 1000; needs `depth_est`) and
    `lambda_isotropic`: the terms train_2dgs.py:100-139 adds after depth_from_iter, inside the same call
    (scorp_gs2d_train_view_ex, ScorpGs2dViewTerms in include/scorp_gs.h: two pixel passes between the loss and the backward, their
    gradient maps folded into the one maps backward, the isotropic gradient in the per-surfel backward kernel - with `optimizer`
    the invisible surfels then take the step with that gradient alone).  The result gains "photometric_loss",
    "depth_sensor_loss", "depth_est_loss", "depth_normal_loss", "render_normal_loss", "isotropic_loss" (unweighted, 0-d views of
    one device tensor) and "render_depth" ([1,H,W], the surface depth the terms were taken on; None when no depth map was
    given); "loss" is the total.  A depth term whose mask is empty or whose range is zero reads NaN and moves nothing.  With
    all six at their defaults the call is the one it always was."""
    from .renderer2d import _camera_rays
    L = _C.lib()
    c = _View(_GS2D, "train_view2d", viewpoint_camera, pc, bg_color, gt_image, mask, scaling_modifier, optimizer, stats)
    H, W, N = c.H, c.W, c.N
    allmap, grad_allmap, loss5 = c.new((7, H, W)), c.new((7, H, W)), c.new((5,))
    rws_bytes = L.scorp_gs2d_regularizers_workspace_bytes(W, H)
    rws = c.new((rws_bytes,), torch.uint8)
    rays_d, rays_o = _camera_rays(viewpoint_camera, c.dev)
    v = _C.ScorpGs2dTrainView()
    c.fill(v)
    v.out_allmap, v.grad_allmap = allmap.data_ptr(), grad_allmap.data_ptr()
    v.rays_d, v.rays_o = rays_d.data_ptr(), rays_o.data_ptr()
    v.lambda_dssim, v.depth_ratio = float(lambda_dssim), float(getattr(pipe, "depth_ratio", 1.0))
    v.lambda_normal, v.lambda_dist = float(lambda_normal), float(lambda_dist)
    v.out_loss3, v.out_reg2 = loss5.data_ptr(), loss5[3:].data_ptr()
    v.reg_workspace, v.reg_workspace_bytes = rws.data_ptr(), rws_bytes
    terms = None
    if _any_term(depth_sensor, depth_est, lambda_depth_sensor, weight_depth_est, weight_depth_normal, lambda_isotropic):
        terms, keep, depth = _view_terms2d(L, c, depth_sensor, depth_est, lambda_depth_sensor, weight_depth_est,
                                           weight_depth_normal, lambda_isotropic)
        _C.check(L.scorp_gs2d_train_view_ex(ctypes.byref(v), ctypes.byref(terms), _stream()), "scorp_gs2d_train_view_ex")
    else:
        _C.check(L.scorp_gs2d_train_view(ctypes.byref(v), _stream()), "scorp_gs2d_train_view")
    header = PairPolicy.pend(c.state, N, H, W)
    c.accumulate()
    extra, total = {}, loss5[0] + loss5[3] + loss5[4]
    if terms is not None:
        t6 = keep[0]
        extra = {"photometric_loss": loss5[0], "depth_sensor_loss": t6[1], "depth_est_loss": t6[2], "depth_normal_loss": t6[3],
                 "render_normal_loss": t6[4], "isotropic_loss": t6[5], "render_depth": depth}
        total = total + t6[0]
    return c.result(loss5, total, header, allmap=allmap, visibility_filter=c.radii > 0, normal_loss=loss5[3], dist_loss=loss5[4], **extra)


def _view_terms2d(L, c, depth_sensor, depth_est, lambda_depth_sensor, weight_depth_est, weight_depth_normal, lambda_isotropic):
    """The ScorpGs2dViewTerms of one view, the tensors it points to (out_terms6 first) and the surface-depth map (or None)."""
    H, W, N = c.H, c.W, c.N
    maps = _depth_maps(c, depth_sensor, depth_est)
    ws_bytes = L.scorp_gs2d_view_terms_workspace_bytes(W, H, N)
    keep = [c.new((6,)), c.new((ws_bytes,), torch.uint8), *maps]
    t = _C.ScorpGs2dViewTerms()
    t.depth_sensor, t.depth_est = (None if m is None else m.data_ptr() for m in maps)
    t.lambda_depth_sensor, t.weight_depth_est = float(lambda_depth_sensor), float(weight_depth_est)
    t.weight_depth_normal, t.lambda_isotropic = float(weight_depth_normal), float(lambda_isotropic)
    t.out_terms6, t.workspace, t.workspace_bytes = keep[0].data_ptr(), keep[1].data_ptr(), ws_bytes
    depth = None
    if maps[0] is not None or maps[1] is not None:
        depth = c.new((1, H, W))
        keep += [depth, c.new((H, W))]
        t.out_depth, t.grad_depth = depth.data_ptr(), keep[-1].data_ptr()
        if weight_depth_normal:
            keep.append(c.new((3, H, W)))
            t.grad_normal = keep[-1].data_ptr()
    return t, keep, depth
