"""3-D segmentation by 2-D object masks: utils/mask.py's get_mask3d / apply_mask3d and the file layout of
segmentation_3dgs.py / segmentation_2dgs.py, for both model kinds.

The reference votes with 1 + 2K full backward passes per camera on a render with colors_precomp = ones (K = prompts) and
reads only |dL/dcolor| of each Gaussian: for the loss mean(render * mask) that norm is S_in / (sqrt(3) H W), S_in being the
blend weight alpha * T the Gaussian put inside the mask (S_out: outside it).  Here one render per camera (the same
preprocess + render as `render(..., override_color=ones)`) is followed by ONE pass of the mask-vote kernel
(scorp_gs3d_mask_vote / scorp_gs2d_mask_vote), which gives S_in and S_out of every object and Gaussian and adds the vote:
    "gradient"  vote[k, i] += (S_in - S_out) / (sqrt(3) H W)      (utils/mask.py:66-70,90-91)
    "binary"    vote[k, i] += [S_in > 0] - [S_out > 0]            (:72-73,92-93)
    "sums"      sums[k, 0, i] += S_in, sums[k, 1, i] += S_out     (the raw sums; not a reference method)
The kernel uses no float atomics, so the votes - whose signs decide the segmentation - are the same bits on every run.
"""
import ctypes
import math
import os

import numpy as np
import torch

from . import _C
from .rasterizer3d import _GS2D, _GS3D, _camera_settings, _inputs_struct, _prep, _preprocess, _ptr, _stream

METHODS = {"sums": _C.VOTE_SUMS, "gradient": _C.VOTE_GRADIENT, "binary": _C.VOTE_BINARY}


def method_code(method):
    """The C ABI's method number of a voting method name."""
    if method == "projection":
        raise ValueError('voting method "projection" is not supported: it reads meta["means2d"], and the reference sets '
                         "meta = None before that branch (utils/mask.py:50,74-82), so it cannot run there either")
    if method not in METHODS:
        raise ValueError(f"unknown voting method {method!r}: expected one of {sorted(METHODS)}")
    return METHODS[method]


def vote_scale(method, H, W):
    """The factor of the "gradient" vote: the channel norm of dL/dcolors_precomp = S / (3 H W) per channel."""
    return 1.0 / (math.sqrt(3.0) * H * W) if method == "gradient" else 1.0


def _model_kind(gaussians):
    from .renderer2d import GaussianModel2D
    from .gaussian_model import GaussianModel
    if isinstance(gaussians, GaussianModel2D):
        return _GS2D
    if isinstance(gaussians, GaussianModel):
        return _GS3D
    raise TypeError(f"expected a GaussianModel or a GaussianModel2D, got {type(gaussians).__name__}")


def prepare_masks(masks, H, W, device):
    """[K, H, W] masks (bool / integer / float tensor or array; nonzero = inside) as contiguous bytes on `device`."""
    m = torch.as_tensor(np.asarray(masks) if not isinstance(masks, torch.Tensor) else masks)
    if m.dim() != 3 or m.shape[0] < 1 or tuple(m.shape[1:]) != (int(H), int(W)):
        raise ValueError(f"masks must be [K, H, W] with K >= 1 at the camera's resolution (H={H}, W={W}); got {tuple(m.shape)}")
    return (m != 0).to(device=device, dtype=torch.uint8).contiguous()


def view_votes(kind, settings, means3D, opacities, masks, method="gradient", scales=None, rotations=None,
               cov3D_precomp=None, out=None):
    """One view from activated parameters: render with colors_precomp = ones (exact pair count: one host sync), then ADD the
    view's votes into `out` ([K, N], or [K, 2, N] for "sums"; allocated as zeros if None).  `kind` is _GS3D or _GS2D,
    `settings` a GaussianRasterizationSettings, `masks` [K, H, W] (prepare_masks).  Two host syncs per view: the pair
    count, and the vote's read of the state header (overflow check)."""
    code = method_code(method)
    if kind is not _GS3D and kind is not _GS2D:
        raise ValueError("kind must be rasterizer3d._GS3D or rasterizer3d._GS2D")
    fn = "scorp_gs2d_mask_vote" if kind is _GS2D else "scorp_gs3d_mask_vote"
    H, W = int(settings.image_height), int(settings.image_width)
    dev = means3D.device
    m = prepare_masks(masks, H, W, dev)
    K, N = m.shape[0], means3D.shape[0]
    shape = (K, 2, N) if code == _C.VOTE_SUMS else (K, N)
    if out is None:
        out = torch.zeros(shape, dtype=torch.float32, device=dev)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"out must be a contiguous float32 tensor of shape {shape} on {dev}")
    if N == 0:
        return out
    with torch.no_grad():
        keep = []
        t = [_prep(x, n) for x, n in ((means3D, "means3D"), (opacities, "opacities"), (scales, "scales"),
                                       (rotations, "rotations"), (cov3D_precomp, "cov3D_precomp"))]
        colors = torch.ones((N, 3), dtype=torch.float32, device=dev)
        args = _inputs_struct(settings, t[0], None, colors, t[1], t[2], t[3], t[4], keep)
        stream = _stream()
        L = _C.lib()
        # exact pair count (a host sync): a reservation could overflow and leave no votes for the view
        radii, state, pairs, capacity, _ = _preprocess(kind, args, N, H, W, dev, stream, True)
        color = torch.empty((3, H, W), dtype=torch.float32, device=dev)
        maps = [torch.empty((c, H, W), dtype=torch.float32, device=dev) for c in kind.maps]
        _C.check(getattr(L, kind.render)(ctypes.byref(args), _ptr(state), _ptr(pairs), capacity, _ptr(color),
                                         *map(_ptr, maps), stream), kind.render)
        scratch_bytes = L.scorp_mask_vote_scratch_bytes(N, W, H, capacity)
        scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
        _C.check(getattr(L, fn)(ctypes.byref(args), _ptr(state), _ptr(pairs), capacity, _ptr(m), K, code,
                                ctypes.c_float(vote_scale(method, H, W)), _ptr(out), _ptr(scratch), scratch_bytes, stream), fn)
    return out


def _masks_of(masks, i, camera):
    return masks(camera) if callable(masks) else masks[i]


def mask_votes(gaussians, cameras, masks, method="gradient", bg=None):
    """Votes of every Gaussian for every object over `cameras`: Tensor [K, N] ([K, 2, N] of (S_in, S_out) for "sums").
    `masks`: one [K, H, W] entry per camera (bool tensors / arrays at the camera's resolution, nonzero = inside), or a
    callable camera -> masks.  `bg` does not change a vote (default: black)."""
    kind = _model_kind(gaussians)
    method_code(method)
    cameras = list(cameras)
    if not callable(masks) and len(masks) != len(cameras):
        raise ValueError(f"{len(masks)} mask sets for {len(cameras)} cameras")
    xyz = gaussians.get_xyz
    dev = xyz.device
    if not xyz.is_cuda:
        raise RuntimeError("mask_votes needs the model on the GPU (scorp_amd has no CPU path)")
    if bg is None:
        bg = torch.zeros(3, dtype=torch.float32, device=dev)
    out = None
    with torch.no_grad():
        means3D, opac, scales, rots = xyz.detach(), gaussians.get_opacity, gaussians.get_scaling, gaussians.get_rotation
        for i, cam in enumerate(cameras):
            settings = _camera_settings(cam, bg, 1.0, gaussians.active_sh_degree)
            m = _masks_of(masks, i, cam)
            if out is not None and len(m) != out.shape[0]:
                raise ValueError(f"camera {i}: {len(m)} masks, the earlier cameras had {out.shape[0]}")
            out = view_votes(kind, settings, means3D, opac, m, method, scales=scales, rotations=rots, out=out)
    if out is None:
        raise ValueError("mask_votes needs at least one camera")
    return out


def get_mask3d(gaussians, cameras, masks, voting_method="gradient"):
    """utils/mask.py:get_mask3d: BoolTensor [K, N], Gaussian i belongs to object k iff its vote is positive (:124)."""
    if voting_method == "sums":
        raise ValueError('get_mask3d votes with "gradient" or "binary"')
    return mask_votes(gaussians, cameras, masks, voting_method) > 0


def _gather_rows(tensors, index):
    """The rows `index` (int32 on the GPU) of each float32 tensor, in one scorp_gather_rows launch."""
    outs = [torch.empty((index.numel(),) + tuple(t.shape[1:]), dtype=torch.float32, device=t.device) for t in tensors]
    # zero-width rows (_features_rest of an SH-0 model is [N, 0, 3]): nothing to copy, the output is already the right shape
    jobs = [(t.detach().float().contiguous(), d) for t, d in zip(tensors, outs) if d.numel() > 0]
    if not jobs:
        return outs
    arr = (_C.ScorpRowTensor * len(jobs))()
    for k, (s, d) in enumerate(jobs):
        arr[k].src, arr[k].dst = s.data_ptr(), d.data_ptr()
        arr[k].row_floats, arr[k].zero_if_fresh = int(s[0].numel()), 0
    _C.check(_C.lib().scorp_gather_rows(arr, len(jobs), ctypes.c_void_p(index.data_ptr()), index.numel(), _stream()),
             "scorp_gather_rows")
    return outs


def apply_mask3d(gaussians, mask3d, path, return_clone_gs=False):
    """segmentation_3dgs.py:apply_mask3d (and its 2DGS twin): a clone of the model holding the rows `mask3d` selects, with
    max_radii2D zeroed, written to `path` as a PLY; returns the clone if `return_clone_gs`."""
    import torch.nn as nn
    _model_kind(gaussians)
    xyz = gaussians.get_xyz
    mask3d = torch.as_tensor(mask3d, device=xyz.device)
    if mask3d.dtype != torch.bool or mask3d.shape != (xyz.shape[0],):
        raise ValueError(f"mask3d must be a bool tensor of shape ({xyz.shape[0]},); got {mask3d.dtype} {tuple(mask3d.shape)}")
    if not xyz.is_cuda:
        raise RuntimeError("apply_mask3d needs the model on the GPU (the row gather is a HIP kernel)")
    with torch.no_grad():
        index = mask3d.nonzero().reshape(-1).to(torch.int32)
        names = ("_xyz", "_features_dc", "_features_rest", "_scaling", "_rotation", "_opacity")
        rows = _gather_rows([getattr(gaussians, n) for n in names], index)
        clone = type(gaussians)(gaussians.max_sh_degree, device=gaussians.device)
        clone.active_sh_degree = gaussians.active_sh_degree
        for n, r in zip(names, rows):
            setattr(clone, n, nn.Parameter(r.requires_grad_(True)))
        clone.max_radii2D = torch.zeros(index.numel(), device=xyz.device)
    clone.save_ply(path)
    return clone if return_clone_gs else None


def segment(gaussians, cameras, masks, prompts, out_dir, voting_method="gradient"):
    """segmentation_3dgs.py:88-96 / segmentation_2dgs.py: <out_dir>/<prompt>.ply per object and <out_dir>/remained.ply of
    the Gaussians no object claimed.  Returns the [K, N] masks."""
    prompts = list(prompts)
    masks3d = get_mask3d(gaussians, cameras, masks, voting_method)
    if len(prompts) != masks3d.shape[0]:
        raise ValueError(f"{len(prompts)} prompts for {masks3d.shape[0]} masks per camera")
    os.makedirs(out_dir, exist_ok=True)
    for m, p in zip(masks3d, prompts):
        apply_mask3d(gaussians, m, os.path.join(out_dir, f"{p}.ply"))
    apply_mask3d(gaussians, masks3d.any(dim=0).logical_not(), os.path.join(out_dir, "remained.ply"))
    return masks3d


def load_prompt_masks(data_dir, prompts, image_name, resolution):
    """The reference's mask files (utils/mask.py:54-57): the alpha channel > 0 of
    <data_dir>/masked_image_rgba/<prompt>/<image_name>.png, one per prompt, as a bool tensor [K, H, W] at `resolution`
    = (W, H) (a mask of another size is resized with nearest neighbour)."""
    try:
        from PIL import Image
    except ImportError as e:
        raise ImportError("load_prompt_masks reads PNG files with Pillow, which is not installed") from e
    W, H = int(resolution[0]), int(resolution[1])
    root = os.path.join(data_dir, "masked_image_rgba")
    out = []
    for p in prompts:
        path = os.path.join(root, p, f"{image_name}.png")
        if not os.path.exists(path):
            raise FileNotFoundError(f"mask file {path} does not exist")
        with Image.open(path) as img:
            if "A" not in img.getbands():
                raise ValueError(f"{path} has no alpha channel (the mask is the alpha channel of an RGBA image)")
            a = img.getchannel("A")
            if a.size != (W, H):
                a = a.resize((W, H), Image.NEAREST)
            out.append(np.asarray(a) > 0)
    return torch.from_numpy(np.stack(out)) if out else torch.zeros((0, H, W), dtype=torch.bool)


def prompt_mask_source(data_dir, prompts):
    """A `masks` callable for mask_votes / get_mask3d / segment: each camera's masks from load_prompt_masks."""
    prompts = list(prompts)
    return lambda camera: load_prompt_masks(data_dir, prompts, camera.image_name, camera.resolution)
