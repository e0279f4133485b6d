"""The pose fit from matched 3-D point pairs on the GPU: the alignment scripts' pc_align_ransac (utils/solution.py:476-557,
called at align_3dgs_clpe_9dof.py:450) and adam_algorithm_3d3d_9dof (utils/solution.py:363-446, called at :437).

The reference runs 2 000 RANSAC iterations in a Python loop and 3 000 Adam steps of some 150 tiny torch kernels each.
Here every hypothesis of a RANSAC call is fitted and counted in one batch (scorp_pose_ransac) and all Adam steps run
inside one kernel launch on the float64 moments of the pairs (scorp_pose_adam_9dof); both in csrc/pose_fit.hip.  Swap
them in with one import:

    from scorp_amd.pose_fit import pc_align_ransac, adam_algorithm_3d3d_9dof
"""
import ctypes
from dataclasses import dataclass

import numpy as np
import torch

from . import _C
from ._points import _device

METHODS = {"umeyama": _C.POSE_UMEYAMA, "kabsch": _C.POSE_KABSCH}
MAX_HYPOTHESES = 65535
MAX_ADAM_ITERATIONS = 1_000_000


@dataclass
class RansacFit:
    """What scorp_pose_ransac returns: the fit over the winner's inliers (R [3, 3], t [3] float64, s), the winning
    hypothesis and its inlier count, every hypothesis's count [n_hyp] int32 and the winner's inlier mask [n] bool."""
    R: np.ndarray
    t: np.ndarray
    s: float
    winner: int
    count: int
    counts: np.ndarray
    mask: np.ndarray


def _pairs(source, target, device, through_fp32=False):
    out = []
    for name, a in (("source", source), ("target", target)):
        t = a.detach() if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
        if t.dim() != 2 or t.shape[1] != 3:
            raise ValueError(f"{name} points must be [n, 3]; got {tuple(t.shape)}")
        if through_fp32:
            t = t.to(torch.float32)
        out.append(t.to(device=device, dtype=torch.float64).contiguous())
    return out


def _workspace(L, n, n_hyp, device):
    ws = torch.empty(int(L.scorp_pose_fit_workspace_bytes(n, n_hyp)) + 256, dtype=torch.uint8, device=device)
    ptr = (ws.data_ptr() + 255) // 256 * 256
    return ws, ptr, ws.numel() - (ptr - ws.data_ptr())


def _run_ransac(P, Q, samples, threshold, min_inlier_ratio, method):
    """The kernel call: P, Q float64 [n, 3] and samples int32 [n_hyp, 3] on one device -> RansacFit."""
    dev = P.device
    n, nh = P.shape[0], samples.shape[0]
    L = _C.lib()
    R = torch.empty(9, dtype=torch.float64, device=dev)
    t = torch.empty(3, dtype=torch.float64, device=dev)
    s = torch.empty(1, dtype=torch.float64, device=dev)
    win = torch.empty(2, dtype=torch.int32, device=dev)
    counts = torch.empty(nh, dtype=torch.int32, device=dev)
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        ws, ws_ptr, ws_bytes = _workspace(L, n, nh, dev)
        code = L.scorp_pose_ransac(P.data_ptr(), Q.data_ptr(), n, samples.data_ptr(), nh, ctypes.c_double(threshold),
                                   ctypes.c_double(min_inlier_ratio), METHODS[method], R.data_ptr(), t.data_ptr(), s.data_ptr(),
                                   win.data_ptr(), counts.data_ptr(), mask.data_ptr(), ws_ptr, ws_bytes, _C.current_stream_ptr())
    if code == _C.ERR_NO_INLIERS:
        raise ValueError("No inliers found in RANSAC.")
    if code == _C.ERR_INVALID:
        raise ValueError(f"scorp_pose_ransac: {_C.lib().scorp_last_error().decode(errors='replace')}")
    _C.check(code, "scorp_pose_ransac")
    w = win.cpu().numpy()
    return RansacFit(R.cpu().numpy().reshape(3, 3), t.cpu().numpy(), float(s.cpu()[0]), int(w[0]), int(w[1]), counts.cpu().numpy(),
                     mask.cpu().numpy().astype(bool))


def ransac_fit(source, target, samples, threshold, min_inlier_ratio=-1.0, method="umeyama"):
    """Every hypothesis of `samples` ([n_hyp, 3] pair indices) fitted on its three pairs and counted over all pairs, the
    winner by the reference's rule (the first hypothesis with the highest count; with min_inlier_ratio > 0 the first whose
    count exceeds min_inlier_ratio * n, if any), its inlier mask and the fit over its inliers.  source / target [n, 3]:
    numpy arrays or torch tensors (used as float64).  Raises ValueError when the winner has fewer than 3 inliers."""
    if method == "umeyama_gen":
        raise NotImplementedError("method 'umeyama_gen' is not built (no caller uses it; on 3 pairs its inverse is singular)")
    if method not in METHODS:
        raise ValueError(f"method must be 'umeyama' or 'kabsch'; got {method!r}")
    if len(source) != len(target):
        raise ValueError("Source and target points must have the same length")
    if len(source) < 3:
        raise ValueError("At least 3 points are required to solve Umeyama.")
    threshold = float(threshold)
    if not np.isfinite(threshold):
        raise ValueError(f"threshold must be finite; got {threshold}")
    tri = samples.detach().cpu().numpy() if isinstance(samples, torch.Tensor) else np.asarray(samples)
    if tri.ndim != 2 or tri.shape[1] != 3 or not 1 <= tri.shape[0] <= MAX_HYPOTHESES:
        raise ValueError(f"samples must be [n_hyp, 3] with 1 <= n_hyp <= {MAX_HYPOTHESES}; got {tri.shape}")
    if not np.issubdtype(tri.dtype, np.integer) or tri.min() < 0 or tri.max() >= len(source):
        raise ValueError(f"samples must be integer pair indices in [0, {len(source)})")
    dev = _device(source, target)
    P, Q = _pairs(source, target, dev)
    tri = torch.as_tensor(np.ascontiguousarray(tri, dtype=np.int32), device=dev)
    return _run_ransac(P, Q, tri, threshold, float(min_inlier_ratio), method)


def _draw_triples(n, count):
    """One np.random.choice(n, 3, replace=False) per iteration on numpy's global generator, as the reference draws."""
    out = np.empty((count, 3), dtype=np.int32)
    for i in range(count):
        out[i] = np.random.choice(n, 3, replace=False)
    return out


def pc_align_ransac(source_points, target_points, threshold=0.5, max_iterations=2000, min_inlier_ratio=-1.0, method="umeyama"):
    """The reference's function of the same name: (R [3, 3], t [3], s) of target ~ s R source + t by RANSAC over 3-pair
    hypotheses, then the same fit over the best inlier set.  The triples come from numpy's global generator exactly as
    the reference draws them, and the generator is left where the reference's loop leaves it (after an early exit at
    iteration i: i + 1 draws), so np.random.seed(k) picks the same hypotheses in both."""
    if len(source_points) != len(target_points):
        raise ValueError("Source and target points must have the same length")
    if len(source_points) < 3:
        raise ValueError("At least 3 points are required to solve Umeyama.")
    if method == "umeyama_gen":
        raise NotImplementedError("method 'umeyama_gen' is not built (no caller uses it; on 3 pairs its inverse is singular)")
    if method not in METHODS:
        raise ValueError(f"method must be 'umeyama' or 'kabsch'; got {method!r}")
    max_iterations = int(max_iterations)
    if max_iterations > MAX_HYPOTHESES:
        raise ValueError(f"max_iterations above {MAX_HYPOTHESES} is not supported")
    if max_iterations < 1:
        raise ValueError("No inliers found in RANSAC.")
    n = len(source_points)
    state = np.random.get_state()
    samples = _draw_triples(n, max_iterations)
    fit = ransac_fit(source_points, target_points, samples, threshold, min_inlier_ratio, method)
    if min_inlier_ratio > 0 and fit.count > min_inlier_ratio * n and fit.winner + 1 < max_iterations:
        np.random.set_state(state)
        _draw_triples(n, fit.winner + 1)
    return fit.R, fit.t, (fit.s if method == "umeyama" else 1.0)


def _start_scale(init_scale, scale_min, scale_max):
    """The reference's init_scale rule (utils/solution.py:379-388)."""
    if isinstance(init_scale, float):
        init_scale = np.array(3 * [init_scale])
    elif isinstance(init_scale, (list, tuple)):
        init_scale = np.array(init_scale)
    if not isinstance(init_scale, np.ndarray) or init_scale.shape != (3,):
        raise ValueError("`init_scale` must be a float, list, or tuple of length 3.")
    if init_scale.min() < scale_min or init_scale.max() > scale_max:
        init_scale = np.array(3 * [scale_min + (scale_max - scale_min) / 2])
    return init_scale.astype(np.float64)


def _run_adam(P, Q, iterations, lr, lambda_reg_scale, lambda_reg_rot, scale_min, scale_max, init_scale, loss_every):
    """The kernel call: P, Q float64 [n, 3] on one device, init_scale float64 [3] (host) -> dict of float64 numpy arrays
    (rotation, translation, scale, rotation_orthogonal, loss, losses)."""
    dev = P.device
    L = _C.lib()
    out = torch.empty(25, dtype=torch.float64, device=dev)
    n_loss = iterations // loss_every if loss_every > 0 else 0
    losses = torch.empty(max(n_loss, 1), dtype=torch.float64, device=dev)
    s0 = (ctypes.c_double * 3)(*[float(v) for v in init_scale])
    f64 = ctypes.c_double
    with torch.cuda.device(dev):
        ws, ws_ptr, ws_bytes = _workspace(L, P.shape[0], 1, dev)
        code = L.scorp_pose_adam_9dof(P.data_ptr(), Q.data_ptr(), P.shape[0], iterations, f64(lr), f64(lambda_reg_scale),
                                      f64(lambda_reg_rot), f64(scale_min), f64(scale_max), s0, out.data_ptr(),
                                      losses.data_ptr() if n_loss else None, loss_every if n_loss else 0, n_loss, ws_ptr, ws_bytes,
                                      _C.current_stream_ptr())
    if code == _C.ERR_INVALID:
        raise ValueError(f"scorp_pose_adam_9dof: {_C.lib().scorp_last_error().decode(errors='replace')}")
    _C.check(code, "scorp_pose_adam_9dof")
    o = out.cpu().numpy()
    return {"rotation": o[0:9].reshape(3, 3).copy(), "translation": o[9:12].copy(), "scale": o[12:15].copy(),
            "rotation_orthogonal": o[15:24].reshape(3, 3).copy(), "loss": float(o[24]), "losses": losses.cpu().numpy()[:n_loss]}


def adam_fit_9dof(source_points, target_points, iterations=1000, lr=1e-3, lambda_reg_scale=2e-5, lambda_reg_rot=1e-4, scale_max=1.5,
                  scale_min=0.75, init_scale=1.0, loss_every=0, device="cuda"):
    """adam_algorithm_3d3d_9dof's computation with float64 results: dict(rotation, translation, scale, rotation_orthogonal,
    loss, losses[iterations // loss_every]).  The points are rounded to fp32 first, as the reference rounds them."""
    if len(source_points) != len(target_points):
        raise ValueError("Source and target points must have the same length")
    if len(source_points) < 3:
        raise ValueError("At least 3 point pairs are required")
    iterations = int(iterations)
    if not 0 <= iterations <= MAX_ADAM_ITERATIONS:
        raise ValueError(f"iterations must be in [0, {MAX_ADAM_ITERATIONS}]; got {iterations}")
    s0 = _start_scale(init_scale, scale_min, scale_max)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"scorp_amd.pose_fit runs on the GPU only; got device={device!r}")
    if dev.index is None:
        dev = _device(source_points, target_points)
    P, Q = _pairs(source_points, target_points, dev, through_fp32=True)
    return _run_adam(P, Q, iterations, float(lr), float(lambda_reg_scale), float(lambda_reg_rot), float(scale_min), float(scale_max),
                     s0, int(loss_every))


def adam_algorithm_3d3d_9dof(source_points, target_points, iterations=1000, verbose_interval=100, lr=1e-3, lambda_reg_scale=2e-5,
                             lambda_reg_rot=1e-4, scale_max=1.5, scale_min=0.75, init_scale=1.0, device="cuda"):
    """The reference's function of the same name: (rotation [3, 3], translation [3], scale [3], rotation_orthogonal [3, 3])
    as float32 numpy arrays, target ~ R Ro^T diag(s) Ro source + t.  With verbose_interval > 0 the loss of every
    verbose_interval-th step is printed after the run (all steps are one kernel launch)."""
    every = int(verbose_interval) if verbose_interval and verbose_interval > 0 else 0
    res = adam_fit_9dof(source_points, target_points, iterations, lr, lambda_reg_scale, lambda_reg_rot, scale_max, scale_min,
                        init_scale, every, device)
    for k, loss in enumerate(res["losses"]):
        print(f"Iteration {(k + 1) * every:4d} | Loss: {loss:.6f}")
    return tuple(res[k].astype(np.float32) for k in ("rotation", "translation", "scale", "rotation_orthogonal"))
