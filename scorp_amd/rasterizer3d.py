"""`diff_gaussian_rasterization`-compatible front-end over libscorp_gs.so.

Same names, argument meaning and error behaviour as the module the reference imports at
gs3dgs/gaussian_renderer/__init__.py:15 and calls at :51-66,101-111:
`GaussianRasterizationSettings` (12 fields) and `GaussianRasterizer(raster_settings)(means3D, means2D, shs,
colors_precomp, opacities, scales, rotations, cov3D_precomp) -> (color[3,H,W], radii[N] int32, depth[1,H,W],
alpha[1,H,W])`, differentiable w.r.t. all eight arguments.  PyTorch supplies device memory, the current
stream and autograd bookkeeping; every kernel is in the HIP library, reached through ctypes.
"""
import contextlib
import ctypes
import math
import threading
from typing import NamedTuple

import torch
import torch.nn as nn

from . import _C


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


class _Pending:
    """One forward issued without a host synchronisation: a copy of its 64-byte StateHeader (pair count, overflow flag),
    the event recorded behind that copy on the stream that produced it, the reservation context it belongs to and the
    number of Gaussians it rendered."""
    __slots__ = ("header", "event", "key", "n")

    def __init__(self, header, event, key, n=0):
        self.header, self.event, self.key, self.n = header, event, key, int(n)

    def numel(self):
        return self.header.numel()


class PairOverflow(RuntimeError):
    """Raised by PairPolicy.drain(): `count` pending views had overflowed their reserved pair buffer (each was discarded on
    the device: no optimizer step, no statistics)."""
    def __init__(self, msg, count):
        super().__init__(msg)
        self.count = int(count)


class PairPolicy:
    """How the (tile,splat) pair buffer is sized.

    "exact"   (default) one 8-byte D2H read per forward tells the exact pair count — what the CUDA original
              does too; always correct.
    "reserve" no host sync: the buffer is sized from the largest count seen so far IN THE SAME CONTEXT times `slack`;
              each forward is queued for `drain()`, which waits for the forward's own stream, raises if any view
              overflowed and grows that context's reservation.  For throughput loops that check once per N views.

    A context is (image height, image width, stream): the align loop changes resolution per render, `bench.py
    --streams` runs views on several streams — each gets its own reservation instead of one process-wide number.  What a
    context remembers is pairs PER GAUSSIAN at the model size it was learned on: when the model grows or shrinks
    (densify_and_prune, every 100 iterations) the reservation scales with it instead of starting again from a default
    (a scene that needs more than 4 pairs per Gaussian used to overflow after every densification).  `reserve` is only
    a caller-set FLOOR for every context (0 = none); `mode` / `slack` are configuration.  A context nobody has sized yet
    starts at max(4 N, 2^20) pairs.
    """
    mode = "exact"
    slack = 1.25
    reserve = 0          # pairs: floor applied to every context (callers that know their workload set it)
    _ctx = {}            # context key -> (reserved pairs, number of Gaussians they were learned on)
    _pending = []        # _Pending entries whose overflow flag has not been read yet
    _MAX_CTX = 64        # contexts kept (least recently learned dropped first)

    @classmethod
    def key(cls, N, H, W):
        return (int(H), int(W), _C.current_stream_ptr())

    @classmethod
    def capacity(cls, N, H, W):
        """Pairs to reserve for a forward of this context."""
        got, n0 = cls._ctx.get(cls.key(N, H, W), (0, 0))
        if got > 0 and n0 > 0 and int(N) != n0:
            got = cls._rescaled(got, n0, N, H, W)
        if got <= 0 and cls.reserve <= 0:
            got = max(4 * int(N), 1 << 20)
        return max(got, int(cls.reserve))

    @classmethod
    def _rescaled(cls, got, n0, N, H, W):
        """What a context learned on n0 Gaussians, for a model of N: the same pairs per Gaussian while the model is the SAME
        model resized (densify_and_prune: within 0.5x ... 2x); anything else is another scene that happens to share the
        resolution and the stream - a 10 k-Gaussian object that fills the screen (200 pairs per Gaussian, align's eager
        sweeps) says nothing about a multi-million-Gaussian scene - and starts from the default, as a context nobody has
        sized.  Never more than every Gaussian in every tile."""
        ratio = int(N) / n0
        if not 0.5 <= ratio <= 2.0:
            return 0
        tiles = ((int(W) + 15) // 16) * ((int(H) + 15) // 16)
        return min(max(int(got * ratio) + 1024, 1 << 16), max(tiles * int(N), 1 << 16))

    @classmethod
    def set_context(cls, N, H, W, pairs):
        """Seed / override the reservation of the current stream's (H, W) context (tests, callers that know their scene)."""
        cls._ctx[cls.key(N, H, W)] = (int(pairs), int(N))

    @classmethod
    def pend(cls, state, N, H, W, header=None):
        """Queue a forward for drain(): copies the header on the current stream and records an event behind the copy.
        `header`: a 64-byte tensor the library already filled with the first four header words (scorp_gs3d_train_view's
        out_header): then nothing is copied."""
        ev = None
        if header is not None:
            hdr = header
            if not torch.cuda.is_current_stream_capturing():
                ev = torch.cuda.Event()
                ev.record()
        elif torch.cuda.is_current_stream_capturing():
            # a captured replay is checked by its capturer (align.SweepPlan), which reads the live headers at the end of
            # the graph: a view of the state (kept alive by the graph's pool anyway) instead of a copy node per view
            hdr = state[:64]
        else:
            hdr = state[:64].clone()     # not the state itself, or every pending view would pin ~100 MB until the drain
            ev = torch.cuda.Event()
            ev.record()
        cls._pending.append(_Pending(hdr, ev, cls.key(N, H, W), N))
        return hdr

    @classmethod
    def drain(cls):
        """Verify every forward issued in "reserve" mode since the last drain (each on its own stream's event)."""
        pend, cls._pending = cls._pending, []
        worst, n_over = 0, 0
        err = None
        if not pend:
            return worst
        for p in pend:
            if p.event is not None:
                p.event.synchronize()     # the header was written on the stream that rendered the view
        # ONE device-to-host copy for all pending headers (first four words: pairs needed, overflow, capacity, -), per
        # device.  One scorp_gs3d_check_overflow per view was a copy and a stream synchronisation each - 32 of them per
        # drain, ~0.1 ms per training iteration of a 100k-Gaussian object.
        words = [None] * len(pend)
        by_dev = {}
        for i, p in enumerate(pend):
            by_dev.setdefault(p.header.device, []).append(i)
        for dev, idx in by_dev.items():
            rows = torch.stack([pend[i].header.reshape(-1).view(torch.uint8)[:16] for i in idx]).cpu().numpy().view("<u4")
            for i, r in zip(idx, rows):
                words[i] = r
        for p, w in zip(pend, words):
            n, overflow, capacity = int(w[0]), int(w[1]), int(w[2])
            worst = max(worst, n)
            if p.key is not None:
                need = int(n * cls.slack) + 1024
                got, n0 = cls._ctx.pop(p.key, (0, 0))
                if n0 > 0 and p.n > 0 and n0 != p.n:
                    got = int(got * (p.n / n0)) if 0.5 <= p.n / n0 <= 2.0 else 0   # what was learned, at this view's model size (_rescaled)
                cls._ctx[p.key] = (max(got, need), p.n if p.n > 0 else n0)   # (re-inserted last: most recently learned)
                while len(cls._ctx) > cls._MAX_CTX:
                    cls._ctx.pop(next(iter(cls._ctx)))
            if overflow:
                n_over += 1
                if err is None:
                    err = f"pair buffer overflow: {n} pairs needed, capacity {capacity}"
        if err:
            raise PairOverflow(f"pair reservation too small ({err}; {n_over} of {len(pend)} pending views); the context's "
                               "reservation has been grown, re-run the view(s)", n_over)
        return worst

    @classmethod
    def reset(cls):
        cls.mode, cls.reserve, cls._ctx, cls._pending = "exact", 0, {}, []


_tls = threading.local()
# SCORP_BACKWARD_DETERMINISTIC=1: every backward of this process runs the atomic-free form (include/scorp_gs.h)
_ENV_FLAGS = _C.BACKWARD_DETERMINISTIC if __import__("os").environ.get("SCORP_BACKWARD_DETERMINISTIC", "0") not in ("", "0") else 0


def _backward_flags():
    return int(getattr(_tls, "backward_flags", 0)) | _ENV_FLAGS


@contextlib.contextmanager
def backward_precision(mode):
    """Forwards issued inside `with backward_precision("exact_fp32"):` run their backward with fp32 MFMAs throughout
    (scorp_gs3d_backward_ex, SCORP_BACKWARD_EXACT_FP32) instead of the default two-term fp16 split of the pixel->splat
    reduction.  The choice is recorded per forward (thread-local while the block is active), so a backward that runs
    after the block still honours it.  Used by the parity tests to compare the two forms.
    "deterministic" / "exact_fp32_deterministic": the same reductions with the sums leaving as plain per-(block, hit) rows
    that a second kernel adds per Gaussian in a fixed order (SCORP_BACKWARD_DETERMINISTIC): no float atomics, two runs
    give the same bits - what a caller that votes on gradient SIGNS wants (utils/mask.py:52,65,89,124)."""
    assert mode in ("split", "exact_fp32", "deterministic", "exact_fp32_deterministic")
    prev = getattr(_tls, "backward_flags", 0)
    _tls.backward_flags = (_C.BACKWARD_EXACT_FP32 if mode.startswith("exact_fp32") else 0) | \
                          (_C.BACKWARD_DETERMINISTIC if mode.endswith("deterministic") else 0)
    try:
        yield
    finally:
        _tls.backward_flags = prev


KEEP_LAST_FORWARD = False   # diagnostics (bench.py): keep (state, N, W, H) of the most recent forward in LAST_FORWARD
LAST_FORWARD = None
LAST_NUM_PAIRS_LOG = []   # pair counts of the most recent "exact"-mode forwards (diagnostics / bench bookkeeping)


def _stream():
    return ctypes.c_void_p(_C.current_stream_ptr())


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _prep(t, name, shape_tail=None):
    """float32, contiguous, on the GPU; None stays None (maps to NULL in the C ABI)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a GPU tensor (scorp_amd has no CPU path)")
    if t.dtype != torch.float32:
        t = t.float()
    t = t.contiguous()
    if t.data_ptr() % 16:      # an offset view: the kernels fetch 16-byte words
        t = t.clone()
    return t


def _inputs_struct(s, means3D, sh, colors_precomp, opacities, scales, rotations, cov3D, keep, sh_rest=None, raw=0):
    """Fill the C struct; `keep` collects tensors that must outlive the call."""
    bg, vm, pm, cp = (_prep(s.bg, "bg"), _prep(s.viewmatrix, "viewmatrix"), _prep(s.projmatrix, "projmatrix"),
                      _prep(s.campos, "campos"))
    keep.extend([bg, vm, pm, cp])
    a = _C.ScorpGs3dInputs()
    a.num_gaussians = means3D.shape[0]
    a.sh_degree = int(s.sh_degree)
    a.sh_coeffs = 0 if sh is None else (sh.shape[1] if sh_rest is None else 1 + sh_rest.shape[1])
    a.shs_rest = None if sh_rest is None else sh_rest.data_ptr()
    a.raw_params = int(raw)
    a.image_width, a.image_height = int(s.image_width), int(s.image_height)
    a.tanfovx, a.tanfovy, a.scale_modifier = float(s.tanfovx), float(s.tanfovy), float(s.scale_modifier)
    a.prefiltered, a.debug = int(bool(s.prefiltered)), int(bool(s.debug))
    a.bg, a.viewmatrix, a.projmatrix, a.campos = bg.data_ptr(), vm.data_ptr(), pm.data_ptr(), cp.data_ptr()
    a.means3D = means3D.data_ptr()
    a.shs = None if sh is None else sh.data_ptr()
    a.colors_precomp = None if colors_precomp is None else colors_precomp.data_ptr()
    a.opacities = opacities.data_ptr()
    a.scales = None if scales is None else scales.data_ptr()
    a.rotations = None if rotations is None else rotations.data_ptr()
    a.cov3D_precomp = None if cov3D is None else cov3D.data_ptr()
    return a


class _Kind(NamedTuple):
    """What the 3DGS and the 2DGS rasterizer do differently; everything else about issuing a view is shared.  The entry
    points are names in libscorp_gs.so."""
    state_bytes: str
    preprocess: str
    render: str
    render_image: str               # the render that leaves no state for a backward pass
    backward_ex: str
    backward_scratch_bytes_ex: str
    maps: tuple                     # channels of the [c,H,W] maps after the colour, in the entry points' order
    grad_widths: dict               # columns of the [N, c] gradients (the others are shaped like their leaf)
    materialize_grads: bool         # False: outputs nobody used arrive in backward as None (the kernels skip those terms)
    flags_mask: int                 # backward flags the kind passes on
    keeps_last_forward: bool        # forwards set LAST_FORWARD under KEEP_LAST_FORWARD


def _grad_widths(**kind_widths):
    return {"means3D": 3, "colors_precomp": 3, "rotations": 4, **kind_widths}


_GS3D = _Kind("scorp_gs3d_state_bytes", "scorp_gs3d_preprocess", "scorp_gs3d_render", "scorp_gs3d_render_image",
              "scorp_gs3d_backward_ex", "scorp_gs3d_backward_scratch_bytes_ex", maps=(1, 1),   # depth, alpha
              grad_widths=_grad_widths(scales=3, cov3D_precomp=6), materialize_grads=False, flags_mask=~0,
              keeps_last_forward=True)
_GS2D = _Kind("scorp_gs2d_state_bytes", "scorp_gs2d_preprocess", "scorp_gs2d_render", "scorp_gs2d_render_image",
              "scorp_gs2d_backward_ex", "scorp_gs2d_backward_scratch_bytes_ex", maps=(7,),     # allmap
              grad_widths=_grad_widths(scales=2, cov3D_precomp=9), materialize_grads=True,
              flags_mask=~_C.BACKWARD_SCRATCH_ZEROED, keeps_last_forward=False)

# The leaves of the two autograd Functions in `apply` order, means2D (a gradient sink only) left out: the ScorpGs3dGrads
# field each gradient goes to.  The stock leaves are named by their fields, the raw ones by the model's leaves.
_STOCK_FIELDS = ("means3D", "shs", "colors_precomp", "opacities", "scales", "rotations", "cov3D_precomp")
_RAW_FIELDS = ("means3D", "shs", "shs_rest", "opacities", "scales", "rotations")
_RAW_NAMES = ("means3D", "features_dc", "features_rest", "opacity", "scaling", "rotation")


def _raw_inputs(settings, pc, keep):
    """A model's raw leaves as the library reads them: (the leaves xyz + pc.raw_leaves(), their prepped tensors, the
    ScorpGs3dInputs with raw_params = 7)."""
    leaves = (pc.get_xyz, *pc.raw_leaves())
    t = [_prep(x.detach(), n) for x, n in zip(leaves, _RAW_NAMES)]
    return leaves, t, _inputs_struct(settings, t[0], t[1], None, t[3], t[4], t[5], None, keep, t[2], 7)


def _camera_settings(camera, bg, scale_modifier, sh_degree, debug=False):
    """The rasterizer settings of one camera at its current resolution (gaussian_renderer/__init__.py:45-58)."""
    w, h = camera.resolution
    return GaussianRasterizationSettings(
        image_height=int(h), image_width=int(w), tanfovx=math.tan(camera.FoVx * 0.5),
        tanfovy=math.tan(camera.FoVy * 0.5), bg=bg, scale_modifier=scale_modifier,
        viewmatrix=camera.world_view_transform, projmatrix=camera.full_proj_transform, sh_degree=sh_degree,
        campos=camera.camera_center, prefiltered=False, debug=debug)


def _new_grads(kind, fields, t, want):
    """Gradient buffers of the prepped leaves `t` (ScorpGs3dGrads `fields`), None where not wanted: [N, width] for
    positions, colours, scales, rotations and covariances, the leaf's own shape for SH and opacity."""
    widths = kind.grad_widths
    g = []
    for f, x, w in zip(fields, t, want):
        g.append(None if not w or x is None else x.new_empty((x.shape[0], widths[f])) if f in widths else torch.empty_like(x))
    return g


def _grads_struct(fields, g, g_means2D):
    grads = _C.ScorpGs3dGrads()
    grads.means2D = _ptr(g_means2D)
    for f, x in zip(fields, g):
        setattr(grads, f, _ptr(x))
    return grads


def _preprocess(kind, args, N, H, W, dev, stream, exact, log=False):
    """Preprocess one launch set and size its pair buffer.  `exact`: from the pair count read back (8 bytes D2H);
    otherwise from PairPolicy's reservation, and the caller queues the view for drain() once it has rendered.  `log`:
    note the exact count in LAST_NUM_PAIRS_LOG.  Returns (radii, state, pairs, capacity, exact pair count or None)."""
    L = _C.lib()
    radii = torch.empty((N,), dtype=torch.int32, device=dev)
    state_bytes = getattr(L, kind.state_bytes)(N, W, H)
    state = torch.empty(state_bytes, dtype=torch.uint8, device=dev)
    _C.check(getattr(L, kind.preprocess)(ctypes.byref(args), _ptr(radii), _ptr(state), state_bytes, stream), kind.preprocess)
    num_pairs = None
    if exact:
        n = ctypes.c_uint64(0)
        _C.check(L.scorp_gs3d_num_pairs(_ptr(state), stream, ctypes.byref(n)), "scorp_gs3d_num_pairs")
        num_pairs = int(n.value)
        capacity = max(num_pairs, 1)
        if log:
            LAST_NUM_PAIRS_LOG.append(num_pairs)
            del LAST_NUM_PAIRS_LOG[:-64]
    else:
        capacity = PairPolicy.capacity(N, H, W)
    pairs = torch.empty(L.scorp_gs3d_pairs_bytes(capacity), dtype=torch.uint8, device=dev)
    return radii, state, pairs, capacity, num_pairs


def _forward(ctx, kind, raw, settings, leaves):
    """Forward of both autograd Functions: allocate outputs + workspaces, run preprocess / render, save for backward.
    Returns (color, radii, *maps)."""
    t = list(map(_prep, leaves, _RAW_NAMES if raw else _STOCK_FIELDS))
    keep = []
    if raw:   # activations fused into the kernels
        args = _inputs_struct(settings, t[0], t[1], None, t[3], t[4], t[5], None, keep, t[2], 7)
    else:
        args = _inputs_struct(settings, *t, keep)
    dev = t[0].device
    N, H, W = t[0].shape[0], int(settings.image_height), int(settings.image_width)
    stream = _stream()
    exact = PairPolicy.mode == "exact"
    # the outputs first: in "exact" mode _preprocess waits for the pair count, and what is left after it is on the
    # critical path
    color = torch.empty((3, H, W), dtype=torch.float32, device=dev)
    maps = []
    for c in kind.maps:
        maps.append(torch.empty((c, H, W), dtype=torch.float32, device=dev))
    radii, state, pairs, capacity, _ = _preprocess(kind, args, N, H, W, dev, stream, exact, log=True)
    # nothing to differentiate (the calls the reference makes under torch.no_grad()): the image-only render, which
    # leaves no state for a backward pass
    fn = kind.render if want_backward(ctx) else kind.render_image
    _C.check(getattr(_C.lib(), fn)(ctypes.byref(args), _ptr(state), _ptr(pairs), capacity, _ptr(color), *map(_ptr, maps),
                                   stream), fn)
    if not exact:
        PairPolicy.pend(state, N, H, W)   # what drain() will look at: a copy of the StateHeader the render just filled in
    if kind.keeps_last_forward and KEEP_LAST_FORWARD:
        global LAST_FORWARD
        LAST_FORWARD = (state, N, W, H)
    # the backward reuses `args`: every tensor it points into is saved below (None leaves stay None)
    ctx.kind, ctx.raw, ctx.args, ctx.size, ctx.capacity = kind, raw, args, (N, W, H), capacity
    # backward_precision(...) / SCORP_BACKWARD_DETERMINISTIC: fixed when the forward is issued
    ctx.backward_flags = _backward_flags() & kind.flags_mask
    ctx.set_materialize_grads(kind.materialize_grads)
    ctx.save_for_backward(*t, state, pairs, *keep)
    ctx.mark_non_differentiable(radii)
    return (color, radii, *maps)


def _backward(ctx, grad_color, grad_maps):
    """Backward of both autograd Functions: (the means2D gradient, the leaves' gradients in `apply` order)."""
    kind, raw, (N, W, H) = ctx.kind, ctx.raw, ctx.size
    fields = _RAW_FIELDS if raw else _STOCK_FIELDS
    n = len(fields)
    saved = ctx.saved_tensors   # (raises if a saved tensor was modified in place since the forward)
    t, state, pairs = saved[:n], saved[n], saved[n + 1]
    dev = state.device
    need = (ctx.needs_input_grad[0],) + ctx.needs_input_grad[2:1 + n]   # (means2D is [1])
    want = list(need)
    if raw:
        want[1] = want[2] = need[1] or need[2]   # the SH gradient is written as a whole
    g = _new_grads(kind, fields, t, want)
    g_means2D = torch.empty((N, 3), dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
    grads = _grads_struct(fields, g, g_means2D)
    if grad_color is None:
        grad_color = torch.zeros((3, H, W), dtype=torch.float32, device=dev)
    gc = _prep(grad_color, "grad_color")
    gm = []
    for x in grad_maps:
        gm.append(None if x is None else _prep(x, "grad"))
    L = _C.lib()
    scratch_bytes = getattr(L, kind.backward_scratch_bytes_ex)(N, W, H, ctx.capacity, ctx.backward_flags)
    scratch = torch.empty(scratch_bytes, dtype=torch.uint8, device=dev)
    _C.check(getattr(L, kind.backward_ex)(ctypes.byref(ctx.args), _ptr(state), _ptr(pairs), ctx.capacity, _ptr(gc),
                                          *map(_ptr, gm), ctypes.byref(grads), _ptr(scratch), scratch_bytes,
                                          ctx.backward_flags, _stream()),
             kind.backward_ex)
    if raw:   # only the SH gradients that were asked for
        g[1], g[2] = g[1] if need[1] else None, g[2] if need[2] else None
    return g_means2D, g


class _Rasterize(torch.autograd.Function):
    """The rasterizer of `kind` (_GS3D, _GS2D) on the stock inputs: (color, radii, *the kind's maps)."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3D_precomp, settings, kind):
        return _forward(ctx, kind, False, settings, (means3D, sh, colors_precomp, opacities, scales, rotations, cov3D_precomp))

    @staticmethod
    def backward(ctx, grad_color, grad_radii, *grad_maps):
        g_means2D, g = _backward(ctx, grad_color, grad_maps)
        return (g[0], g_means2D, *g[1:], None, None)


class _RasterizeRaw(torch.autograd.Function):
    """Same rasterizer on the GaussianModel's RAW storage (logit opacity, log scale, un-normalised quaternion,
    _features_dc / _features_rest kept apart): the activations of gaussian_model.py:126-146 and the SH concat run
    inside the per-Gaussian kernels, and the gradients come back w.r.t. the raw leaves."""

    @staticmethod
    def forward(ctx, means3D, means2D, f_dc, f_rest, opacity_raw, scaling_raw, rotation_raw, settings, kind):
        return _forward(ctx, kind, True, settings, (means3D, f_dc, f_rest, opacity_raw, scaling_raw, rotation_raw))

    @staticmethod
    def backward(ctx, grad_color, grad_radii, *grad_maps):
        g_means2D, g = _backward(ctx, grad_color, grad_maps)
        return (g[0], g_means2D, *g[1:], None, None)


def want_backward(ctx):
    """True if a backward pass can follow this forward.  `ctx.needs_input_grad` alone says yes for every leaf parameter
    even under torch.no_grad() (it ignores the grad mode, and inside Function.forward the mode is always off), so the
    wrappers below note the caller's grad mode before `apply`."""
    return bool(getattr(_tls, "grad_mode", True)) and any(ctx.needs_input_grad)


def rasterize_gaussians_raw(means3D, means2D, f_dc, f_rest, opacity_raw, scaling_raw, rotation_raw, raster_settings):
    _tls.grad_mode = torch.is_grad_enabled()
    return _RasterizeRaw.apply(means3D, means2D, f_dc, f_rest, opacity_raw, scaling_raw, rotation_raw, raster_settings, _GS3D)


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings):
    _tls.grad_mode = torch.is_grad_enabled()
    return _Rasterize.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                            raster_settings, _GS3D)


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions):
        """Frustum test of the upstream API (not called by the reference): view-space z > 0.2."""
        with torch.no_grad():
            vm = self.raster_settings.viewmatrix
            z = positions @ vm[:3, 2] + vm[3, 2]
            return z > 0.2

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None):
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception("Please provide excatly one of either SHs or precomputed colors!")
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                                   self.raster_settings)


class _RenderTail(torch.autograd.Function):
    """(render_depth, visibility_filter) from (depth, alpha, radii) in one launch: gaussian_renderer/__init__.py:113-120."""

    @staticmethod
    def forward(ctx, depth, alpha, radii):
        L = _C.lib()
        depth, alpha = _prep(depth, "depth"), _prep(alpha, "alpha")
        radii = radii.contiguous()
        out = torch.empty_like(depth)
        vis = torch.empty(radii.shape, dtype=torch.bool, device=radii.device)
        _C.check(L.scorp_gs3d_render_tail(_ptr(depth), _ptr(alpha), depth.numel(), _ptr(radii), radii.numel(), _ptr(out),
                                          _ptr(vis), _stream()), "scorp_gs3d_render_tail")
        ctx.save_for_backward(depth, alpha)
        ctx.mark_non_differentiable(vis)
        return out, vis

    @staticmethod
    def backward(ctx, g_out, _g_vis):
        L = _C.lib()
        depth, alpha = ctx.saved_tensors
        g_out = _prep(g_out, "grad")
        g_depth, g_alpha = torch.empty_like(depth), torch.empty_like(alpha)
        _C.check(L.scorp_gs3d_render_tail_backward(_ptr(g_out), _ptr(depth), _ptr(alpha), depth.numel(), _ptr(g_depth),
                                                   _ptr(g_alpha), _stream()), "scorp_gs3d_render_tail_backward")
        return g_depth, g_alpha, None


def render_tail(depth, alpha, radii):
    """render_depth = nan_to_num(depth / alpha, 0, 0) and visibility_filter = radii > 0, fused."""
    if not depth.is_cuda:
        raise RuntimeError("render_tail needs GPU tensors (scorp_amd has no CPU path)")
    return _RenderTail.apply(depth, alpha, radii.int())
