"""Stacked views and the scoring render of the 2DGS path: argument checks through the C ABI and the choice of the kind in
the Python layer.  Validation runs before any HIP call, so the dummy pointers are never dereferenced: no GPU needed."""
import ctypes
import math
import types

import pytest
import torch

DUMMY = 0x10000   # non-zero, 256-byte aligned
INVALID = -1      # SCORP_ERR_INVALID


@pytest.fixture(scope="module")
def L():
    from scorp_amd import _C, build
    build.build()
    return _C.lib()


def inputs(**kw):
    from scorp_amd import _C
    inp = _C.ScorpGs3dInputs(num_gaussians=1, sh_degree=0, sh_coeffs=1, image_width=64, image_height=96, tanfovx=1.0,
                             tanfovy=1.0, scale_modifier=1.0, bg=DUMMY, viewmatrix=DUMMY, projmatrix=DUMMY, campos=DUMMY,
                             means3D=DUMMY, shs=DUMMY, opacities=DUMMY, scales=DUMMY, rotations=DUMMY)
    for k, v in kw.items():
        setattr(inp, k, v)
    return inp


def preprocess(L, inp):
    return L.scorp_gs2d_preprocess(ctypes.byref(inp), DUMMY, DUMMY, 0, None)   # (state_bytes 0: never past the state check)


def score(L, inp, tgt_depth=DUMMY, tgt_alpha=DUMMY, rows=96, depth_ratio=1.0, acc=DUMMY):
    return L.scorp_gs2d_render_score(ctypes.byref(inp), DUMMY, DUMMY, 1024, tgt_depth, tgt_alpha, rows, depth_ratio, 1.0, acc, None)


def refused(L, rc, *reasons):
    assert rc == INVALID
    msg = L.scorp_last_error()
    assert any(r in msg for r in reasons), msg


def test_render_score_is_exported_and_declared(L):
    from scorp_amd import _C
    assert "scorp_gs2d_render_score" in _C.EXPORTS and hasattr(L, "scorp_gs2d_render_score")
    assert len(L.scorp_gs2d_render_score.argtypes) == 11


def test_preprocess_reads_num_views(L):
    refused(L, preprocess(L, inputs(num_views=-1)), b"negative")
    refused(L, preprocess(L, inputs(num_views=2, image_height=100)), b"multiple of 16")
    refused(L, preprocess(L, inputs(num_views=2, scales=None, rotations=None, cov3D_precomp=DUMMY)), b"cov3D_precomp")
    refused(L, preprocess(L, inputs(num_views=2, num_gaussians=1 << 30)), b"too large")
    refused(L, preprocess(L, inputs(num_views=2, image_height=16 * 40000)), b"too large")
    # a stacked image that is accepted gets as far as the state check (state_bytes = 0 here) - and so does one view with
    # a given transform, which stays legal
    refused(L, preprocess(L, inputs(num_views=2)), b"state buffer")
    refused(L, preprocess(L, inputs(num_views=1, scales=None, rotations=None, cov3D_precomp=DUMMY)), b"state buffer")


def test_render_and_backward_are_forward_only(L):
    from scorp_amd import _C
    inp = inputs(num_views=2)
    refused(L, L.scorp_gs2d_render(ctypes.byref(inp), DUMMY, DUMMY, 1024, DUMMY, DUMMY, None), b"forward only")
    grads = _C.ScorpGs3dGrads()
    refused(L, L.scorp_gs2d_backward(ctypes.byref(inp), DUMMY, DUMMY, 1024, DUMMY, DUMMY, ctypes.byref(grads), DUMMY, 1 << 20, None),
            b"forward only")
    refused(L, L.scorp_gs2d_backward_ex(ctypes.byref(inp), DUMMY, DUMMY, 1024, DUMMY, DUMMY, ctypes.byref(grads), DUMMY, 1 << 20, 0,
                                        None), b"forward only")
    # scorp_gs2d_render_image takes the stacked inputs: it gets past them, to its own output check
    refused(L, L.scorp_gs2d_render_image(ctypes.byref(inp), DUMMY, DUMMY, 1024, None, None, None), b"output image pointer")
    # the one-call training view refuses them before its preprocess (which would write num_views x N radii)
    view = _C.ScorpGs2dTrainView(inputs=ctypes.addressof(inp), out_radii=DUMMY, state=DUMMY, state_bytes=1 << 30, pairs=DUMMY,
                                 capacity=1024, out_color=DUMMY, out_allmap=DUMMY, gt=DUMMY, out_loss3=DUMMY, out_reg2=DUMMY,
                                 grad_color=DUMMY, grads=ctypes.addressof(grads))
    refused(L, L.scorp_gs2d_train_view(ctypes.byref(view), None), b"forward only")


def test_render_score_argument_errors(L):
    one, two = inputs(), inputs(num_views=2)    # 96 rows; 192 stacked rows
    refused(L, score(L, one, tgt_depth=None), b"targets")
    refused(L, score(L, one, tgt_alpha=None), b"targets")
    refused(L, score(L, one, acc=None), b"targets")
    refused(L, score(L, one, rows=40), b"multiple of 16")          # not a multiple of 16
    refused(L, score(L, two, rows=80, ), b"multiple of 16")        # a multiple of 16 that does not divide the 192 rows
    refused(L, score(L, two, rows=0), b"multiple of 16")
    refused(L, score(L, one, depth_ratio=1.5), b"depth_ratio")
    refused(L, score(L, one, depth_ratio=-0.25), b"depth_ratio")
    refused(L, score(L, one, depth_ratio=float("nan")), b"depth_ratio")
    refused(L, score(L, one, depth_ratio=math.inf), b"depth_ratio")
    refused(L, score(L, inputs(num_views=-1)), b"negative")
    refused(L, score(L, inputs(num_views=2, image_height=100), rows=100), b"multiple of 16")
    refused(L, L.scorp_gs2d_render_score(ctypes.byref(one), None, DUMMY, 1024, DUMMY, DUMMY, 96, 1.0, 1.0, DUMMY, None), b"state")


# ---- the Python layer picks the kind from the model ----

def standin(cls, sh_degree=0, on_gpu=False):
    """A model of class `cls` with a handful of CPU rows; `on_gpu`: its position tensor claims to live on the GPU (what
    align._stacked_ok asks before anything is launched)."""
    from scorp_amd.synthetic import make_gaussians
    from scorp_amd.renderer2d import GaussianModel2D
    m = cls.from_raw(make_gaussians(8, sh_degree, 1, scale_dims=2 if cls is GaussianModel2D else 3), sh_degree, device="cpu")
    if on_gpu:
        m._xyz = types.SimpleNamespace(is_cuda=True)
    return m


def test_multiview_picks_the_kind_from_the_model():
    from scorp_amd import multiview
    from scorp_amd.gaussian_model import GaussianModel
    from scorp_amd.renderer2d import GaussianModel2D
    from scorp_amd.synthetic import ring_cameras
    stack = multiview.ViewStack(ring_cameras(2, 32, 32, 0))
    bg = torch.zeros(3)
    # (no CPU path: the refusal names the entry point the model's kind would have gone to)
    with pytest.raises(RuntimeError, match="scorp_gs2d_render_image"):
        multiview.render_stacked(standin(GaussianModel2D), stack, bg)
    with pytest.raises(RuntimeError, match="scorp_gs3d_render_image"):
        multiview.render_stacked(standin(GaussianModel), stack, bg)
    with pytest.raises(TypeError, match="GaussianModel"):
        multiview.render_stacked(types.SimpleNamespace(get_xyz=torch.zeros(1, 3)), stack, bg)


def test_surfel_alpha_depth_is_the_renderers_expression():
    from scorp_amd.multiview import surfel_alpha_depth
    allmap = torch.zeros(7, 2, 3)
    allmap[0], allmap[1], allmap[5] = 3.0, 0.5, 4.0
    allmap[1, 0, 0] = 0.0                 # empty pixel: 3 / 0 = inf -> 0
    allmap[0, 0, 1] = 0.0
    allmap[1, 0, 1] = 0.0                 # 0 / 0 = nan -> 0
    allmap[5, 1, 2] = float("nan")
    for r in (0.0, 0.25, 1.0):
        alpha, depth = surfel_alpha_depth(allmap, r)
        assert torch.equal(alpha, allmap[1])
        e = torch.full((2, 3), 6.0)
        e[0, 0] = e[0, 1] = 0.0
        m = torch.full((2, 3), 4.0)
        m[1, 2] = 0.0
        assert torch.equal(depth, e * (1 - r) + r * m)


def test_stacked_ok_and_the_default_renderer_follow_the_kind():
    from scorp_amd import align, renderer, renderer2d
    from scorp_amd.gaussian_model import GaussianModel
    from scorp_amd.renderer2d import GaussianModel2D
    from scorp_amd.synthetic import ring_cameras
    cams = ring_cameras(3, 64, 48, 0)
    surfels, gaussians = standin(GaussianModel2D, on_gpu=True), standin(GaussianModel, on_gpu=True)
    assert align._stacked_ok(surfels, cams, renderer2d.render)
    assert align._stacked_ok(gaussians, cams, renderer.render)
    assert not align._stacked_ok(surfels, cams, renderer.render)        # the 3DGS renderer cannot draw surfels
    assert not align._stacked_ok(gaussians, cams, renderer2d.render)
    assert not align._stacked_ok(surfels, cams, lambda *a: renderer2d.render(*a))   # a stand-in renderer: nothing to stack
    assert not align._stacked_ok(standin(GaussianModel2D, 1, on_gpu=True), cams, renderer2d.render)   # view-dependent colour
    assert not align._stacked_ok(standin(GaussianModel2D), cams, renderer2d.render)                   # not on the GPU
    assert not align._stacked_ok(surfels, ring_cameras(3, 64, 40, 0), renderer2d.render)              # height % 16
    assert not align._stacked_ok(surfels, cams[:2] + ring_cameras(1, 32, 48, 0), renderer2d.render)   # two resolutions
    # a caller that leaves the renderer at its default hands over a surfel model without choosing anything
    assert align._render_of(surfels, renderer.render) is renderer2d.render
    assert align._render_of(gaussians, renderer.render) is renderer.render
    mine = lambda *a: None
    assert align._render_of(surfels, mine) is mine
    assert align.DEPTH_RATIO == 1.0   # the reference's PipelineParams.depth_ratio
