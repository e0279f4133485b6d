"""The blend backward's per-chunk tail at the edges of its structure, against the float64 oracle.

A wave replays its block's hits 64 at a time (a chunk), 16 at a time through the matrix phase (a group).  The groups leave
each hit's block-frame moments in the hit's own staging entries; ONE pass per chunk (lane = hit) turns them into the ten
screen-space gradients, and the chunk's rows are sent off while the next chunk is being staged (after the loop for the
last one).  What can go wrong sits at the boundaries: a partial last group, a chunk that is exactly full, the flush of
chunk 0 next to the staging of chunk 1, staging entries used a second and a third time.

Scenes: n large, faint splats (scale ~3, every opacity 0.03) in front of a small image, so that every splat is a hit of
every block and no pixel saturates: a block's replay length is about n (asserted on the 8x8 image, whose single block
with pixels is all that `scorp_gs3d_debug_work` counts).  All four forms of the reduction, with and without depth /
alpha upstream gradients, the colour-only replay, the deterministic rows' repeatability, and the atomic form against
the deterministic form of the same precision (summation order only: the 2e-5 relative L1 of DESIGN.md section 2)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests.util import assert_no_further_from_f64, grad_errors, image_weights, make_case

pytestmark = pytest.mark.gpu

# hit count -> the replay length the case is there for
HITS = {16: 16, 31: 31, 33: 33, 48: 48, 63: 63, 64: 64, 66: 65, 128: 128, 130: 129}
SIZES = [(8, 8), (13, 11), (37, 21)]
MODES = ["exact_fp32", "exact_fp32_deterministic", "split", "deterministic"]
GRADS = ("means3D", "means2D", "opacities", "shs", "scales", "rotations")
FORMS_TOL = 2e-5

_scenes, _oracles, _hip = {}, {}, {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need a GPU"
    from scorp_amd import _C
    _C.lib()
    return torch.device("cuda:0")


def scene(n, size):
    if (n, size) not in _scenes:
        W, H = size
        kw, _ = make_case(N=n, W=W, H=H, deg=2, seed=30 + n, log_scale=math.log(3.0), log_scale_std=0.1, bg=(0.3, 0.1, 0.6))
        kw["opacities"] = np.full_like(kw["opacities"], 0.03)
        _scenes[n, size] = kw
    return _scenes[n, size]


def weights(n, size, depth_alpha):
    wc, wd, wa = image_weights(size[1], size[0], 30 + n)
    if not depth_alpha:
        wd, wa = np.zeros_like(wd), np.zeros_like(wa)
    return wc, wd, wa


def oracle_grads(n, size, depth_alpha):
    """(float32, float64) oracle gradients, computed once per scene and shared read-only."""
    key = (n, size, depth_alpha)
    if key not in _oracles:
        from oracle.gs_oracle import OracleRender
        kw, w = scene(n, size), weights(n, size, depth_alpha)
        both = []
        for dt in (np.float32, np.float64):
            g = OracleRender(dt, **kw).backward(*w)
            g = {k: np.asarray(g[k]) for k in GRADS}
            for a in g.values():
                a.setflags(write=False)
            both.append(g)
        _oracles[key] = tuple(both)
    return _oracles[key]


def run_hip(n, size, depth_alpha, mode, dev):
    from scorp_amd.rasterizer3d import backward_precision
    from scorp_amd.refcall import render3d_reference_call
    kw = scene(n, size)
    wc, wd, wa = weights(n, size, depth_alpha)
    with backward_precision(mode):
        out, t = render3d_reference_call(kw, dev, requires_grad=True)
    color, _, depth, alpha = out
    loss = (color * torch.tensor(wc, device=dev)).sum()
    if depth_alpha:
        loss = loss + (depth * torch.tensor(wd, device=dev)).sum() + (alpha * torch.tensor(wa, device=dev)).sum()
    loss.backward()
    g = {k: t[k].grad.detach().cpu().numpy() for k in GRADS}
    for a in g.values():
        a.setflags(write=False)
    return g


def hip_grads(n, size, depth_alpha, mode, dev):
    key = (n, size, depth_alpha, mode)
    if key not in _hip:
        _hip[key] = run_hip(n, size, depth_alpha, mode, dev)
    return _hip[key]


@pytest.mark.parametrize("n", list(HITS))
def test_replay_length_reaches_the_boundary(n, dev):
    """On the 8x8 image the one block with pixels replays at least the boundary's hits and at most n."""
    from scorp_amd import _C
    from scorp_amd import rasterizer3d as R
    from scorp_amd.refcall import render3d_reference_call
    R.KEEP_LAST_FORWARD = True
    try:
        render3d_reference_call(scene(n, (8, 8)), dev, requires_grad=True)
    finally:
        R.KEEP_LAST_FORWARD = False
    st, n_, w_, h_ = R.LAST_FORWARD
    o3 = (ctypes.c_uint64 * 3)()
    _C.check(_C.lib().scorp_gs3d_debug_work(st.data_ptr(), n_, w_, h_, ctypes.byref(o3), R._stream()), "scorp_gs3d_debug_work")
    R.LAST_FORWARD = None
    replay = int(o3[1])
    print(f"n = {n}: replay length {replay}")
    assert HITS[n] <= replay <= n, f"replay length {replay} outside [{HITS[n]}, {n}]"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("depth_alpha", [True, False])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("n", list(HITS))
def test_chunk_tail_against_f64(n, size, depth_alpha, mode, dev):
    got = hip_grads(n, size, depth_alpha, mode, dev)
    g32, g64 = oracle_grads(n, size, depth_alpha)
    for name in GRADS:
        assert np.abs(g64[name]).sum() > 0, f"{name}: the scene left nothing to compare"
        assert np.isfinite(got[name]).all(), f"{name}: non-finite gradient"
        assert_no_further_from_f64(name, got[name], g32[name], g64[name])


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_colour_only_chunk_tail_against_f64(size, dev):
    """Only the SH gradient is requested: the split form's colour-only replay, across a chunk boundary."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from scorp_amd.rasterizer3d import backward_precision
    from scorp_amd.refcall import _leaves, _settings
    n = 66
    kw = scene(n, size)
    wc, _, _ = weights(n, size, False)
    T, t, means2D = _leaves(kw, dev, False, ("means3D", "shs", "colors_precomp", "scales", "rotations", "cov3D_precomp"))
    t["shs"].requires_grad_(True)
    with backward_precision("split"):
        out = GaussianRasterizer(raster_settings=_settings(GaussianRasterizationSettings, kw, T, False))(
            means3D=t["means3D"], means2D=means2D, opacities=t["opacities"], shs=t["shs"], colors_precomp=t["colors_precomp"],
            scales=t["scales"], rotations=t["rotations"], cov3D_precomp=t["cov3D_precomp"])
    (out[0] * torch.tensor(wc, device=dev)).sum().backward()
    for name in ("means3D", "opacities", "scales", "rotations"):
        assert t[name].grad is None, name
    got = t["shs"].grad.detach().cpu().numpy()
    g32, g64 = oracle_grads(n, size, False)
    assert np.abs(g64["shs"]).sum() > 0 and np.isfinite(got).all()
    assert_no_further_from_f64("shs", got, g32["shs"], g64["shs"])


@pytest.mark.parametrize("mode", ["exact_fp32_deterministic", "deterministic"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("n", [66, 130])
def test_deterministic_rows_repeat(n, size, mode, dev):
    first = hip_grads(n, size, True, mode, dev)
    again = run_hip(n, size, True, mode, dev)
    for name in GRADS:
        assert np.array_equal(first[name], again[name]), f"{name}: two runs of the {mode} form differ"


@pytest.mark.parametrize("forms", [("exact_fp32", "exact_fp32_deterministic"), ("split", "deterministic")], ids=lambda f: f[0])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("n", [64, 66, 130])
def test_atomic_form_equals_deterministic_form(n, size, forms, dev):
    atomic, det = (hip_grads(n, size, True, m, dev) for m in forms)
    for name in GRADS:
        e = grad_errors(atomic[name], det[name])[1]
        print(f"{forms[0]} n = {n} {size[0]}x{size[1]} {name}: relative L1 {e:.2e}")
        assert e <= FORMS_TOL, f"{name}: {forms[0]} vs {forms[1]} relative L1 {e:.3e} > {FORMS_TOL:g}"
