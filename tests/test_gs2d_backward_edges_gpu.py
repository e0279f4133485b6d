"""The 2DGS blend backward (blend2d_backward_wave_kernel, gs2d_backward.hip) at the edges of its structure, against the
float64 oracle.

A wave replays its block's hits 32 at a time (a chunk, k2BChunk) and sends them through the matrix pipe two at a time
(`pend`, flush_pair); an odd hit is flushed alone at the end of every chunk with the read-out lanes 32..51 silent
(`hh < pend`); a hit live on no pixel is skipped and shifts the pairing of every hit after it; the record fetch runs two
chunks ahead, so a third and a fourth chunk reuse registers and staging slots; the distortion recurrence (`last_dL_dT`)
is carried across chunks, the median depth is one selected hit (`pos1 == med_c`), and the split form's `Sh == 0` hits
take their 1 / p.z scale at replay time.  Eight instantiations: maps / no maps x split / exact x atomic / deterministic.

Scenes (tests/gs2d_edge_fixtures.py; tests/test_gs2d_backward_edges_cpu.py checks them in float64): n faint surfels
selected so that ALL n blend into pixel (3, 3) - its block replays exactly n hits, n = 1, 2, 3, 31, 32, 33, 63, 64, 65, 96,
97 - on 8x8, 13x11 and 37x21 images (partial blocks, blocks outside the image, shorter lists beside the anchor block), and
four variants (saturating, low-pass mix, horizon, uncovered pixels).  Gradients come through render2d_reference_call
under backward_precision(mode) and are held by tests.util.assert_no_further_from_f64 at its defaults; the colour-only
cases call scorp_gs2d_backward_ex with dL_dallmap = NULL (the autograd route materialises a zero map gradient, so it never
reaches the kHasMap = false instantiations).

Measured on an MI355X (for the record, not bars; 1 736 tensors), worst over the edge cases, variants and single channels,
per mode relL1(HIP, f64) | relL1(oracle32, f64) of the same tensor:
  split                     5.43e-05 | 4.32e-06   (n = 1, 37x21, all maps, scales)
  exact_fp32                2.80e-05 | 1.15e-05   (n = 1, 8x8, all maps, scales)
  deterministic             4.07e-05 | 4.32e-06   (n = 1, 37x21, all maps, scales)
  exact_fp32_deterministic  2.80e-05 | 1.15e-05   (n = 1, 8x8, all maps, scales)
The fp32 oracle's own worst is 3.49e-05 (n = 65, distortion alone, scales): the floor of 1e-4 governs every case.  One
tensor has no digits to compare: under the median channel alone the gradient to the scales is a cancellation residue (the
depth of a ray-plane intersection does not depend on the in-plane scales; float64 leaves 1e-9 of the fp32 residue) - there
the same assertion reads "the kernel's residue is at most 1.25 x the fp32 oracle's" (0.98 split, 1.11 exact).
Atomic vs deterministic rows, worst: 6.5e-07 relative L1 (exact_fp32, n = 97, 37x21, scales).  Split vs exact under
upstream gradients x 1e-6, x 1e4 and with one block's gradients zero, worst: 1.9e-06 relative L1, 2.2e-06 of max.
Pools: 600 (8x8), 6 000 (13x11), 48 000 (37x21) surfels drawn; 212, 1 082, 1 122 pass conditions (a) and (b); the 97 taken
end at candidate 97, 141 and 498 (the rest were refused by condition (c), see the fixtures).
The kernel passed as it stood; nothing in gs2d_backward.hip changed with this suite.

What the lengths catch (read off the kernel, and a control-flow model of the anchor block's replay): without the
`hh < pend` guard, the odd hit's flush reads matrix rows 8..15 out once more - the previous pair's second hit, still in
place, is added to its surfel a second time (n = 1: the prologue's scratch): every odd n misses in the two atomic modes,
by 1 / n of the hits (33: 3 %).  The deterministic rows are blind to it for n >= 3: the same row is rewritten with the same
value.  With the chunk-end flush dropped, the odd hit's sums never leave: every odd n misses in all four modes (n = 1: all
gradients zero).  Even n pass both in the anchor block; 13x11 and 37x21 have odd lists in their other blocks."""
import numpy as np
import pytest
import torch

from tests import gs2d_edge_fixtures as F
from tests.util import assert_no_further_from_f64, grad_errors

pytestmark = pytest.mark.gpu

MODES = ["split", "exact_fp32", "deterministic", "exact_fp32_deterministic"]
FORMS_TOL = 2e-5                     # atomic vs deterministic rows: summation order only
SPLIT_L1, SPLIT_MAX = 2e-5, 1e-4     # split vs exact (test_split_backward_equals_exact_fp32_backward_2d)
CHANNELS = ("depth", "alpha", "normal_x", "normal_y", "normal_z", "median", "distortion")
size_id = lambda s: f"{s[0]}x{s[1]}"

_hip = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need a GPU"
    from scorp_amd import _C
    _C.lib()
    return torch.device("cuda:0")


def run_hip(scene, wc, wa, mode, dev):
    """{leaf: gradient} of sum(color wc) + sum(allmap wa); wa = None: colour only, dL_dallmap = NULL at the C ABI."""
    from scorp_amd import rasterizer3d as R
    from scorp_amd.refcall import render2d_reference_call
    with R.backward_precision(mode):
        (color, _, allmap), t = render2d_reference_call(scene.kw, dev, requires_grad=True)
    if wa is not None:
        ((color * torch.tensor(wc, device=dev)).sum() + (allmap * torch.tensor(wa, device=dev)).sum()).backward()
        g = {k: t[k].grad for k in F.GRADS}
    else:
        ctx = color.grad_fn                  # the autograd context of the forward: state, pair buffer, recorded flags
        assert type(ctx).__name__ == "_RasterizeBackward" and ctx.kind.backward_ex == "scorp_gs2d_backward_ex"
        g_means2D, g = R._backward(ctx, torch.tensor(wc, device=dev), (None,))   # None -> NULL
        g = dict(zip(R._STOCK_FIELDS, g), means2D=g_means2D)
    g = {k: g[k].detach().cpu().numpy() for k in F.GRADS}
    for a in g.values():
        a.setflags(write=False)
    return g


def grads(scene, key, mode, dev, seed=7):
    """HIP and oracle gradients of a scene under the upstream gradients `key` ("all" | "colour"), cached."""
    wc, wa = F.upstream(scene.size, seed, maps=key == "all")
    k = (scene.name, key, mode)
    if k not in _hip:
        _hip[k] = run_hip(scene, wc, wa, mode, dev)
    return _hip[k], F.oracle_grads(scene, key, wc, wa)


def hold(tag, mode, got, g32, g64, nonzero=True):
    for name in F.GRADS:
        assert np.isfinite(got[name]).all(), f"{name}: non-finite gradient"
        if not np.abs(g64[name]).sum():
            assert not nonzero, f"{name}: the scene left nothing to compare"
            assert not np.abs(got[name]).sum(), f"{name}: the oracle's gradient is zero, the kernel's is not"
            continue
        e_hip, e_o32 = grad_errors(got[name], g64[name])[1], grad_errors(g32[name], g64[name])[1]
        print(f"EDGE {mode} {tag} {name}: relL1(HIP, f64) {e_hip:.3e} relL1(oracle32, f64) {e_o32:.3e}")
        assert_no_further_from_f64(name, got[name], g32[name], g64[name])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("key", ["all", "colour"])
@pytest.mark.parametrize("size", F.SIZES, ids=size_id)
@pytest.mark.parametrize("n", F.LENGTHS)
def test_chunk_and_pair_edges_against_f64(n, size, key, mode, dev):
    scene = F.edge_scene(n, size)
    got, (g32, g64) = grads(scene, key, mode, dev)
    hold(f"{scene.name} {key}", mode, got, g32, g64)


@pytest.mark.parametrize("mode", ["split", "exact_fp32"])
@pytest.mark.parametrize("channel", range(7), ids=CHANNELS)
def test_one_map_channel_at_a_time(channel, mode, dev):
    """n = 65 on 13x11 (three chunks: 32 + 32 + 1): one allmap channel alone carries the upstream gradient."""
    scene = F.edge_scene(65, (13, 11))
    wc, wa = F.upstream(scene.size, 11)
    wc[:] = 0.0
    wa[[c for c in range(7) if c != channel]] = 0.0
    got = run_hip(scene, wc, wa, mode, dev)
    g32, g64 = F.oracle_grads(scene, f"channel{channel}", wc, wa)
    assert all(np.abs(g64[name]).sum() > 0 for name in ("means3D", "rotations"))   # (the median gives opacity and scales none)
    hold(f"{scene.name} {CHANNELS[channel]}", mode, got, g32, g64, nonzero=False)   # (no colour gradient: shs is an exact zero)


VARIANTS = {"saturating": (F.saturating_scene, lambda s: s.check()), "lowpass": (F.lowpass_scene, F.check_lowpass),
            "horizon": (F.horizon_scene, F.check_horizon)}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_variants_against_f64(variant, mode, dev):
    build, check = VARIANTS[variant]
    scene = build()
    check(scene)
    got, (g32, g64) = grads(scene, "all", mode, dev)
    hold(scene.name, mode, got, g32, g64)


def _zero_block(w):
    w = w.copy()
    w[:, 0:8, 8:16] = 0.0
    return w


@pytest.mark.parametrize("scale,zero_block", [(1e-6, False), (1e4, False), (1.0, True)], ids=["x1e-6", "x1e4", "zero_block"])
@pytest.mark.parametrize("which", ["horizon", "n65"])
def test_wave_scale_split_against_exact(which, scale, zero_block, dev):
    """The split form's per-wave power of two under upstream gradients of 1e-6 and 1e4, and with every upstream gradient of
    ONE block zero (eb == 0: sv = 1) beside blocks that have some: split == exact within 2e-5 relative L1, 1e-4 of max."""
    scene = F.horizon_scene() if which == "horizon" else F.edge_scene(65, (13, 11))
    assert scene.size == (13, 11)
    wc, wa = F.upstream(scene.size, 13)
    wc, wa = wc * np.float32(scale), wa * np.float32(scale)
    if zero_block:                           # the block of pixels x = 8 .. 12, y = 0 .. 7
        wc, wa = _zero_block(wc), _zero_block(wa)
        assert not wc[:, :8, 8:].any() and not wa[:, :8, 8:].any() and wc[:, :8, :8].all() and wc[:, 8:, 8:].all()
    gs, ge = run_hip(scene, wc, wa, "split", dev), run_hip(scene, wc, wa, "exact_fp32", dev)
    for name in F.GRADS:
        assert np.isfinite(gs[name]).all() and np.abs(ge[name]).sum() > 0, name
        mx, l1 = grad_errors(gs[name], ge[name])
        print(f"SPLIT-EXACT {scene.name} {name}: rel L1 {l1:.2e}, max {mx:.2e}")
        assert l1 < SPLIT_L1 and mx < SPLIT_MAX, f"{name}: split vs exact rel L1 {l1:.2e}, max {mx:.2e}"


@pytest.mark.parametrize("mode", ["deterministic", "exact_fp32_deterministic"])
def test_nan_upstream_on_uncovered_pixels_is_dropped(mode, dev):
    """Pixels nothing was blended into (a whole block, and pixels scattered through blocks that have hits): NaN upstream
    gradients there give finite gradients, bit-equal to the run with zeros there."""
    scene = F.uncovered_scene()
    none = F.uncovered_mask(scene)
    wc, wa = F.upstream(scene.size, 17)
    wc0, wa0, wcn, wan = wc.copy(), wa.copy(), wc.copy(), wa.copy()
    wc0[:, none], wa0[:, none] = 0.0, 0.0
    wcn[:, none], wan[:, none] = np.nan, np.nan
    zeros, nans = run_hip(scene, wc0, wa0, mode, dev), run_hip(scene, wcn, wan, mode, dev)
    g32, g64 = F.oracle_grads(scene, "zeros_on_uncovered", wc0, wa0)
    hold(scene.name, mode, zeros, g32, g64)
    for name in F.GRADS:
        assert np.isfinite(nans[name]).all(), f"{name}: NaN upstream gradients on uncovered pixels reach the result"
        assert np.array_equal(nans[name], zeros[name]), f"{name}: differs from the run with zeros on the uncovered pixels"


@pytest.mark.parametrize("mode", ["deterministic", "exact_fp32_deterministic"])
@pytest.mark.parametrize("size", F.SIZES, ids=size_id)
@pytest.mark.parametrize("n", [33, 65, 97])
def test_deterministic_rows_repeat(n, size, mode, dev):
    scene = F.edge_scene(n, size)
    first, _ = grads(scene, "all", mode, dev)
    again = run_hip(scene, *F.upstream(scene.size, 7), mode, dev)
    for name in F.GRADS:
        assert np.array_equal(first[name], again[name]), f"{name}: two runs of the {mode} form differ"


@pytest.mark.parametrize("forms", [("split", "deterministic"), ("exact_fp32", "exact_fp32_deterministic")], ids=lambda f: f[0])
@pytest.mark.parametrize("size", F.SIZES, ids=size_id)
@pytest.mark.parametrize("n", [32, 33, 97])
def test_atomic_form_equals_deterministic_form(n, size, forms, dev):
    scene = F.edge_scene(n, size)
    atomic, det = (grads(scene, "all", m, dev)[0] for m in forms)
    for name in F.GRADS:
        e = grad_errors(atomic[name], det[name])[1]
        print(f"FORMS {forms[0]} {scene.name} {name}: relative L1 {e:.2e}")
        assert e <= FORMS_TOL, f"{name}: {forms[0]} vs {forms[1]} relative L1 {e:.3e} > {FORMS_TOL:g}"
