"""The all-fp32 blend backward (SCORP_BACKWARD_EXACT_FP32) at the edges of its matrix layout, against the float64 oracle.

The exact form reduces each half-group of 8 hits on v_mfma_f32_4x4x1_16b_f32: 16 blocks of (hit quad, pixel row of the
8x8 block), followed by a sum over the eight rows across lanes.  These scenes are small enough that every splat covers
(nearly) every pixel block, so a block's hit count is about N: partial quads, partial half-groups, partial groups of 16
and a second chunk of 64 are all reached, on images whose sides are not multiples of 8 or 16 (pixels outside the image
carry zeros through the same lanes).  Both dispatches of the exact form are covered: with and without depth / alpha
upstream gradients, and the deterministic rows."""
import math

import numpy as np
import pytest
import torch

from tests.util import assert_no_further_from_f64, image_weights, make_case

pytestmark = pytest.mark.gpu

HITS = [1, 7, 8, 9, 15, 17, 65]
SIZES = [(13, 11), (37, 21)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need a GPU"
    from scorp_amd import _C
    _C.lib()
    return torch.device("cuda:0")


@pytest.mark.parametrize("mode", ["exact_fp32", "exact_fp32_deterministic"])
@pytest.mark.parametrize("depth_alpha", [True, False])
@pytest.mark.parametrize("n", HITS)
def test_exact_backward_partial_groups_against_f64(n, depth_alpha, mode, dev):
    from oracle.gs_oracle import OracleRender
    from scorp_amd.rasterizer3d import backward_precision
    from scorp_amd.refcall import render3d_reference_call
    W, H = SIZES[HITS.index(n) % 2]
    seed = 30 + n
    kw, _ = make_case(N=n, W=W, H=H, deg=2, seed=seed, log_scale=math.log(0.5), log_scale_std=0.2, bg=(0.3, 0.1, 0.6))
    wc, wd, wa = image_weights(H, W, seed)
    if not depth_alpha:
        wd, wa = np.zeros_like(wd), np.zeros_like(wa)
    with backward_precision(mode):
        out, t = render3d_reference_call(kw, dev, requires_grad=True)
    color, _, depth, alpha = out
    loss = (color * torch.tensor(wc, device=dev)).sum()
    if depth_alpha:
        loss = loss + (depth * torch.tensor(wd, device=dev)).sum() + (alpha * torch.tensor(wa, device=dev)).sum()
    loss.backward()
    g32 = OracleRender(np.float32, **kw).backward(wc, wd, wa)
    g64 = OracleRender(np.float64, **kw).backward(wc, wd, wa)
    checked = 0
    for name, key in (("means3D", "means3D"), ("means2D", "means2D"), ("opacities", "opacities"), ("shs", "shs"),
                      ("scales", "scales"), ("rotations", "rotations")):
        got = t[name].grad.detach().cpu().numpy()
        if not np.abs(np.asarray(g64[key])).sum():
            np.testing.assert_array_equal(got, 0.0)   # (nothing visible: every gradient is an exact zero)
            continue
        assert np.isfinite(got).all(), f"{name}: non-finite gradient"
        assert_no_further_from_f64(name, got, g32[key], g64[key])
        checked += 1
    assert n == 1 or checked, "the scene left nothing to compare"
