"""gs2d_maps.hip held to the float64 yardstick of tests/surfel_maps_reference.py at its tile edges: the maps' forward and
backward (scorp_gs2d_maps_forward / _backward), the regularisers' forward and backward (scorp_gs2d_regularizers_*: the
kReg instantiation without terms, g_out2), on the shapes that reach every seam of the 64 x 4 tiles and their two-pixel halo,
on a smooth surface, one with an empty disc, two one-pixel lines of coverage (the clamp of normalize() with a gradient),
a synthetic ray table with one centre on each side of the 1e-12 threshold, and planted non-finite depths.

Tolerances come from e_ref = |float32 CPU run - float64 run| of the yardstick itself, never from the kernel: per channel
4 e_ref + one float32 ulp of the channel's float64 maximum, per planted element 4 e_ref + 2^-22 |float64|
(tests/test_surfel_maps_cpu.py shows that the two runs take the same decisions everywhere, so nothing is left out).

Measured on an MI355X, worst over the thirteen shapes, the three depth ratios and every weighting: kernel error | e_ref, as
a fraction of the channel's float64 maximum (worst channel), and for the planted elements as a fraction of the element
(worst element), with the largest error / bound among them.

    case           maps forward          maps backward         regularisers backward   planted elements (maps | regularisers)
    smooth         1.29e-05 | 1.29e-05   1.68e-05 | 1.66e-05   1.39e-05 | 1.39e-05     -
    disc           1.29e-05 | 1.29e-05   1.68e-05 | 1.66e-05   1.39e-05 | 1.39e-05     -
    lines          0        | 0          1.33e-07 | 1.33e-07   1.18e-07 | 1.07e-07     1.09e-07 | 1.09e-07 (0.16 of the bound) | 1.41e-07 | 1.41e-07 (0.18)
    lines_camera   1.37e-04 | 1.37e-04   4.94e-06 | 4.79e-06   1.82e-04 | 1.82e-04     -
    threshold      0        | 0          1.18e-07 | 9.75e-08   1.01e-07 | 6.51e-08     1.12e-06 | 1.12e-06 (0.45) | 8.25e-07 | 8.25e-07 (0.45)
    nonfinite      9.65e-06 | 9.65e-06   1.68e-05 | 1.66e-05   5.10e-05 | 1.22e-04     -

The kernel's error is the yardstick's own float32 error to two digits almost everywhere: both round the same back-projected
points, and the difference of two neighbouring points is what limits the chain.  The regularisers' values: kernel error at
most 1.05e-07 of the value, at most 0.18 of the derived bound.  The real render (4 502 empty pixels of 7 680, clamp-branch
entries of 1e9 at isolated covered pixels): maps backward 1.9e+03 of a maximum of 1.2e+09 (1.5e-06), regularisers backward
1.6e-04 of 2.1e+02 (7.9e-07), the two values 4e-09 and 3e-08 relative.

Two inputs are not the first ones tried.  The lines on the smooth surface under the ring camera ("lines_camera") are
ill-conditioned where the clamp runs - the float32 run of the yardstick is itself off by 2e-4 of such an element at 9 x 63 and
by 14 % of one at 3 x 321, and an element where the float32 run happens to land within 1e-8 then leaves the kernel 2^-22 of
room for a chain that loses five digits - so that case is held per channel, and the per-element comparison runs on "lines",
the same two lines on exactly representable points (see the case builders).  And the planted elements of the threshold case
are the pixels a non-zero frame gradient reaches, listed from the positions of the two tilted rays: a pixel next to them
that no frame gradient reaches carries render_alpha's weight plus the surface-depth weight's chain, two terms of order one
that cancel to 1e-2 at 8 x 128 (3, 66), which is a property of the random weights and not of the planted centre.

One more finding: with the backward's kn = lambda g0 * (1 / HW) (three roundings) the exact "lines" case at 3 x 321 missed its
channel bound by 3 % (2.98e-11 against 2.90e-11 on a maximum of 1.7e-04: e_ref is nearly zero where every operation of the
restatement is exact); the kernel now divides lambda g0 by HW as the mean's backward does, and has the restatement's bits
there.
"""
import math

import pytest
import torch

from tests import surfel_maps_reference as ref

pytestmark = pytest.mark.gpu

LN, LD = 0.05, 100.0
NO_INTERIOR = ((1, 1), (1, 7), (7, 1), (2, 2))
PER_ELEMENT = (0, 1, 5)        # the g_allmap channels compared per element at a case's planted pixels


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _ulp32(x):
    """One float32 ulp at magnitude x."""
    return 0.0 if x == 0 else 2.0 ** (max(math.floor(math.log2(x)), -126) - 23)


def _gpu(c, dev):
    return c.allmap.to(dev), c.view.to(dev), c.rays_d.to(dev), c.rays_o.to(dev)


def _maps_direct(A, ratio, ws):
    """scorp_gs2d_maps_forward + _backward through the C ABI, a None weight as a NULL pointer; every output pre-filled with
    NaN so that an element the kernels do not write shows."""
    from scorp_amd import _C
    from scorp_amd.rasterizer3d import _ptr, _stream
    L = _C.lib()
    allmap, view, rays_d, rays_o = A
    H, W = allmap.shape[-2:]
    outs = [torch.full((ch, H, W), math.nan, device=allmap.device) for ch in (1, 3, 1, 1, 3)]
    _C.check(L.scorp_gs2d_maps_forward(W, H, _ptr(allmap), _ptr(view), _ptr(rays_d), _ptr(rays_o), float(ratio),
                                       *[_ptr(o) for o in outs], _stream()), "scorp_gs2d_maps_forward")
    g = torch.full((7, H, W), math.nan, device=allmap.device)
    _C.check(L.scorp_gs2d_maps_backward(W, H, _ptr(allmap), _ptr(view), _ptr(rays_d), _ptr(rays_o), float(ratio), _ptr(outs[3]),
                                        *[_ptr(w) for w in ws], _ptr(g), _stream()), "scorp_gs2d_maps_backward")
    return outs, g


def _reg_backward_direct(A, ratio, ln, ld, g_out2):
    from scorp_amd import _C
    from scorp_amd.rasterizer3d import _ptr, _stream
    allmap, view, rays_d, rays_o = A
    H, W = allmap.shape[-2:]
    g = torch.full((7, H, W), math.nan, device=allmap.device)
    _C.check(_C.lib().scorp_gs2d_regularizers_backward(W, H, _ptr(allmap), _ptr(view), _ptr(rays_d), _ptr(rays_o), float(ratio),
                                                       float(ln), float(ld), _ptr(g_out2), _ptr(g), _stream()),
             "scorp_gs2d_regularizers_backward")
    return g


def _hold(tag, got, want, e, planted, per_element, stats):
    """got [C,H,W] (the kernel's, any device) against want, e = e_ref [C,H,W] (float64, CPU).  Channels in per_element: the
    planted pixels per element, the rest per channel with the planted ones out of the maxima; other channels: per channel.
    A miss is noted in stats["misses"] (the test fails on them at its end, with all of them in sight)."""
    got = got.detach().cpu().double()
    assert got.shape == want.shape and bool(torch.isfinite(got).all()), tag
    err, misses = (got - want).abs(), stats.setdefault("misses", [])
    for ch in range(got.shape[0]):
        sel = torch.ones_like(planted)
        if ch in per_element and bool(planted.any()):
            sel = ~planted
            ep, wp, rp = err[ch][planted], want[ch][planted].abs(), e[ch][planted]
            bound = 4 * rp + 2.0 ** -22 * wp
            stats["planted_n"] = stats.get("planted_n", 0) + int(ep.numel())
            if bool((ep > 0).any()):
                stats["planted"] = max(stats.get("planted", 0.0), float((ep / bound.clamp_min(1e-300)).max()))
                nz = wp > 0
                stats["planted_rel"] = max(stats.get("planted_rel", 0.0), float((ep[nz] / wp[nz]).max()) if bool(nz.any()) else 0.0)
                stats["planted_eref_rel"] = max(stats.get("planted_eref_rel", 0.0), float((rp[nz] / wp[nz]).max()) if bool(nz.any()) else 0.0)
            for at in torch.nonzero(ep > bound).flatten().tolist():
                misses.append(f"{tag} channel {ch}, planted element {at}: kernel {float(got[ch][planted][at])!r}, float64 "
                              f"{float(want[ch][planted][at])!r}, |difference| {float(ep[at]):.3e}, e_ref {float(rp[at]):.3e}, "
                              f"bound {float(bound[at]):.3e}")
        if bool(sel.any()):
            k, er, top = float(err[ch][sel].max()), float(e[ch][sel].max()), float(want[ch][sel].abs().max())
            if top > 0:
                stats["kernel"], stats["e_ref"] = max(stats.get("kernel", 0.0), k / top), max(stats.get("e_ref", 0.0), er / top)
            if not k <= 4 * er + _ulp32(top):
                misses.append(f"{tag} channel {ch}: kernel error {k:.3e}, e_ref {er:.3e}, channel maximum {top:.3e}")


def _no_misses(*all_stats):
    misses = [m for s in all_stats for m in s.get("misses", [])]
    for m in misses:
        print("MISS " + m)
    assert not misses, f"{len(misses)} comparisons beyond their bound, the first: {misses[0]}"


def _report(what, shape, case, stats):
    print(f"TABLE {what} {shape[0]}x{shape[1]} {case}: kernel error {stats.get('kernel', 0.0):.2e} | e_ref {stats.get('e_ref', 0.0):.2e} "
          f"of the channel maximum (worst channel); {stats.get('planted_n', 0)} planted elements: kernel error {stats.get('planted_rel', 0.0):.2e} | "
          f"e_ref {stats.get('planted_eref_rel', 0.0):.2e} of the element (worst), worst error / bound {stats.get('planted', 0.0):.2f}")


@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_maps_forward_and_backward_match_the_float64_yardstick(shape, dev):
    """Every case x depth ratio at one shape.  Upstream weights: all five, each one alone (the other four NULL, through
    autograd's None) and all five NULL (the C ABI directly: g_allmap exactly zero).  render_alpha and render_dist are
    allmap[1] and allmap[6] bit for bit, surf_normal is exactly zero on the one-pixel border (everywhere on a shape without
    an interior pixel, where g_surf_normal alone also gives an exactly zero gradient); every other map and every
    g_allmap channel within 4 e_ref + one ulp of the channel's maximum, the planted elements of the lines and threshold
    cases within 4 e_ref + 2^-22 |float64| each."""
    from scorp_amd.rasterizer2d import surfel_maps
    H, W = shape
    ws = ref.upstream_weights(H, W)
    ws_dev = [w.to(dev) for w in ws]
    configs = [("all", list(range(5)))] + [(ref.MAPS[k], [k]) for k in range(5)]
    every = []
    for case in ref.CASES:
        c = ref.make_case(case, H, W)
        A = _gpu(c, dev)
        fwd, bwd = {}, {}
        every += [fwd, bwd]
        for ratio in ref.RATIOS:
            tag = f"{case} {H}x{W} ratio {ratio}"
            m64 = em = None
            for name, keep in configs:
                sub = [w if k in keep else None for k, w in enumerate(ws)]
                m64_, g64, em_, eg = ref.maps_e_ref(c.allmap, c.view, c.rays_d, c.rays_o, ratio, sub)
                m64, em = m64 or m64_, em or em_
                a = A[0].clone().requires_grad_(True)
                outs = surfel_maps(a, A[1], A[2], A[3], ratio)
                sum((outs[k] * ws_dev[k]).sum() for k in keep).backward()
                _hold(f"{tag}, weights {name}: g_allmap", a.grad, g64, eg, c.planted, PER_ELEMENT, bwd)
                if name == "all":
                    assert torch.equal(outs[0].detach()[0], A[0][1]) and torch.equal(outs[2].detach()[0], A[0][6]), tag
                    sn = outs[4].detach()
                    border = torch.ones(H, W, dtype=torch.bool, device=dev)
                    border[1:-1, 1:-1] = False
                    assert float(sn[:, border].abs().max()) == 0.0, tag
                    _hold(f"{tag}: render_normal", outs[1], m64[1], em[1], c.planted, (), fwd)
                    _hold(f"{tag}: surf_depth", outs[3], m64[3], em[3], c.planted, (), fwd)
                    _hold(f"{tag}: surf_normal", sn, m64[4], em[4], c.planted_normals, (0, 1, 2), fwd)
                if name == "surf_normal" and shape in NO_INTERIOR:
                    assert float(a.grad.abs().max()) == 0.0, tag
            outs, g = _maps_direct(A, ratio, [None] * 5)
            assert float(g.abs().max()) == 0.0 and bool(torch.isfinite(torch.cat(outs)).all()), tag
            if shape in NO_INTERIOR:
                assert float(outs[4].abs().max()) == 0.0, tag
        _report("maps forward", shape, case, fwd)
        _report("maps backward", shape, case, bwd)
    _no_misses(*every)


def _crop_runs(dev, H, W, case, ratio=0.5):
    c, ws = ref.make_case(case, H, W), ref.upstream_weights(H, W)
    wide = _maps_direct(_gpu(c, dev), ratio, [w.to(dev) for w in ws])
    return c, ws, wide


@pytest.mark.parametrize("case", ["smooth", "disc"])
def test_a_tile_seam_at_every_position_changes_no_bit(case, dev):
    """The backward stages points and frame gradients per 64 x 4 tile and promises the same expressions in the same order per
    value; every operation is local (radius 1 for surf_normal, 2 for the gradient).  So a crop run on its own - its seams
    elsewhere relative to the content - gives the wide run's bits away from the crop's edge: columns [s, s + 66) of the
    13 x 130 case for every s in 0..63 (surf_normal one pixel in, g_allmap three pixels in), and rows [s, s + 17) of a
    21 x 66 case for s in 0..3.  No tolerance."""
    ratio = 0.5
    H, W = 13, 130
    c, ws, (outs_w, g_w) = _crop_runs(dev, H, W, case)
    rays = c.rays_d.reshape(H, W, 3)
    for s in range(64):
        A = (c.allmap[:, :, s:s + 66].contiguous().to(dev), c.view.to(dev), rays[:, s:s + 66].reshape(-1, 3).contiguous().to(dev),
             c.rays_o.to(dev))
        outs, g = _maps_direct(A, ratio, [w[:, :, s:s + 66].contiguous().to(dev) for w in ws])
        assert torch.equal(outs[4][:, 1:-1, 1:-1], outs_w[4][:, 1:-1, s + 1:s + 65]), f"surf_normal, column shift {s}"
        assert torch.equal(g[:, :, 3:-3], g_w[:, :, s + 3:s + 63]), f"g_allmap, column shift {s}"
    H, W = 21, 66
    c, ws, (outs_w, g_w) = _crop_runs(dev, H, W, case)
    rays = c.rays_d.reshape(H, W, 3)
    for s in range(4):
        A = (c.allmap[:, s:s + 17].contiguous().to(dev), c.view.to(dev), rays[s:s + 17].reshape(-1, 3).contiguous().to(dev),
             c.rays_o.to(dev))
        outs, g = _maps_direct(A, ratio, [w[:, s:s + 17].contiguous().to(dev) for w in ws])
        assert torch.equal(outs[4][:, 1:-1, 1:-1], outs_w[4][:, s + 1:s + 16, 1:-1]), f"surf_normal, row shift {s}"
        assert torch.equal(g[:, 3:-3], g_w[:, s + 3:s + 14]), f"g_allmap, row shift {s}"
    assert bool(torch.isfinite(g_w).all()) and float(g_w.abs().max()) > 0


@pytest.mark.parametrize("shape", ref.SHAPES + ((1024, 3), (1028, 3)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_regularizer_values_match_the_float64_yardstick(shape, dev):
    """(lambda_normal mean(1 - render_normal . surf_normal), lambda_dist mean(render_dist)), every case x ratio; 1024 x 3 and
    1028 x 3 are 256 and 257 workgroups, the last one past the finalize kernel's first stride.  With term_i the per-pixel
    float64 term and e_ref(term_i) its float32-against-float64 error, each value is within
    lambda (4 mean e_ref(term_i) + 9 2^-24 mean |term_i|) + 2^-24 |value|: the eight-level float32 tree over a
    workgroup's 256 pixels and its four-way add (nine roundings of a partial sum of terms of one sign or bounded by
    mean |term|), the final cast, and nothing from the double-precision finalize.  A shape without an interior pixel has the
    normal value exactly float32(lambda_normal): every pixel contributes exactly 1, a lane outside the image nothing.  Two
    calls give the same bits."""
    from scorp_amd.rasterizer2d import surfel_regularizer_losses
    H, W = shape
    for case in ref.CASES:
        c = ref.make_case(case, H, W)
        A = _gpu(c, dev)
        for ratio in ref.RATIOS:
            r64, er = ref.regularizers_e_ref(c.allmap, c.view, c.rays_d, c.rays_o, ratio, LN, LD)
            with torch.no_grad():
                out = surfel_regularizer_losses(*A, ratio, LN, LD)
                again = surfel_regularizer_losses(*A, ratio, LN, LD)
            assert torch.equal(out, again)
            for k, (lam, term) in enumerate(((LN, "term_n"), (LD, "term_d"))):
                want, got = float(r64["values"][k]), float(out[k])
                bound = lam * (4 * float(er[term].mean()) + 9 * 2.0 ** -24 * float(r64[term].abs().mean())) + 2.0 ** -24 * abs(want)
                print(f"TABLE regularisers forward {H}x{W} {case} ratio {ratio} value {k}: kernel error {abs(got - want):.2e} | "
                      f"lambda mean e_ref {lam * float(er[term].mean()):.2e} | bound {bound:.2e} of {want:.6e}")
                assert abs(got - want) <= bound, (case, shape, ratio, k, got, want)
            if shape in NO_INTERIOR:
                assert float(out[0]) == float(torch.tensor(LN, dtype=torch.float32)), (case, shape, ratio)


def test_regularizer_workspace_one_byte_short_is_refused_before_any_launch(dev):
    """A host check: SCORP_ERR_INVALID, the output untouched."""
    from scorp_amd import _C
    from scorp_amd.rasterizer3d import _ptr, _stream
    L = _C.lib()
    H, W = 13, 130
    A = _gpu(ref.make_case("smooth", H, W), dev)
    wb = L.scorp_gs2d_regularizers_workspace_bytes(W, H)
    assert wb >= 8 * ((W + 63) // 64) * ((H + 3) // 4)
    ws = torch.empty(wb, dtype=torch.uint8, device=dev)
    out = torch.full((2,), -7.0, device=dev)
    args = (W, H, _ptr(A[0]), _ptr(A[1]), _ptr(A[2]), _ptr(A[3]), 0.5, LN, LD, _ptr(out), _ptr(ws))
    assert L.scorp_gs2d_regularizers_forward(*args, wb - 1, _stream()) == _C.ERR_INVALID
    assert b"workspace" in L.scorp_last_error()
    torch.cuda.synchronize()
    assert out.tolist() == [-7.0, -7.0]
    assert L.scorp_gs2d_regularizers_forward(*args, wb, _stream()) == 0
    assert bool(torch.isfinite(out).all()) and float(out[0]) != -7.0


G_OUT2 = (None, (1.0, 1.0), (2.0, 0.5), (1.0, 0.0), (0.0, 1.0))


@pytest.mark.parametrize("shape", ref.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_regularizer_backward_matches_float64_autograd_of_the_scalar(shape, dev):
    """d (g_out2 . values) / d allmap, every case x ratio x g_out2 in {NULL, (1, 1), (2, 0.5), (1, 0), (0, 1)}: the channel
    and planted-element bounds of the maps' test (on the lines, G = -kn render_normal alpha is non-zero where the clamp
    runs).  g_allmap[6] is one constant: the same bits at every pixel, within two float32 ulps of lambda_dist g1 / (H W)
    (float32 roundings of lambda g1 and of the division produce it).  g0 = 0 or lambda_normal = 0: channels 0-5 exactly zero; g1 = 0 or
    lambda_dist = 0: channel 6 exactly zero.  NULL gives the bits of (1, 1)."""
    from scorp_amd.rasterizer2d import surfel_regularizer_losses
    H, W = shape
    every = []
    for case in ref.CASES:
        c = ref.make_case(case, H, W)
        A = _gpu(c, dev)
        stats = {}
        every.append(stats)
        for ratio in ref.RATIOS:
            g_null = None
            for g2 in G_OUT2:
                tag = f"{case} {H}x{W} ratio {ratio} g_out2 {g2}"
                r64, er = ref.regularizers_e_ref(c.allmap, c.view, c.rays_d, c.rays_o, ratio, LN, LD, g2)
                if g2 is None:
                    g = g_null = _reg_backward_direct(A, ratio, LN, LD, None)
                else:
                    a = A[0].clone().requires_grad_(True)
                    (surfel_regularizer_losses(a, A[1], A[2], A[3], ratio, LN, LD) * torch.tensor(g2, device=dev)).sum().backward()
                    g = a.grad
                _hold(tag, g, r64["g_allmap"], er["g_allmap"], c.planted, PER_ELEMENT, stats)
                g0, g1 = g2 or (1.0, 1.0)
                assert bool((g[6] == g[6].flatten()[0]).all()), tag
                want6 = LD * g1 / (H * W)
                assert abs(float(g[6, 0, 0]) - want6) <= 2 * _ulp32(want6), tag
                if g0 == 0.0:
                    assert float(g[:6].abs().max()) == 0.0, tag
                if g1 == 0.0:
                    assert float(g[6].abs().max()) == 0.0, tag
                if g2 == (1.0, 1.0):
                    assert torch.equal(g, g_null), tag
            ones = torch.ones(2, device=dev)
            assert float(_reg_backward_direct(A, ratio, 0.0, LD, ones)[:6].abs().max()) == 0.0, (case, shape, ratio)
            assert float(_reg_backward_direct(A, ratio, LN, 0.0, ones)[6].abs().max()) == 0.0, (case, shape, ratio)
        _report("regularisers backward", shape, case, stats)
    _no_misses(*every)


@pytest.fixture(scope="module")
def real_render(dev):
    """The allmap of renderer2d.render: 3 000 surfels of SH degree 1, 96 x 80 - silhouettes and the rasterizer's own empty
    pixels - with its camera's ray table, on the CPU."""
    from scorp_amd.renderer2d import GaussianModel2D, _camera_rays, render
    from scorp_amd.synthetic import make_gaussians, ring_cameras
    from scorp_amd.train import PipelineParams
    pipe = PipelineParams()
    pipe.depth_ratio = 0.5
    raw = make_gaussians(3000, 1, 23, log_scale_mean=math.log(0.05), scale_dims=2)
    cam = ring_cameras(3, 96, 80, 4, radius=6.0, device=dev)[1]     # far enough for the cloud to leave empty pixels beside it
    m = GaussianModel2D.from_raw(raw, 1, device=dev)
    m.active_sh_degree = 1
    with torch.no_grad():
        allmap = render(cam, m, pipe, torch.zeros(3, device=dev)).allmap.clone()
    rays_d, rays_o = _camera_rays(cam, dev)
    return ref.Case(allmap.cpu(), cam.world_view_transform.cpu(), rays_d.cpu().contiguous(), rays_o.cpu().contiguous(),
                    torch.zeros(80, 96, dtype=torch.bool))


def test_a_real_render_matches_the_float64_yardstick(real_render, dev):
    """The plain maps backward (all five upstream weights) and the regularisers on the allmap of a real render, depth ratio
    0.5, at the tolerance the project applies to this chain on real renders (tests/test_surfel_terms_gpu.py): g_allmap
    within 2e-4 of its maximum + 1e-12, the two values within 1e-5 relative."""
    from scorp_amd.rasterizer2d import surfel_maps, surfel_regularizer_losses
    c, ratio = real_render, 0.5
    H, W = c.allmap.shape[-2:]
    empty, seen = int((c.allmap[1] == 0).sum()), int((c.allmap[1] > 0).sum())
    print(f"TABLE real render: {empty} empty pixels, {seen} covered")
    assert empty > 0 and seen > 0.2 * H * W
    A = _gpu(c, dev)
    ws = ref.upstream_weights(H, W)
    _, g64 = ref.maps_autograd(c.allmap, c.view, c.rays_d, c.rays_o, ratio, ws)
    a = A[0].clone().requires_grad_(True)
    outs = surfel_maps(a, A[1], A[2], A[3], ratio)
    sum((o * w.to(dev)).sum() for o, w in zip(outs, ws)).backward()
    err, top = float((a.grad.cpu().double() - g64).abs().max()), float(g64.abs().max())
    print(f"TABLE real render maps backward: max |difference| {err:.3e} of max {top:.3e}")
    assert bool(torch.isfinite(a.grad).all()) and err <= 2e-4 * top + 1e-12
    g2 = (2.0, 0.5)
    r64 = ref.regularizers_autograd(c.allmap, c.view, c.rays_d, c.rays_o, ratio, LN, LD, g2)
    a = A[0].clone().requires_grad_(True)
    out = surfel_regularizer_losses(a, A[1], A[2], A[3], ratio, LN, LD)
    (out * torch.tensor(g2, device=dev)).sum().backward()
    for k in range(2):
        got, want = float(out.detach()[k]), float(r64["values"][k])
        print(f"TABLE real render value {k}: {got:.9g} against {want:.9g}")
        assert abs(got - want) <= 1e-5 * abs(want)
    err, top = float((a.grad.cpu().double() - r64["g_allmap"]).abs().max()), float(r64["g_allmap"].abs().max())
    print(f"TABLE real render regularisers backward: max |difference| {err:.3e} of max {top:.3e}")
    assert bool(torch.isfinite(a.grad).all()) and err <= 2e-4 * top + 1e-12
