"""The float64 yardstick of the 2DGS per-pixel maps and regularisers (tests/surfel_maps_reference.py) checked without a GPU,
before tests/test_surfel_maps_edges_gpu.py holds gs2d_maps.hip to it: its float32 run is the restatement of
oracle/surfel_maps_ref.py bit for bit, its float64 autograd agrees with central finite differences, the planted cases have
the closed forms they were planted for, and on every (case, shape, ratio) the GPU module runs the float32 and the float64
run take the same decisions everywhere, so that no element has to be left out of any comparison."""
import math

import pytest
import torch

from tests import surfel_maps_reference as ref

EPS = 1e-12      # torch.nn.functional.normalize's default, kNormEps of gs2d_maps.hpp


def _sn_only(H, W, at, value):
    """Upstream weights with nothing but g_surf_normal at one pixel."""
    w = torch.zeros(3, H, W)
    w[:, at[0], at[1]] = torch.tensor(value)
    return [None, None, None, None, w]


@pytest.mark.parametrize("case", ref.CASES)
def test_float32_run_of_the_yardstick_is_the_restatement(case):
    """maps_autograd(dtype=float32) against oracle.surfel_maps_ref.surfel_maps_ref under float32 autograd: the five maps the
    same bits, the gradient the same bits wherever the restatement's is a number (its nan_to_num leaves 0 * NaN where the
    yardstick writes the documented zero, and nowhere else)."""
    from oracle.surfel_maps_ref import surfel_maps_ref
    for H, W in ((3, 3), (5, 65), (13, 130)):
        for ratio in ref.RATIOS:
            c, ws = ref.make_case(case, H, W), ref.upstream_weights(H, W)
            maps, g = ref.maps_autograd(c.allmap, c.view, c.rays_d, c.rays_o, ratio, ws, dtype=torch.float32)
            a = c.allmap.clone().requires_grad_(True)
            outs = surfel_maps_ref(a, c.view, c.rays_d, c.rays_o, ratio)
            sum((o * w).sum() for o, w in zip(outs, ws)).backward()
            for name, x, y in zip(ref.MAPS, maps, outs):
                assert torch.equal(x, y.detach()), (name, H, W, ratio)
            num = ~torch.isnan(a.grad)
            assert torch.equal(g[num], a.grad[num]) and not torch.isnan(g).any(), (H, W, ratio)
            assert bool(num[2:5].all()) and bool(num[6].all())
            assert bool((num[:2] | ~ref.decisions(c.allmap)[0]).all())     # NaN only where the quotient is not kept


@pytest.mark.parametrize("case", ["smooth", "disc"])
@pytest.mark.parametrize("ratio", ref.RATIOS)
def test_yardstick_agrees_with_float64_finite_differences(case, ratio):
    """7 x 9: d (sum_k (map_k w_k).sum()) / d allmap by float64 autograd against central differences of the float64 forward
    (h = 1e-6), every one of the 7 x 63 entries - interior, border and next-to-border pixels, empty ones included - and the
    same for the regularisers' scalar.  The alpha that weights surf_normal is held at the unperturbed one, as render()
    detaches it.  3e-7 of the gradient's maximum: h^2 times a third derivative of order one, plus 1e-16 |f| / h of rounding."""
    H, W, h = 7, 9, 1e-6
    c, ws = ref.make_case(case, H, W), ref.upstream_weights(H, W)
    e_ok, m_ok = ref.decisions(c.allmap)
    a64, v, rd, ro = c.allmap.double(), c.view.double(), c.rays_d.double(), c.rays_o.double()
    if case == "disc":
        assert int((c.allmap[1] == 0).sum()) >= 3
    g_out2, ln, ld = (2.0, 0.5), 0.05, 100.0

    def f_maps(a):
        maps = ref.maps_from_allmap(a, e_ok, m_ok, v, rd, ro, ratio, alpha_weight=a64[1:2])
        return float(sum((m * w.double()).sum() for m, w in zip(maps, ws)))

    def f_reg(a):
        _, rn, dist, _, sn = ref.maps_from_allmap(a, e_ok, m_ok, v, rd, ro, ratio, alpha_weight=a64[1:2])
        return float(g_out2[0] * ln * (1 - (rn * sn).sum(dim=0)).mean() + g_out2[1] * ld * dist.mean())

    g_maps = ref.maps_autograd(c.allmap, c.view, c.rays_d, c.rays_o, ratio, ws)[1]
    g_reg = ref.regularizers_autograd(c.allmap, c.view, c.rays_d, c.rays_o, ratio, ln, ld, g_out2)["g_allmap"]
    for name, f, g in (("maps", f_maps, g_maps), ("regularisers", f_reg, g_reg)):
        worst = 0.0
        for ch in range(7):
            for i in range(H):
                for j in range(W):
                    ap, am = a64.clone(), a64.clone()
                    ap[ch, i, j] += h
                    am[ch, i, j] -= h
                    worst = max(worst, abs((f(ap) - f(am)) / (2 * h) - float(g[ch, i, j])))
        print(f"{case} ratio {ratio} {name}: max |autograd - finite difference| {worst:.3e} of max {float(g.abs().max()):.3e}")
        assert worst <= 3e-7 * float(g.abs().max())


def test_threshold_case_has_one_centre_on_each_side_of_the_clamp():
    """13 x 130: at the "clamp" centre |dv x dh| = 2^-40 < 1e-12, the forward normal is (0, 0, 2^-40 / 1e-12) alpha (length
    0.909 alpha) and the gradient is (G / 1e-12) through the cross product; at the "normalise" centre |dv x dh| = 2^-39,
    the normal is (0, 0, 1) alpha and the gradient is (G - n (n . G)) / 2^-39 through the cross product.  Both in closed
    form for an upstream weight on that centre's surf_normal alone, read at the centre's lower neighbour (whose ray is
    (2^-20, 0, 1)): (2^-40 Gz - 2^-20 Gx) / 1e-12 against -2^20 Gx - the two formulas differ by the 9 % between 2^-40 and
    1e-12, so each centre tells which one ran.  The float32 lengths are exactly 2^-40 and 2^-39."""
    H, W, ratio = 13, 130, 0.5
    c = ref.make_case("threshold", H, W)
    assert set(c.centres) == {"clamp", "normalise"}
    sd32 = ref.maps_autograd(c.allmap, c.view, c.rays_d, c.rays_o, ratio, [None] * 5, dtype=torch.float32)[0][3]
    len32 = ref.frame_lengths(sd32, c.rays_d, c.rays_o)
    Gw = (0.75, -1.25, 0.5)
    for kind, (y, x) in c.centres.items():
        assert float(len32[y - 1, x - 1]) == (2.0 ** -40 if kind == "clamp" else 2.0 ** -39)
        assert c.planted_normals[y, x] and c.planted[y - 1, x] and c.planted[y + 1, x] and c.planted[y, x - 1] and c.planted[y, x + 1]
        alpha = float(c.allmap[1, y, x])
        maps, g = ref.maps_autograd(c.allmap, c.view, c.rays_d, c.rays_o, ratio, _sn_only(H, W, (y, x), Gw))
        want_z = alpha * (2.0 ** -40 / EPS if kind == "clamp" else 1.0)
        assert maps[4][0, y, x] == 0 and maps[4][1, y, x] == 0 and abs(float(maps[4][2, y, x]) - want_z) <= 1e-14
        G = [w * alpha for w in Gw]
        gd = (2.0 ** -40 * G[2] - 2.0 ** -20 * G[0]) / EPS if kind == "clamp" else -(2.0 ** 20) * G[0]
        other = -(2.0 ** 20) * G[0] if kind == "clamp" else (2.0 ** -40 * G[2] - 2.0 ** -20 * G[0]) / EPS
        got = float(g[5, y + 1, x])
        assert abs(got - ratio * gd) <= 1e-12 * abs(ratio * gd) and abs(got - ratio * other) > 0.05 * abs(got)
        assert abs(float(g[0, y + 1, x]) - (1 - ratio) * gd / float(c.allmap[1, y + 1, x])) <= 1e-12 * abs(gd)
    assert 0.90 < 2.0 ** -40 / EPS < 0.91


def test_lines_case_runs_the_clamp_with_a_gradient():
    """13 x 130, an upstream weight on the surf_normal of one centre of the vertical line, two rows from the crossing: dh is
    exactly zero (both horizontal neighbours are empty: the same point rays_o), so is the cross product; g_dv = dh x gc = 0,
    g_dh = (G / 1e-12) x dv, which reaches the median depth of the two EMPTY horizontal neighbours as +- g_dh . rays_d times
    depth_ratio - order 1e11 - and nothing else.  (The "lines" case: exactly representable points, dv = (0, 1/4, 0).)"""
    H, W, ratio = 13, 130, 0.5
    c = ref.make_case("lines", H, W)
    yl, xl = c.centres["cross"]
    y, x, Gw = yl + 2, xl, (0.75, -1.25, 0.5)
    assert c.allmap[1, y, x] > 0 and c.allmap[1, y, x - 1] == 0 and c.allmap[1, y, x + 1] == 0
    maps, g = ref.maps_autograd(c.allmap, c.view, c.rays_d, c.rays_o, ratio, _sn_only(H, W, (y, x), Gw))
    len64 = ref.frame_lengths(maps[3], c.rays_d.double(), c.rays_o.double())
    assert float(len64[y - 1, x - 1]) == 0.0 and float(maps[4][:, y, x].abs().max()) == 0.0
    rays, sd = c.rays_d.double().reshape(H, W, 3), maps[3][0]
    dv = sd[y + 1, x] * rays[y + 1, x] - sd[y - 1, x] * rays[y - 1, x]
    assert float(dv.norm()) > 1e-3
    gc = torch.tensor(Gw, dtype=torch.float64) * float(c.allmap[1, y, x]) / EPS
    g_dh = torch.linalg.cross(gc, dv)
    for xn, sign in ((x + 1, 1.0), (x - 1, -1.0)):
        want = ratio * sign * float(g_dh @ rays[y, xn])
        assert abs(want) > 1e10 and abs(float(g[5, y, xn]) - want) <= 1e-12 * abs(want)
    rest = g.clone()
    rest[5, y, x - 1] = rest[5, y, x + 1] = 0.0
    assert float(rest.abs().max()) == 0.0            # g_dv = 0: nothing reaches the line's own pixels


def test_nonfinite_case_has_zero_depth_and_zero_gradient_where_planted():
    """13 x 130 and 5 x 65: at a subnormal alpha the float32 quotient overflows and the float64 one does not - the expected
    depth is 0 in both runs and channels 0 and 1 carry nothing but render_alpha's own weight; at a NaN or +inf median the
    median depth is 0 and channel 5 carries nothing; the sites lie on the border and on both sides of the first tile seam."""
    for H, W in ((13, 130), (5, 65)):
        c, ws = ref.make_case("nonfinite", H, W), ref.upstream_weights(H, W)
        s = c.sites
        assert (0, 0) in s["subnormal_alpha"] and (H - 1, W - 1) in s["nan_median"] and (H - 1, 0) in s["inf_median"]
        assert (3, 63) in s["subnormal_alpha"] and (4, 64) in s["subnormal_alpha"] and (3, 64) in s["nan_median"] and (4, 63) in s["inf_median"]
        for y, x in s["subnormal_alpha"]:
            q32, q64 = c.allmap[0, y, x] / c.allmap[1, y, x], c.allmap[0, y, x].double() / c.allmap[1, y, x].double()
            assert c.allmap[1, y, x] > 0 and math.isinf(float(q32)) and math.isfinite(float(q64))
        assert all(math.isnan(float(c.allmap[5, y, x])) for y, x in s["nan_median"])
        assert all(float(c.allmap[5, y, x]) == math.inf for y, x in s["inf_median"])
        for dtype in (torch.float64, torch.float32):
            m0, g0 = ref.maps_autograd(c.allmap, c.view, c.rays_d, c.rays_o, 0.0, ws, dtype=dtype)
            m1, g1 = ref.maps_autograd(c.allmap, c.view, c.rays_d, c.rays_o, 1.0, ws, dtype=dtype)
            for y, x in s["subnormal_alpha"]:
                assert float(m0[3][0, y, x]) == 0.0 and float(g0[0, y, x]) == 0.0 and float(g0[1, y, x]) == float(ws[0][0, y, x])
            for y, x in s["nan_median"] + s["inf_median"]:
                assert float(m1[3][0, y, x]) == 0.0 and float(g1[5, y, x]) == 0.0
            assert torch.isfinite(g0).all() and torch.isfinite(g1).all()


@pytest.mark.parametrize("case", ref.CASES)
def test_float32_and_float64_take_the_same_decisions_on_every_gpu_case(case):
    """Every (shape, ratio) of the GPU module, the two extra regulariser shapes included; the exclusion cap is ZERO:
    * the maps and gradients of both runs, maps' loss and regularisers' scalar, hold no NaN and no infinity - every element is
      compared;
    * the decisions the yardstick takes are the restatement's own nan_to_num outcomes (its float32 surface depth is the same
      bits), and float64 leaves no quotient it keeps non-finite;
    * both runs are on the same side of the clamp at every centre, and no float32 length is close enough to 1e-12 for another
      association or a fused multiply-add to change sides: it is exactly 0, exactly the planted 2^-40 or 2^-39, or above
      1e-9."""
    from oracle.surfel_maps_ref import surfel_maps_ref
    for H, W in ref.SHAPES + ((1024, 3), (1028, 3)):
        c, ws = ref.make_case(case, H, W), ref.upstream_weights(H, W)
        e_ok, m_ok = ref.decisions(c.allmap)
        q64 = c.allmap[0:1].double() / c.allmap[1:2].double()
        assert bool(torch.isfinite(q64[e_ok]).all())
        for ratio in ref.RATIOS:
            with torch.no_grad():
                sd_restated = surfel_maps_ref(c.allmap, c.view, c.rays_d, c.rays_o, ratio)[3]
            m64, g64, em, eg = ref.maps_e_ref(c.allmap, c.view, c.rays_d, c.rays_o, ratio, ws)
            m32 = ref.maps_autograd(c.allmap, c.view, c.rays_d, c.rays_o, ratio, ws, dtype=torch.float32)[0]
            assert torch.equal(m32[3], sd_restated), (H, W, ratio)
            assert all(bool(torch.isfinite(x).all()) for x in m64 + em + [g64, eg]), (H, W, ratio)
            r64, er = ref.regularizers_e_ref(c.allmap, c.view, c.rays_d, c.rays_o, ratio, 0.05, 100.0, (2.0, 0.5))
            assert all(bool(torch.isfinite(x).all()) for x in list(er.values()) + [r64["g_allmap"], r64["values"]]), (H, W, ratio)
            len32 = ref.frame_lengths(m32[3], c.rays_d, c.rays_o)
            len64 = ref.frame_lengths(m64[3], c.rays_d.double(), c.rays_o.double())
            assert torch.equal(len32 > EPS, len64 > EPS), (H, W, ratio)
            near = (len32 != 0) & (len32 < 1e-9)
            if case == "threshold":
                near &= (len32 != 2.0 ** -40) & (len32 != 2.0 ** -39)
            assert int(near.sum()) == 0, (H, W, ratio)
