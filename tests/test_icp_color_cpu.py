"""The coloured ICP yardstick (tests/icp_color_reference.py), the properties of every fixture the GPU tests rely on
(tests/icp_color_fixtures.py), shown with the float64 reference alone, the header's declarations and the argument errors of
scorp_amd/icp.py that need no device.  No GPU."""
import numpy as np
import pytest
import torch

from tests import icp_color_fixtures as cfx
from tests import icp_color_reference as cref
from tests import icp_plane_fixtures as pfx
from tests import icp_plane_reference as pref
from tests import icp_probe_fixtures as fx


def _ratios_clear(eigenvalues):
    """icp_plane_reference.eig_ratios_clear for the gradient rule's M (rows of three eigenvalues)."""
    return pref.eig_ratios_clear(list(eigenvalues))


# ---- the update, on the yardstick alone ----

def test_constant_colour_and_lambda_one_give_the_point_to_plane_step():
    src, Ip, tgt, nrm, Iq, grad, r, inits, _ = cfx.margin_fixture()
    flat_p, flat_q, zero = np.full(len(src), 0.4), np.full(len(tgt), 0.4), np.zeros_like(grad)
    for T0 in inits:
        want = pref.registration_icp(src, tgt, nrm, r, T0, max_iteration=cfx.RUN_UPDATES, relative_fitness=0.0, relative_rmse=0.0)
        for lam in cfx.LAMBDAS:
            y = cref.registration_icp(src, flat_p, tgt, nrm, flat_q, zero, r, T0, lam, max_iteration=cfx.RUN_UPDATES,
                                      relative_fitness=0.0, relative_rmse=0.0)
            d = float(np.abs(y["transformation"] - want["transformation"]).max())
            print(f"constant colour, lambda {lam}: |T - point-to-plane yardstick| after {cfx.RUN_UPDATES} updates {d:.3g}")
            assert d <= 1e-13 and y["passes"] == want["passes"]
        y = cref.registration_icp(src, Ip, tgt, nrm, Iq, grad, r, T0, 1.0, max_iteration=cfx.RUN_UPDATES, relative_fitness=0.0,
                                  relative_rmse=0.0)
        assert np.abs(y["transformation"] - want["transformation"]).max() <= 1e-13


def test_terms_of_the_system():
    """A zero normal leaves the colour term, a zero gradient with equal intensities the geometric one; no pairs and
    coincident pairs of equal intensity give the identity exactly."""
    rng = np.random.default_rng(4)
    q = rng.normal(size=(80, 3)) + (3.0, -2.0, 1.0)
    x = q + rng.normal(scale=0.02, size=q.shape)
    n = pfx.unit_normals(80, 5).astype(np.float64)
    d = cfx.tangent_gradients(n, 6).astype(np.float64)
    Iq, Ip = rng.random(80), rng.random(80)
    ct, s = pref.frame(q)
    A0, b0 = pref.system(x, q, n, ct, s)
    A, b = cref.system(x, q, n, np.zeros_like(d), Iq, Iq, 0.7, ct, s)
    assert np.abs(A - 0.7 * A0).max() <= 1e-13 * np.abs(A0).max() and np.abs(b - 0.7 * b0).max() <= 1e-13 * np.abs(b0).max()
    A, b = cref.system(x, q, np.zeros_like(n), d, Iq, Ip, 0.7, ct, s)
    J = np.hstack([np.cross(x - ct, d) / s, d])
    rho = (d * (x - q)).sum(axis=1) + Iq - Ip
    np.testing.assert_allclose(A, 0.3 * J.T @ J, atol=1e-12 * np.abs(A).max())
    np.testing.assert_allclose(b, 0.3 * J.T @ rho, atol=1e-12 * np.abs(b).max())
    assert np.array_equal(cref.reference_update(q, q, n, d, Iq, Iq, 0.5, ct, s), np.eye(4))
    e = np.zeros((0, 3))
    assert np.array_equal(cref.reference_update(e, e, e, e, Iq[:0], Iq[:0], 0.5, ct, s), np.eye(4))


def test_pairs_of_keeps_the_source_index_of_every_pair():
    src, Ip, tgt, nrm, Iq, grad, r, inits, _ = cfx.margin_fixture()
    from scipy.spatial import cKDTree
    s64, t64 = src.astype(np.float64), tgt.astype(np.float64)
    for T0 in inits:
        _, _, xs, idx, sel = cref.pairs_of(cKDTree(t64), t64, s64, np.array(T0), r)
        want_x, si, ti = cfx.first_pairs(src, tgt, T0, r)
        assert np.array_equal(sel, si) and np.array_equal(idx, ti) and np.array_equal(xs, want_x)


# ---- fixture conditions, asserted again by the GPU tests ----

def test_attributes_are_fp32_and_differ_per_point():
    Iq, grad = cfx.aggregate_target_attributes()
    n = pfx.aggregate_normals().astype(np.float64)
    assert Iq.dtype == grad.dtype == np.float32 and 0.0 <= Iq.min() and Iq.max() <= 1.0
    length = np.linalg.norm(grad.astype(np.float64), axis=1)
    assert length.min() >= 0.5 * (1 - 1e-6) and length.max() <= 4.0 * (1 + 1e-6)
    assert np.abs((grad.astype(np.float64) * n).sum(axis=1)).max() <= 1e-6 * 4.0          # tangent, to fp32 rounding
    for Ip in (cfx.aggregate_source_intensity(4097), cfx.margin_fixture()[1], cfx.rank_deficient("planar")[1]):
        assert Ip.dtype == np.float32 and len(np.unique(Ip)) >= 0.99 * len(Ip)


@pytest.mark.parametrize("ns", fx.AGGREGATE_NS)
def test_aggregate_fixture_conditions(ns):
    src, tgt, r, inits, pairs = fx.aggregate_fixture(ns)
    Ip, (Iq, grad), nrm = cfx.aggregate_source_intensity(ns), cfx.aggregate_target_attributes(), pfx.aggregate_normals()
    ct, s = pref.frame(tgt)
    extent = float(np.ptp(tgt.astype(np.float64), axis=0).max())
    rng = np.random.default_rng(0)
    for lam in cfx.LAMBDAS:
        for j, T0 in enumerate(inits):
            p = cfx.first_pass(src, Ip, tgt, nrm, Iq, grad, r, T0)
            assert len(p[0]) == pairs[j][0].sum()
            _, eig = cref.reference_update(*p, lam, ct, s, return_eig=True)
            assert pref.eig_ratios_clear([eig])
            _, bound, own = cfx.one_update_bound(p, lam, ct, s, T0, extent, rng)
            print(f"ns {ns} lambda {lam} init {j}: order sensitivity {own:.3g}, bound {bound:.3g}")


def test_margin_fixture_conditions():
    src, Ip, tgt, nrm, Iq, grad, r, inits, runs = cfx.margin_fixture()
    assert len(inits) == 3 and set(runs) == set(cfx.LAMBDAS)
    for lam, ys in runs.items():
        assert all(len(y["poses"]) == cfx.RUN_UPDATES + 1 for y in ys)
        assert pfx.poses_have_margin(src, tgt, [T for y in ys for T in y["poses"]], r)
        assert all(pref.eig_ratios_clear(y["eigenvalues"]) for y in ys)
        assert all(min(y["passes"]) > 100 for y in ys)
        print(f"lambda {lam}: pairs per pass {[y['passes'] for y in ys]}")
    # the colour term matters: at lambda 0.5 the first step differs from point-to-plane's by far more than any bound
    y0 = pref.registration_icp(src, tgt, nrm, r, inits[0], max_iteration=1, relative_fitness=0.0, relative_rmse=0.0)
    assert np.abs(runs[0.5][0]["poses"][1] - y0["poses"][1]).max() > 1e-4


def test_a_gather_through_the_wrong_order_is_visible():
    """The step with the source intensities in another order is off by more than 1 000x the one-update bound."""
    src, Ip, tgt, nrm, Iq, grad, r, inits, _ = cfx.margin_fixture()
    ct, s = pref.frame(tgt)
    extent = float(np.ptp(tgt.astype(np.float64), axis=0).max())
    wrong = np.array(Ip)[np.random.default_rng(1).permutation(len(Ip))]
    for lam in cfx.LAMBDAS:
        p = cfx.first_pass(src, Ip, tgt, nrm, Iq, grad, r, inits[0])
        want, bound, _ = cfx.one_update_bound(p, lam, ct, s, inits[0], extent, np.random.default_rng(0))
        off = float(np.abs(cref.reference_update(*cfx.first_pass(src, wrong, tgt, nrm, Iq, grad, r, inits[0]), lam, ct, s)
                           @ inits[0] - want).max())
        print(f"lambda {lam}: shuffled source intensities move the step by {off:.3g}, bound {bound:.3g}")
        assert off > 1000.0 * bound


def test_quarter_zero_fixture_conditions():
    src, _, tgt, _, Iq, _, r, inits, _ = cfx.margin_fixture()
    Ip, nrm, grad, no_normal, no_gradient = cfx.quarter_zero()
    assert len(no_normal) == len(no_gradient) == len(tgt) // 4 and not np.isin(no_normal, no_gradient).any()
    ct, s = pref.frame(tgt)
    for T0 in inits:
        xs, si, ti = cfx.first_pairs(src, tgt, T0, r)
        a, b = np.isin(ti, no_normal), np.isin(ti, no_gradient)
        assert a.sum() > 30 and b.sum() > 30
        assert not nrm[ti[a]].any() and not grad[ti[b]].any() and np.array_equal(Ip[si[b]], Iq[ti[b]])
        for lam in cfx.LAMBDAS:
            _, eig = cref.reference_update(*cfx.first_pass(src, Ip, tgt, nrm, Iq, grad, r, T0), lam, ct, s, return_eig=True)
            assert pref.eig_ratios_clear([eig])


@pytest.mark.parametrize("name", cfx.RANK_DEFICIENT)
def test_rank_deficient_fixture_conditions(name):
    src, Ip, tgt, nrm, Iq, grad, r, y = cfx.rank_deficient(name)
    if name != "identical64":
        assert pfx.poses_have_margin(src, tgt, y["poses"], r)
    assert pref.eig_ratios_clear(y["eigenvalues"])
    eig = y["eigenvalues"][0]
    # one pair constrains the motion along its normal and along its gradient; several x at one q with one normal and one
    # gradient leave the translation along n cross d free; the planar target's tangent gradients fix what its normals leave
    assert int((eig > 1e-12 * eig.max()).sum()) == {"one_source_point": 2, "one_pair": 2, "identical64": 5, "planar": 6}[name]
    assert y["passes"][0] == {"one_source_point": 1, "one_pair": 1}.get(name, len(src))
    U = y["poses"][1]
    assert np.isfinite(U).all() and np.linalg.det(U[:3, :3]) == pytest.approx(1.0, abs=1e-9)


def test_textured_sheet_conditions():
    s = cfx.textured_sheet()
    src, tgt = s["source"], s["target"]
    assert len(tgt) == 1600 and len(src) == 900
    ep = cfx.rms_alignment_error(s["plane"]["transformation"], src)
    for lam, y in s["colored"].items():
        ec = cfx.rms_alignment_error(y["transformation"], src)
        print(f"textured sheet (seed {s['seed']}), lambda {lam}: start {s['start']:.3g}, coloured {ec:.3g} in {y['iterations']} updates, "
              f"point-to-plane {ep:.3g} in {s['plane']['iterations']}")
        assert ec < 0.1 * ep and y["iterations"] < cfx.SHEET_MAX_ITERATION
        assert pfx.poses_have_margin(src, tgt, y["poses"], s["r"], relative=False)
        assert pref.eig_ratios_clear(y["eigenvalues"])
    assert np.abs((s["gradients"].astype(np.float64) * s["normals"].astype(np.float64)).sum(axis=1)).max() <= 1e-5


# ---- the gradient rule ----

@pytest.mark.parametrize("name", cfx.GRADIENTS)
def test_gradient_fixture_conditions(name):
    f = cfx.gradient_fixture(name)
    assert np.mean(~f["margin"]) <= cfx.MARGIN_CAP
    assert _ratios_clear(f["eigenvalues"])
    assert f["neighbors"].dtype == np.int32 and f["neighbors"].shape == (len(f["rows"]), f["knn"])
    d, n = f["gradients"], f["normals"][f["rows"]].astype(np.float64)
    assert np.abs((d * n).sum(axis=1)).max() <= 1e-6 * max(1.0, np.abs(d).max())           # tangent (fp32 normals)
    print(f"{name}: {len(f['rows'])} rows, {np.mean(~f['margin']):.4f} without the neighbour margin, order sensitivity up to "
          f"{f['sensitivity'].max():.3g}, largest component {np.abs(d).max():.3g}")


def test_gradient_rule_on_the_exact_clouds():
    f = cfx.gradient_fixture("plane_linear")
    off = float(np.abs(f["gradients"] - f["slope"] * [1.0, 1.0, 0.0]).max())
    print(f"linear intensity on a plane: |d - tangential slope| {off:.3g}")
    assert off <= 1e-13
    f = cfx.gradient_fixture("line")
    off = float(np.abs(f["gradients"] - f["axis"] * (f["axis"] @ f["slope"])).max())
    print(f"linear intensity on a line: |d - its component along the line| {off:.3g}")
    assert off <= 1e-13
    f = cfx.gradient_fixture("one_neighbour")
    assert not f["gradients"].any()                                     # fewer than two neighbours: zero
    f = cfx.gradient_fixture("knn_over_n")
    assert (f["neighbors"][:, 20:] == -1).all() and (f["neighbors"][:, :20] >= 0).all() and f["gradients"].any()
    # a zero or non-finite normal projects nothing out: the plain least-squares gradient in 3-D
    pts, inten, nb = f["points"], f["intensity"], f["neighbors"]
    for bad in (0.0, np.nan, np.inf):
        d = cref.color_gradients(pts, np.full((20, 3), bad), inten, nb)
        u = pts[1:].astype(np.float64) - pts[0].astype(np.float64)
        want = np.linalg.lstsq(u.T @ u, u.T @ (inten[1:].astype(np.float64) - float(inten[0])), rcond=None)[0]
        np.testing.assert_allclose(d[0], want, rtol=1e-9)


# ---- the package, without a device ----

def test_estimation_is_registered_and_the_header_declares_the_entry_points():
    from scorp_amd import _C, icp
    assert "colored" in icp.ESTIMATIONS and icp.ESTIMATIONS[:3] == ("point_to_point", "point_to_plane", "generalized")
    for name in ("scorp_icp_colored", "scorp_icp_colored_workspace_bytes", "scorp_color_gradients"):
        assert name in _C.FUNCTIONS, name
    assert len(_C.FUNCTIONS["scorp_icp_colored"][1]) == len(_C.FUNCTIONS["scorp_icp_point_to_plane"][1]) + 4


def test_argument_errors_that_need_no_device():
    from scorp_amd import icp
    src, Ip, tgt, nrm, Iq, grad, r, inits, _ = cfx.margin_fixture()
    with pytest.raises(ValueError, match="source_colors and target_colors"):
        icp.registration_icp(src, tgt, r, inits, estimation="colored")
    with pytest.raises(ValueError, match="source_colors and target_colors"):
        icp.registration_icp(src, tgt, r, inits, estimation="colored", source_colors=Ip)
    for lam in (-0.1, 1.5, np.nan, np.inf):
        with pytest.raises(ValueError, match="lambda_geometric"):
            icp.registration_icp(src, tgt, r, inits, estimation="colored", source_colors=Ip, target_colors=Iq, lambda_geometric=lam)
    with pytest.raises(ValueError, match="target_gradients"):
        icp.registration_icp(src, tgt, r, inits, estimation="colored", source_colors=Ip, target_colors=Iq, target_gradients=grad[:-1])
    bad = np.array(grad)
    bad[3, 1] = np.nan
    with pytest.raises(ValueError, match="target_gradients"):
        icp.registration_icp(src, tgt, r, inits, estimation="colored", source_colors=Ip, target_colors=Iq, target_gradients=bad)
    for wrong in (np.zeros((5, 2)), np.zeros((5, 3, 1)), np.float32(0.5)):
        with pytest.raises(ValueError, match="colors must be"):
            icp.intensities(wrong)
    with pytest.raises(ValueError, match="NaN"):
        icp.intensities(np.array([0.1, np.nan]))
    with pytest.raises(ValueError, match="knn"):
        icp.estimate_color_gradients(tgt, Iq, knn=2)
    rots = np.tile(np.eye(3), (2, 1, 1))
    with pytest.raises(ValueError, match="source_colors"):
        icp.get_ICP_fitting_transformation_best(np.array(tgt), np.array(src), rots, r, estimation="colored",
                                                source_colors=np.array(Ip)[:-1], target_colors=np.array(Iq))


def test_the_fpfh_route_refuses_the_estimation_it_has_no_colours_for():
    from scorp_amd.global_registration import get_FPFH_fitting_transformation
    pts = np.random.default_rng(0).random((50, 3))
    with pytest.raises(ValueError, match="colours"):
        get_FPFH_fitting_transformation(pts, pts, 0.1, estimation="colored")


def test_model_colors():
    from scorp_amd import icp
    from scorp_amd.sh import C0

    class Model:                       # what model_colors reads of either model kind
        def __init__(self, dc):
            self._features_dc = dc

    dc = torch.tensor(np.random.default_rng(2).normal(scale=2.0, size=(40, 1, 3)), dtype=torch.float32)
    c = icp.model_colors(Model(dc))
    assert c.shape == (40, 3) and c.dtype == torch.float32 and 0.0 <= float(c.min()) and float(c.max()) <= 1.0
    want = np.clip(0.5 + np.float32(C0) * dc[:, 0, :].numpy(), 0.0, 1.0)
    np.testing.assert_allclose(c.numpy(), want, atol=1e-7)
    assert (c == 0.0).any() and (c == 1.0).any() and ((c > 0.0) & (c < 1.0)).any()
