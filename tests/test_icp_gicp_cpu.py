"""The generalized ICP yardstick (tests/icp_gicp_reference.py), the properties of every fixture the GPU tests rely on
(tests/icp_gicp_fixtures.py), shown with the float64 reference alone, and the pure-torch covariance helpers of
scorp_amd/icp.py.  No GPU."""
import numpy as np
import pytest
import torch

from tests import icp_gicp_fixtures as gfx
from tests import icp_gicp_reference as gref
from tests import icp_plane_fixtures as pfx
from tests import icp_plane_reference as pref
from tests import icp_probe_fixtures as fx
from tests.icp_gicp_fixtures import first_pass, one_update_bound


# ---- the update, on the yardstick alone ----

def test_projector_weights_give_the_point_to_plane_sums():
    """W = n n^T: A and b are icp_plane_reference.system's, term for term."""
    rng = np.random.default_rng(4)
    q = rng.normal(size=(200, 3)) + (3.0, -2.0, 1.0)
    x = q + rng.normal(scale=0.02, size=q.shape)
    n = pfx.unit_normals(200, 5).astype(np.float64)
    ct, s = pref.frame(q)
    A0, b0 = pref.system(x, q, n, ct, s)
    A1, b1 = gref.system(x, q, None, None, ct, s, W=n[:, :, None] * n[:, None, :])
    assert np.abs(A1 - A0).max() <= 1e-12 * np.abs(A0).max()
    assert np.abs(b1 - b0).max() <= 1e-12 * np.abs(b0).max()
    U0 = pref.reference_update(x, q, n, ct, s)
    U1 = gref.reference_update(x, q, None, None, ct, s, W=n[:, :, None] * n[:, None, :])
    np.testing.assert_allclose(U1, U0, atol=1e-13)


def test_coincident_pairs_give_the_identity_exactly():
    rng = np.random.default_rng(6)
    q = rng.normal(size=(50, 3))
    C = gref.unpack(gfx.random_spd(50, 1))
    ct, s = pref.frame(q)
    assert np.array_equal(gref.reference_update(q, q, C, C, ct, s), np.eye(4))
    e = np.zeros((0, 3))
    assert np.array_equal(gref.reference_update(e, e, C[:0], C[:0], ct, s), np.eye(4))


def test_pairs_without_a_positive_definite_sum_add_nothing():
    rng = np.random.default_rng(7)
    q = rng.normal(size=(60, 3))
    x = q + rng.normal(scale=0.02, size=q.shape)
    Cp, Cq = gref.unpack(gfx.random_spd(60, 2)), gref.unpack(gfx.random_spd(60, 3))
    ct, s = pref.frame(q)
    want = gref.reference_update(x[20:], q[20:], Cp[20:], Cq[20:], ct, s)
    Cp[:10], Cq[:10] = 0.0, 0.0                                  # M = 0
    Cq[10:15, 0, 0] = -10.0                                       # M00 < 0
    Cp[15:20] = np.nan
    assert not gref.positive_definite(Cp + Cq)[:20].any() and gref.positive_definite(Cp + Cq)[20:].all()
    assert np.array_equal(gref.reference_update(x, q, Cp, Cq, ct, s), want)
    # every covariance zero: A = 0, l_max = 0, the identity
    src, _, tgt, _, r, inits, _ = gfx.margin_fixture()
    z = np.zeros((len(src), 6)), np.zeros((len(tgt), 6))
    y = gref.registration_icp(src, tgt, z[0], z[1], r, inits[0], max_iteration=2)
    assert y["fitness"] > 0.5 and np.array_equal(y["transformation"], inits[0])


def test_update_lowers_the_generalized_residual():
    rng = np.random.default_rng(8)
    q = rng.normal(size=(120, 3))
    x = q @ pref.rotation_zyx([0.01, -0.02, 0.015]).T + (0.01, 0.02, -0.01)
    Cp, Cq = gref.unpack(gfx.random_spd(120, 4)), gref.unpack(gfx.random_spd(120, 5))
    ct, s = pref.frame(q)
    U = gref.reference_update(x, q, Cp, Cq, ct, s)
    W = np.linalg.inv(Cp + Cq)
    cost = lambda p: float(np.einsum("na,nab,nb->", p - q, W, p - q))
    assert cost(x @ U[:3, :3].T + U[:3, 3]) < 0.01 * cost(x)
    assert np.linalg.det(U[:3, :3]) == pytest.approx(1.0, abs=1e-12)


# ---- fixture conditions, asserted again by the GPU tests ----

def test_source_covariances_differ_per_point_and_are_well_conditioned():
    for c6 in (gfx.aggregate_source_covariances(4097), gfx.margin_fixture()[1], gfx.rank_deficient("one_pair")[1]):
        assert c6.dtype == np.float32 and c6.shape[1] == 6
        assert len(np.unique(c6, axis=0)) == len(c6)
        cond = gfx.condition_numbers(c6)
        assert (np.linalg.eigvalsh(gref.unpack(c6))[:, 0] > 0).all() and cond.max() <= gfx.CONDITION_CAP
    Cq = gfx.aggregate_target_covariances()
    n = pfx.aggregate_normals().astype(np.float64)
    np.testing.assert_allclose(np.einsum("na,nab,nb->n", n, gref.unpack(Cq), n), gfx.EPSILON, rtol=1e-3)


@pytest.mark.parametrize("ns", fx.AGGREGATE_NS)
def test_aggregate_fixture_conditions(ns):
    src, tgt, r, inits, pairs = fx.aggregate_fixture(ns)
    Cp, Cq = gfx.aggregate_source_covariances(ns), gfx.aggregate_target_covariances()
    ct, s = pref.frame(tgt)
    extent = float(np.ptp(tgt.astype(np.float64), axis=0).max())
    rng = np.random.default_rng(0)
    for j, T0 in enumerate(inits):
        xs, qs, Cs, Ct = first_pass(src, Cp, tgt, Cq, r, T0)
        assert len(xs) == pairs[j][0].sum()
        _, lam = gref.reference_update(xs, qs, Cs, Ct, ct, s, return_eig=True)
        assert pref.eig_ratios_clear([lam])
        _, bound, own, inv = one_update_bound(xs, qs, Cs, Ct, ct, s, T0, extent, rng)
        print(f"ns {ns} init {j}: order sensitivity {own:.3g}, cofactor against numpy inverse {inv:.3g}, bound {bound:.3g}")


def test_margin_fixture_conditions():
    src, Cp, tgt, Cq, r, inits, runs = gfx.margin_fixture()
    assert len(inits) == 3 and all(len(y["poses"]) == gfx.RUN_UPDATES + 1 for y in runs)
    assert all(gfx.rotation_angle_degrees(T[:3, :3]) >= 30.0 for T in inits)
    assert pfx.poses_have_margin(src, tgt, [T for y in runs for T in y["poses"]], r)
    assert all(pref.eig_ratios_clear(y["eigenvalues"]) for y in runs)
    assert all(min(y["passes"]) > 100 for y in runs)


def test_leaving_the_source_covariances_unrotated_is_visible():
    """At the rotated inits the step with C_p in place of A_T C_p A_T^T is off by more than 1 000x the one-update bound."""
    src, Cp, tgt, Cq, r, inits, _ = gfx.margin_fixture()
    ct, s = pref.frame(tgt)
    extent = float(np.ptp(tgt.astype(np.float64), axis=0).max())
    for j, T0 in enumerate(inits):
        xs, qs, Cs, Ct = first_pass(src, Cp, tgt, Cq, r, T0)
        want, bound, _, _ = one_update_bound(xs, qs, Cs, Ct, ct, s, T0, extent, np.random.default_rng(0))
        xs, qs, Cu, Ct = first_pass(src, Cp, tgt, Cq, r, T0, rotate_source=False)
        off = float(np.abs(gref.reference_update(xs, qs, Cu, Ct, ct, s) @ T0 - want).max())
        print(f"init {j}: unrotated C_p moves the step by {off:.3g}, bound {bound:.3g}")
        assert off > 1000.0 * bound


def test_quarter_zero_fixture_conditions():
    src, _, tgt, _, r, inits, _ = gfx.margin_fixture()
    Cp, Cq, hit = gfx.quarter_zero()
    ct, s = pref.frame(tgt)
    for j, T0 in enumerate(inits):
        xs, qs, Cs, Ct = first_pass(src, Cp, tgt, Cq, r, T0)
        bad = ~gref.positive_definite(Cs + Ct)
        assert bad.sum() == len(hit[j]) > 30 and not np.abs((Cs + Ct)[bad]).any()
        _, lam = gref.reference_update(xs, qs, Cs, Ct, ct, s, return_eig=True)
        assert pref.eig_ratios_clear([lam])


@pytest.mark.parametrize("name", gfx.RANK_DEFICIENT)
def test_rank_deficient_fixture_conditions(name):
    src, Cp, tgt, Cq, r, y = gfx.rank_deficient(name)
    if name != "identical64":
        assert pfx.poses_have_margin(src, tgt, y["poses"], r)
    assert pref.eig_ratios_clear(y["eigenvalues"])
    lam = y["eigenvalues"][0]
    # one pair with a positive definite W constrains the three translations; several x at one q all six
    assert int((lam > 1e-12 * lam.max()).sum()) == {"one_source_point": 3, "one_pair": 3, "identical64": 6}[name]
    assert y["passes"][0] == {"one_source_point": 1, "one_pair": 1}.get(name, len(src))
    U = y["poses"][1]
    assert np.isfinite(U).all() and np.linalg.det(U[:3, :3]) == pytest.approx(1.0, abs=1e-9)


def test_planted_pose_is_reached_from_both_starts():
    p = gfx.planted()
    counts = []
    for src, Cp, T0, want, y in p["starts"]:
        T = y["transformation"]
        assert np.abs(T - want)[:3].max() < 0.02
        assert y["iterations"] < pfx.PLANTED_MAX_ITERATION and pref.eig_ratios_clear(y["eigenvalues"])
        counts.append(y["iterations"])
    assert gfx.rotation_angle_degrees(p["starts"][1][2][:3, :3]) >= 30.0
    print(f"planted pose: generalized {counts} updates, point-to-plane {p['plane']['iterations']}, point-to-point "
          f"{p['point']['iterations']}")
    assert counts[0] <= p["plane"]["iterations"] < p["point"]["iterations"]


def test_cofactor_and_numpy_inverse_agree_on_every_fixture():
    src, Cp, tgt, Cq, r, inits, _ = gfx.margin_fixture()
    cases = [("margin", src, Cp, tgt, Cq, r, inits[0], gfx.RUN_UPDATES)]
    for name in gfx.RANK_DEFICIENT:
        s_, cp, t_, cq, r_, _ = gfx.rank_deficient(name)
        cases.append((name, s_, cp, t_, cq, r_, np.eye(4), 1))
    p = gfx.planted()
    s_, cp, T0, _, _ = p["starts"][1]
    cases.append(("planted, rotated start", s_, cp, p["target"], p["target_covariances"], p["r"], T0, 3))
    for name, s_, cp, t_, cq, r_, T0, n in cases:
        a = gref.registration_icp(s_, t_, cp, cq, r_, T0, max_iteration=n, relative_fitness=0.0, relative_rmse=0.0)
        b = gref.registration_icp(s_, t_, cp, cq, r_, T0, max_iteration=n, relative_fitness=0.0, relative_rmse=0.0, inverse="numpy")
        d = float(np.abs(a["transformation"] - b["transformation"]).max())
        print(f"{name}: {n} updates, cofactor against numpy inverse {d:.3g}")
        # the same rule twice: an inverse good to 1e-16 cond(M) <= 2e-13, times the conditioning of the 6x6 (64 identical
        # points leave the rotation to a cluster 0.02 wide).  The GPU tests take their bound from the measured value.
        assert d <= 1e-9


# ---- the pure-torch helpers ----

def test_covariances_from_normals():
    from scorp_amd import icp
    n = pfx.unit_normals(100, 1)
    C = icp.covariances_from_normals(torch.tensor(np.array(n)))
    assert C.shape == (100, 6) and C.dtype == torch.float32 and C.device.type == "cpu"
    assert np.array_equal(C.numpy(), gfx.covariances_of_normals(n))
    assert np.array_equal(icp.covariances_from_normals(np.array(n)).numpy(), C.numpy())
    assert np.array_equal(icp.covariances_from_normals(n, epsilon=0.25).numpy(), gfx.covariances_of_normals(n, 0.25))
    zero = icp.covariances_from_normals(torch.zeros(2, 3))
    assert np.array_equal(zero.numpy(), np.tile([1.0, 0.0, 0.0, 1.0, 0.0, 1.0], (2, 1)).astype(np.float32))
    lam = np.linalg.eigvalsh(gref.unpack(C.numpy()))
    np.testing.assert_allclose(lam, np.tile([1e-3, 1.0, 1.0], (100, 1)), rtol=1e-4)
    with pytest.raises(ValueError):
        icp.covariances_from_normals(torch.zeros(4, 2))


def test_covariance_arguments_are_packed_and_checked():
    from scorp_amd import icp
    c6 = gfx.random_spd(20, 3)
    full = gref.unpack(c6).astype(np.float32)
    cpu = torch.device("cpu")
    assert np.array_equal(icp._covariances("c", full, 20, cpu).numpy(), c6)
    assert np.array_equal(icp._covariances("c", torch.tensor(full), 20, cpu).numpy(), c6)
    assert np.array_equal(icp._covariances("c", np.array(c6), 20, cpu).numpy(), c6)
    bad = full.copy()
    bad[3, 0, 1] += 1e-3 * np.abs(bad[3]).max()
    with pytest.raises(ValueError, match="symmetric"):
        icp._covariances("c", bad, 20, cpu)
    for wrong in (full[:19], c6[:19], np.zeros((20, 5), np.float32)):
        with pytest.raises(ValueError, match="must be"):
            icp._covariances("c", wrong, 20, cpu)
    for v in (np.nan, np.inf):
        bad = np.array(c6)
        bad[5, 2] = v
        with pytest.raises(ValueError):
            icp._covariances("c", bad, 20, cpu)
    assert "generalized" in icp.ESTIMATIONS


def test_model_covariances_full_mode_caps_the_condition_number():
    from scorp_amd import icp

    class Model:                       # what model_covariances reads of a GaussianModel
        def __init__(self, scales, rot):
            self._scaling, self._rotation = torch.log(scales), rot

        @property
        def get_scaling(self):
            return torch.exp(self._scaling)

    rng = np.random.default_rng(2)
    rot = torch.tensor(rng.normal(size=(50, 4)))
    scales = torch.tensor(10.0 ** rng.uniform(-4, 0, (50, 3)))
    from scorp_amd.gaussian_model import build_rotation
    R = build_rotation(rot).numpy()
    for cols in (3, 2):                # a surfel model brings two scales
        C = icp.model_covariances(Model(scales[:, :cols], rot), mode="full")
        assert C.shape == (50, 6) and C.dtype == torch.float32
        var = np.zeros((50, 3))
        var[:, :cols] = scales[:, :cols].numpy() ** 2
        var = np.maximum(var, 1e-3 * var.max(axis=1, keepdims=True))
        want = np.einsum("nab,nb,ncb->nac", R, var, R)
        np.testing.assert_allclose(gref.unpack(C.numpy()), want, rtol=1e-5, atol=1e-7 * want.max())
        assert gfx.condition_numbers(C.numpy()).max() <= 1e3 * (1 + 1e-3)
    with pytest.raises(ValueError):
        icp.model_covariances(Model(scales, rot), mode="other")
