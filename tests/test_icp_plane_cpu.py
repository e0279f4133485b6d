"""The point-to-plane yardstick (tests/icp_plane_reference.py), the properties of every fixture the GPU tests rely on
(tests/icp_plane_fixtures.py), shown with the float64 reference alone, and the host side of scorp_amd/icp.py that runs
before the library is touched.  No GPU."""
import numpy as np
import pytest
import torch

from tests import icp_plane_fixtures as pfx
from tests import icp_plane_reference as pref
from tests import icp_probe_fixtures as fx
from tests import icp_reference as ref


# ---- update and convergence, on the yardstick alone ----

def test_update_is_the_identity_without_pairs():
    e = np.zeros((0, 3))
    assert np.array_equal(pref.reference_update(e, e, e, np.array([1.0, 2.0, 3.0]), 0.5), np.eye(4))
    tgt = np.random.default_rng(0).random((50, 3))
    y = pref.registration_icp(tgt + 5.0, tgt, pfx.unit_normals(50, 0), 0.01, np.eye(4), max_iteration=3)
    assert y["fitness"] == 0.0 and y["passes"] == [0, 0] and np.array_equal(y["transformation"], np.eye(4))
    # zero normals: A = 0, l_max = 0, the identity as well
    y = pref.registration_icp(tgt + 0.001, tgt, np.zeros((50, 3)), 0.1, np.eye(4), max_iteration=2)
    assert y["fitness"] == 1.0 and np.array_equal(y["transformation"], np.eye(4))


def test_update_solves_the_linearised_problem():
    """Against a direct least-squares solve of min sum (rho + J . xi)^2 on a full-rank system."""
    rng = np.random.default_rng(2)
    q = rng.normal(size=(80, 3))
    n = pfx.unit_normals(80, 3).astype(np.float64)
    x = q @ pref.rotation_zyx([0.01, -0.02, 0.015]).T + (0.01, 0.02, -0.01)      # a small rigid move of the target
    ct, s = pref.frame(q)
    A, b = pref.system(x, q, n, ct, s)
    xi, lam = pref.min_norm_step(A, b)
    J = np.hstack([np.cross(x - ct, n) / s, n])
    direct = np.linalg.lstsq(J, -(n * (x - q)).sum(axis=1), rcond=None)[0]
    np.testing.assert_allclose(xi, direct, atol=1e-12)
    U = pref.reference_update(x, q, n, ct, s)
    assert np.linalg.det(U[:3, :3]) == pytest.approx(1.0, abs=1e-12)
    np.testing.assert_allclose(U[:3, :3], pref.rotation_zyx(xi[:3] / s), atol=0)
    # the update lowers the point-to-plane residual
    x2 = x @ U[:3, :3].T + U[:3, 3]
    assert ((n * (x2 - q)).sum(axis=1) ** 2).sum() < 0.01 * ((n * (x - q)).sum(axis=1) ** 2).sum()


def test_planted_pose_in_fewer_updates_than_point_to_point():
    src, tgt, nrm, r, R0, t0, yp, y2 = pfx.planted()
    T = yp["transformation"]
    print(f"planted pose: point-to-plane {yp['iterations']} updates (rmse {yp['inlier_rmse']:.3g}), point-to-point "
          f"{y2['iterations']} (rmse {y2['inlier_rmse']:.3g})")
    assert np.abs(T[:3, :3] - R0).max() < 0.02 and np.abs(T[:3, 3] - t0).max() < 0.02
    assert yp["iterations"] < y2["iterations"] < pfx.PLANTED_MAX_ITERATION
    assert yp["fitness"] == 1.0
    a = np.arccos(np.clip((np.trace(R0) - 1) / 2, -1, 1))
    assert np.rad2deg(a) == pytest.approx(5.0) and np.linalg.norm(t0) == pytest.approx(0.02 * np.ptp(tgt, axis=0).max())
    assert pref.eig_ratios_clear(yp["eigenvalues"])


def test_planar_target_moves_only_along_its_normal():
    src, tgt, nrm, r, y = pfx.rank_deficient("planar")
    assert (tgt[:, 2] == 0).all() and (nrm == (0, 0, 1)).all()
    U = y["poses"][1]                                       # T after one update from the identity
    assert np.abs(U[:2, 3]).max() <= 1e-12 and np.abs(U[:3, :3] - np.eye(3)).max() <= 1e-12
    assert U[2, 3] == pytest.approx(-float(src[0, 2]), abs=1e-9)        # the z offset is removed
    lam = y["eigenvalues"][0]
    assert (lam > 1e-12 * lam.max()).sum() == 3              # rotation about x and y, translation along z


# ---- fixture conditions, asserted again by the GPU tests ----

@pytest.mark.parametrize("ns", fx.AGGREGATE_NS)
def test_aggregate_fixture_conditions(ns):
    src, tgt, r, inits, pairs = fx.aggregate_fixture(ns)
    nrm = pfx.aggregate_normals()
    assert nrm.shape == tgt.shape and nrm.dtype == np.float32
    np.testing.assert_allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-6)
    assert pfx.poses_have_margin(src, tgt, list(inits), r, relative=False)
    ct, s = pref.frame(tgt)
    for T0, (hit, idx) in zip(inits, pairs):
        x = src.astype(np.float64) @ T0[:3, :3].T + T0[:3, 3]
        _, lam = pref.reference_update(x[hit], tgt[idx[hit]], nrm[idx[hit]], ct, s, return_eig=True)
        assert pref.eig_ratios_clear([lam])


def test_margin_fixture_conditions():
    src, tgt, nrm, r, inits, runs = pfx.margin_fixture()
    assert len(inits) == 3 and all(len(y["poses"]) == pfx.RUN_UPDATES + 1 for y in runs)
    assert pfx.poses_have_margin(src, tgt, [T for y in runs for T in y["poses"]], r)
    assert all(pref.eig_ratios_clear(y["eigenvalues"]) for y in runs)
    assert all(min(y["passes"]) > 100 for y in runs)


@pytest.mark.parametrize("name", sorted(pfx.RANK_DEFICIENT))
def test_rank_deficient_fixture_conditions(name):
    src, tgt, nrm, r, y = pfx.rank_deficient(name)
    if name != "identical64":
        assert pfx.poses_have_margin(src, tgt, y["poses"], r)
    assert pref.eig_ratios_clear(y["eigenvalues"])
    lam = y["eigenvalues"][0]
    rank = int((lam > 1e-12 * lam.max()).sum())
    # (one normal, several x: the translation along it and the rotations about the two axes across it)
    assert rank == {"planar": 3, "one_source_point": 1, "one_pair": 1, "identical64": 3}[name]
    assert y["passes"][0] == {"one_source_point": 1, "one_pair": 1}.get(name, len(src))
    U = y["poses"][1]
    assert np.isfinite(U).all() and np.linalg.det(U[:3, :3]) == pytest.approx(1.0, abs=1e-9)


@pytest.mark.parametrize("name", sorted(pfx.NORMALS))
def test_normals_fixture_stays_under_the_cap(name):
    f = pfx.normals_fixture(name)
    n, k = len(f["points"]), min(f["knn"], len(f["points"]))
    assert f["idx"].shape == (len(f["rows"]), k) and (f["idx"][:, 0] == f["rows"]).all()      # itself first: d^2 = 0
    lack_margin, lack_gap = float(np.mean(~f["margin"])), float(np.mean(~f["gap"]))
    print(f"{name}: n {n}, k {k}, {lack_margin:.4f} without the neighbour margin, {lack_gap:.4f} without margin or eigen-gap")
    assert lack_margin <= pfx.MARGIN_CAP and lack_gap <= pfx.MARGIN_CAP
    np.testing.assert_allclose(np.linalg.norm(f["normals"], axis=1), 1.0, atol=1e-12)
    assert (np.take_along_axis(f["normals"], np.abs(f["normals"]).argmax(axis=1)[:, None], axis=1) > 0).all()


def test_knn_brute_force_orders_ties_by_index():
    tgt, _, _, _, _ = fx.ties_fixture(0)
    idx, dk, dk1 = pref.knn_brute(tgt, 7)
    d2 = ((tgt[idx].astype(np.float64) - tgt[:, None, :].astype(np.float64)) ** 2).sum(axis=2)
    assert (np.diff(d2, axis=1) >= 0).all()
    tied = np.diff(d2, axis=1) == 0
    assert tied.any() and (np.diff(idx, axis=1)[tied] > 0).all()


def test_normals_yardstick_on_a_plane_and_tiny_clouds():
    rng = np.random.default_rng(0)
    p = np.column_stack([rng.random((200, 2)), np.full(200, 0.25)])
    np.testing.assert_allclose(pref.estimate_normals(p, 10), np.tile([0, 0, 1.0], (200, 1)), atol=1e-12)
    for n in (1, 2):
        assert np.array_equal(pref.estimate_normals(p[:n], 30), np.tile([0, 0, 1.0], (n, 1)))


# ---- the front end, before the library is touched ----

@pytest.fixture
def no_device(monkeypatch):
    from scorp_amd import _C

    def touched(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_C, "lib", touched)


def test_front_end_argument_errors(no_device):
    from scorp_amd import icp
    p = np.random.default_rng(0).random((20, 3)).astype(np.float32)
    n = pfx.unit_normals(20, 0)
    with pytest.raises(ValueError, match="estimation"):
        icp.registration_icp(p, p, 0.1, np.eye(4), estimation="point_to_line")
    with pytest.raises(ValueError, match="estimation"):
        icp.get_ICP_fitting_transformation_best(p, p, np.eye(3)[None], 0.1, estimation="plane")
    with pytest.raises(ValueError, match="shape"):
        icp.registration_icp(p, p, 0.1, np.eye(4), estimation="point_to_plane", target_normals=n[:19])
    with pytest.raises(ValueError, match="shape"):
        icp.registration_icp(p, p, 0.1, np.eye(4), estimation="point_to_plane", target_normals=n[:, :2])
    for bad, word in ((np.nan, "NaN"), (np.inf, "Inf"), (-np.inf, "Inf")):
        m = np.array(n)
        m[3, 1] = bad
        with pytest.raises(ValueError, match=f"target_normals contains {word} values"):
            icp.registration_icp(p, p, 0.1, np.eye(4), estimation="point_to_plane", target_normals=m)
        with pytest.raises(ValueError, match=f"target_normals contains {word} values"):
            icp.registration_icp(p, p, 0.1, np.eye(4), estimation="point_to_plane", target_normals=torch.tensor(m))
    with pytest.raises(ValueError):
        icp.registration_icp(p, p, 0.0, np.eye(4), estimation="point_to_plane", target_normals=n)
    for knn in (2, 33, 0):
        with pytest.raises(ValueError, match="knn"):
            icp.estimate_normals(p, knn=knn)
    q = np.array(p)
    q[0, 0] = np.nan
    with pytest.raises(ValueError, match="points contains NaN values"):
        icp.estimate_normals(q)
    with pytest.raises(ValueError):
        icp.estimate_normals(p[:, :2])
    with pytest.raises(TypeError):      # positional: the reference's four arguments only
        icp.get_ICP_fitting_transformation_best(p, p, np.eye(3)[None], 0.1, "point_to_plane")


def _quat_of(axis, angle):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * axis])


def _rodrigues(axis, angle):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def test_model_normals_for_both_kinds():
    from scorp_amd import icp
    from scorp_amd.gaussian_model import GaussianModel
    from scorp_amd.renderer2d import GaussianModel2D
    cases = [((0, 0, 1), 0.0), ((1, 0, 0), np.pi / 2), ((1, 2, -1), 0.7), ((0, 1, 0), -1.1)]
    quats = np.stack([3.0 * _quat_of(ax, an) for ax, an in cases])          # (not normalised: build_rotation does that)
    R = np.stack([_rodrigues(ax, an) for ax, an in cases])
    m2 = GaussianModel2D(0, device="cpu")
    m2._rotation = torch.tensor(quats, dtype=torch.float32)
    m2._scaling = torch.zeros(4, 2)
    n2 = icp.model_normals(m2)
    assert n2.shape == (4, 3) and not n2.requires_grad
    np.testing.assert_allclose(n2.numpy(), R[:, :, 2], atol=1e-6)
    np.testing.assert_allclose(n2[1].numpy(), [0, -1, 0], atol=1e-6)     # 90 degrees about x takes z to -y
    m3 = GaussianModel(0, device="cpu")
    m3._rotation = torch.tensor(quats, dtype=torch.float32)
    m3._scaling = torch.log(torch.tensor([[0.1, 0.2, 0.3], [0.3, 0.05, 0.2], [0.2, 0.3, 0.01], [0.02, 0.3, 0.1]]))
    n3 = icp.model_normals(m3)
    want = np.stack([R[0][:, 0], R[1][:, 1], R[2][:, 2], R[3][:, 0]])
    np.testing.assert_allclose(n3.numpy(), want, atol=1e-6)
    with pytest.raises(TypeError):
        icp.model_normals(object())
