"""The ICP yardstick (tests/icp_reference.py) and the host side of scorp_amd/icp.py, without a GPU."""
import ctypes
import os

import numpy as np
import pytest

from tests import icp_reference as ref

ROT64 = os.path.join(os.path.dirname(__file__), "golden", "rotations_64.npz")


def test_yardstick_recovers_a_planted_transform():
    q = ref.asymmetric_object(3000, 0)
    a = np.deg2rad(8.0)
    R0 = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    t0 = np.array([0.05, -0.02, 0.03])
    p = (q - t0) @ R0            # q = R0 p + t0, noise-free
    res = ref.registration_icp(p, q, 0.2, np.eye(4), max_iteration=200)
    assert res["fitness"] == 1.0
    np.testing.assert_allclose(res["transformation"][:3, :3], R0, atol=1e-6)
    np.testing.assert_allclose(res["transformation"][:3, 3], t0, atol=1e-6)
    assert res["inlier_rmse"] < 1e-6


def test_update_is_a_direct_kabsch():
    rng = np.random.default_rng(1)
    x = rng.normal(size=(50, 3))
    R = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    R *= np.sign(np.linalg.det(R))
    q = x @ R.T + (1.0, 2.0, 3.0) + rng.normal(scale=0.01, size=x.shape)
    U = ref.kabsch_update(x, q)
    # direct: H = sum (x - xm)(q - qm)^T = V S W^T, R = W diag(1, 1, det(W V^T)) V^T
    xm, qm = x.mean(0), q.mean(0)
    V, _, Wt = np.linalg.svd((x - xm).T @ (q - qm))
    d = np.sign(np.linalg.det(Wt.T @ V.T))
    Rd = Wt.T @ np.diag([1, 1, d]) @ V.T
    np.testing.assert_allclose(U[:3, :3], Rd, atol=1e-12)
    np.testing.assert_allclose(U[:3, 3], qm - Rd @ xm, atol=1e-12)
    assert np.linalg.det(U[:3, :3]) == pytest.approx(1.0)
    assert np.array_equal(ref.kabsch_update(x[:0], q[:0]), np.eye(4))


def test_init_list_order_duplicate_identity():
    from scorp_amd import icp
    rots = np.load(ROT64)["rotations"]
    assert rots.shape == (64, 3, 3)
    co, cr = np.array([1.0, 2.0, 3.0]), np.array([-0.5, 0.25, 0.0])
    T = icp.icp_inits(rots, co, cr)
    assert T.shape == (67, 4, 4) and T.dtype == np.float64
    for i, R in enumerate(rots):
        np.testing.assert_array_equal(T[i, :3, :3], R)
        np.testing.assert_array_equal(T[i, :3, 3], co - R @ cr)
    np.testing.assert_array_equal(T[64], T[65])
    np.testing.assert_array_equal(T[64, :3, 3], co - cr)
    np.testing.assert_array_equal(T[64, :3, :3], np.eye(3))
    np.testing.assert_array_equal(T[66], np.eye(4))
    np.testing.assert_array_equal(T[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (67, 1)))
    np.testing.assert_array_equal(T, ref.icp_inits(rots, co, cr))


def test_downsampling_rule():
    from scorp_amd import icp
    assert np.array_equal(icp.downsample_indices(100, 400), np.arange(400))          # not more than 4x: all
    assert np.array_equal(icp.downsample_indices(100, 401), np.arange(401))          # k = int(401 / 400) = 1
    assert np.array_equal(icp.downsample_indices(100, 850), np.arange(0, 850, 2))    # k = 2: 0, 2, 4, ...
    assert np.array_equal(icp.downsample_indices(1000, 8000), np.arange(0, 8000, 2))
    assert np.array_equal(icp.downsample_indices(10, 1000), np.arange(0, 1000, 25))
    for a, b in ((100, 850), (7, 1000), (3, 3)):
        assert np.array_equal(icp.downsample_indices(a, b), ref.downsample_indices(a, b))


def test_first_max_tie_rule(monkeypatch):
    """The first init with the highest fitness wins (the reference's strict >), whatever comes after it."""
    from scorp_amd import icp
    rots = np.load(ROT64)["rotations"][:4]
    n = len(rots) + 3
    fit = np.array([0.5, 0.9, 0.7, 0.9, 0.9, 0.1, 0.9])
    T = np.stack([np.eye(4) * (j + 1) for j in range(n)])

    def fake(source, target, r, inits, max_iteration=30, **kw):
        assert max_iteration == 400 and len(inits) == n
        return icp.ICPResult(T.copy(), fit.copy(), np.zeros(n), np.zeros(n, np.int32))

    monkeypatch.setattr(icp, "registration_icp", fake)
    p = np.random.default_rng(0).random((20, 3))
    best = icp.get_ICP_fitting_transformation_best(p, p, rots, 0.1)
    assert np.array_equal(best, T[1])
    assert best.dtype == np.float64 and best.shape == (4, 4)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_front_end_rejects_non_finite_before_the_device(monkeypatch, bad):
    from scorp_amd import icp, _C

    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_C, "lib", no_device)
    p = np.random.default_rng(0).random((20, 3))
    q = p.copy()
    q[3, 1] = bad
    rots = np.load(ROT64)["rotations"][:2]
    with pytest.raises(ValueError):
        icp.get_ICP_fitting_transformation_best(q, p, rots, 0.1)
    with pytest.raises(ValueError):
        icp.get_ICP_fitting_transformation_best(p, q, rots, 0.1)
    with pytest.raises(ValueError):
        icp.registration_icp(q, p, 0.1, np.eye(4))
    with pytest.raises(ValueError):
        icp.registration_icp(p, p, 0.0, np.eye(4))
    with pytest.raises(ValueError):
        icp.registration_icp(p, p, 0.1, np.eye(4), max_iteration=-1)


def test_workspace_bytes_is_exported_and_answers():
    from scorp_amd import build, _C
    build.build()
    lib = ctypes.CDLL(build.LIB)
    assert hasattr(lib, "scorp_icp_workspace_bytes") and hasattr(lib, "scorp_icp_point_to_point")
    L = _C.lib()
    assert L.scorp_version() >= 102
    small = L.scorp_icp_workspace_bytes(1, 1, 1)
    big = L.scorp_icp_workspace_bytes(200_000, 100_000, 67)
    assert 0 < small < big
    assert big >= 200_000 * 16 + 100_000 * 16        # the sorted clouds at least
    assert big == L.scorp_icp_workspace_bytes(200_000, 100_000, 67)
