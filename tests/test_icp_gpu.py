"""Multi-start point-to-point ICP on the GPU (scorp_icp_point_to_point, scorp_amd/icp.py) against the float64 yardstick
tests/icp_reference.py (Open3D registration_icp's semantics over scipy's cKDTree)."""
import os

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

from tests import icp_reference as ref

pytestmark = pytest.mark.gpu

ROT64 = os.path.join(os.path.dirname(__file__), "golden", "rotations_64.npz")


@pytest.fixture(scope="module")
def icp():
    from scorp_amd import icp as m
    return m


def _margin_ok(src, tgt, T_list, r):
    """No source point's d^2 within 1e-4 r^2 of r^2 and no second-nearest within 1e-3 (relative) of the nearest, at
    every pose of T_list."""
    tree = cKDTree(tgt)
    for T in T_list:
        x = src @ T[:3, :3].T + T[:3, 3]
        d, _ = tree.query(x, k=2)
        d1, d2 = d[:, 0], d[:, 1]
        if np.any(np.abs(d1 ** 2 - r * r) <= 1e-4 * r * r):
            return False
        near = d1 <= r
        if np.any((d2[near] - d1[near]) <= 1e-3 * d1[near]):
            return False
    return True


def _margin_fixture():
    """A jittered lattice (spacing 0.1) as the target and a slightly moved, noisy copy of part of it as the source: every
    source point has one clear nearest neighbour, well inside r, at every pass of a 5-iteration run from each of three
    inits.  The first seed with the margin property at all those poses."""
    g = np.stack(np.meshgrid(*[np.arange(8) * 0.1] * 3, indexing="ij"), -1).reshape(-1, 3)
    for seed in range(50):
        rng = np.random.default_rng(seed)
        tgt = (g + rng.uniform(-0.012, 0.012, g.shape)).astype(np.float32)
        a = np.deg2rad(3.0)
        R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        sub = tgt[rng.choice(len(tgt), 300, replace=False)].astype(np.float64)
        src = ((sub - 0.35) @ R + 0.35 + (0.01, -0.01, 0.005) + rng.normal(scale=0.002, size=sub.shape)).astype(np.float32)
        r = 0.045
        inits = np.stack([np.eye(4)] * 3)
        inits[1, :3, 3] = (-0.008, 0.006, -0.004)
        b = np.deg2rad(-2.0)
        inits[2, :3, :3] = [[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]]
        tree = cKDTree(tgt.astype(np.float64))
        poses = []
        for T0 in inits:
            T = T0.copy()
            poses.append(T.copy())
            for _ in range(5):
                _, _, xs, qs, _ = ref.correspondence_pass(tree, tgt.astype(np.float64), src.astype(np.float64), T, r)
                T = ref.kabsch_update(xs, qs) @ T
                poses.append(T.copy())
        if _margin_ok(src.astype(np.float64), tgt.astype(np.float64), poses, r):
            return src, tgt, r, inits, poses
    pytest.fail("no seed gave the margin property")


@pytest.mark.parametrize("max_iteration", [0, 1, 5])
def test_margin_fixture_matches_yardstick(icp, max_iteration):
    src, tgt, r, inits, poses = _margin_fixture()
    assert _margin_ok(src.astype(np.float64), tgt.astype(np.float64), poses, r)   # the fixture property, at every pose
    res = icp.registration_icp(src, tgt, r, inits, max_iteration=max_iteration, relative_fitness=0.0, relative_rmse=0.0)
    extent = float(np.ptp(tgt, axis=0).max())
    for j, T0 in enumerate(inits):
        y = ref.registration_icp(src, tgt, r, T0, max_iteration=max_iteration, relative_fitness=0.0, relative_rmse=0.0)
        assert res.iterations[j] == y["iterations"] == max_iteration
        assert int(round(res.fitness[j] * len(src))) == y["passes"][-1]          # pair count of the last pass, exactly
        assert res.fitness[j] == pytest.approx(y["fitness"], abs=1e-12)
        assert res.inlier_rmse[j] == pytest.approx(y["inlier_rmse"], rel=1e-6)
        np.testing.assert_allclose(res.transformation[j, :3, :3], y["transformation"][:3, :3], atol=1e-6)
        np.testing.assert_allclose(res.transformation[j, :3, 3], y["transformation"][:3, 3], atol=1e-6 * extent)


def _realistic(seed=3):
    rng = np.random.default_rng(seed)
    tgt = ref.asymmetric_object(6000, seed).astype(np.float32)
    obj = ref.asymmetric_object(9000, seed + 100)
    obj = obj[obj[:, 0] < 0.35]                                   # partly cropped
    # the planted rotation: 12 degrees away from one of the inits' rotations (an ICP basin is not the whole of SO(3))
    a = np.deg2rad(12.0)
    tilt = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    R0 = tilt @ np.load(ROT64)["rotations"][4]
    t0 = np.array([0.3, -0.2, 0.1])
    # the generated copy: in its own frame, q = R0 p + t0 maps it back onto the original
    src = ((obj - t0) @ R0 + rng.normal(scale=0.003, size=obj.shape)).astype(np.float32)
    return src, tgt, R0, t0


def test_realistic_fixture_matches_yardstick(icp):
    src, tgt, R0, t0 = _realistic()
    rots = np.load(ROT64)["rotations"][:13]                       # 13 + 3 = 16 inits
    bbox = np.ptp(tgt, axis=0)
    r = float(bbox.mean() / 10 * 1.6)                             # the alignment script's threshold
    best_ref, results = ref.get_ICP_fitting_transformation_best(tgt, src, rots, r, workers=16, return_all=True)
    inits = ref.icp_inits(rots, tgt.mean(axis=0), src.mean(axis=0))
    res = icp.registration_icp(src, tgt, r, inits, max_iteration=400)
    fit_ref = np.array([y["fitness"] for y in results])
    np.testing.assert_allclose(res.fitness, fit_ref, atol=2e-4)
    for j, y in enumerate(results):
        if y["iterations"] < 400:
            np.testing.assert_allclose(res.transformation[j], y["transformation"], atol=1e-3)
    best = icp.get_ICP_fitting_transformation_best(tgt, src, rots, r)
    top = fit_ref.max()
    tied = [results[j]["transformation"] for j in range(len(results)) if fit_ref[j] >= top - 2e-4]
    assert any(np.allclose(best, T, atol=1e-3) for T in tied)
    np.testing.assert_allclose(best, best_ref, atol=1e-3)
    # the planted pose
    assert np.abs(best[:3, :3] - R0).max() < 0.02
    assert np.abs(best[:3, 3] - t0).max() < 0.02


def test_deterministic_and_batch_independent(icp):
    src, tgt, _, _ = _realistic(5)
    rots = np.load(ROT64)["rotations"][:5]
    inits = ref.icp_inits(rots, tgt.mean(axis=0), src.mean(axis=0))
    r = float(np.ptp(tgt, axis=0).mean() * 0.16)
    a = icp.registration_icp(src, tgt, r, inits, max_iteration=60)
    b = icp.registration_icp(src, tgt, r, inits, max_iteration=60)
    for f in ("transformation", "fitness", "inlier_rmse", "iterations"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    for j in (0, 3, len(inits) - 1):
        s = icp.registration_icp(src, tgt, r, inits[j], max_iteration=60)
        assert np.array_equal(s.transformation[0], a.transformation[j])
        assert s.fitness[0] == a.fitness[j] and s.inlier_rmse[0] == a.inlier_rmse[j]
        assert s.iterations[0] == a.iterations[j]


def test_no_pairs_keeps_the_init(icp):
    src, tgt, _, _ = _realistic(7)
    T0 = np.eye(4)
    T0[:3, 3] = (5.0, 0.0, 0.0)
    res = icp.registration_icp(src, tgt, 1e-3, T0, max_iteration=30)
    assert res.fitness[0] == 0.0 and res.inlier_rmse[0] == 0.0
    assert np.array_equal(res.transformation[0], T0)


def test_single_points_and_single_init(icp):
    tgt = np.array([[0.1, 0.2, 0.3]], np.float32)
    src = np.array([[0.0, 0.0, 0.0]], np.float32)
    res = icp.registration_icp(src, tgt, 1.0, np.eye(4), max_iteration=10)
    y = ref.registration_icp(src, tgt, 1.0, np.eye(4), max_iteration=10)
    assert res.fitness[0] == 1.0 and y["fitness"] == 1.0
    np.testing.assert_allclose(res.transformation[0], y["transformation"], atol=1e-6)
    np.testing.assert_allclose(res.transformation[0][:3, 3], tgt[0], atol=1e-6)
    many = ref.asymmetric_object(500, 1).astype(np.float32)
    res = icp.registration_icp(many, tgt, 2.0, np.eye(4), max_iteration=10)
    assert res.fitness[0] == 1.0
    np.testing.assert_allclose(np.linalg.det(res.transformation[0, :3, :3]), 1.0, atol=1e-9)
    res = icp.registration_icp(src, many, 2.0, np.eye(4), max_iteration=10)
    y = ref.registration_icp(src, many, 2.0, np.eye(4), max_iteration=10)
    np.testing.assert_allclose(res.transformation[0], y["transformation"], atol=1e-6)


def test_far_from_origin(icp):
    src, tgt, R0, t0 = _realistic(11)
    off = np.array([1000.0, -1000.0, 1000.0])
    src_f = (src.astype(np.float64) + off).astype(np.float32)
    tgt_f = (tgt.astype(np.float64) + off).astype(np.float32)
    T0 = np.eye(4)
    T0[:3, :3] = R0
    T0[:3, 3] = off + t0 - R0 @ off + 0.01
    r = float(np.ptp(tgt, axis=0).mean() * 0.16)
    res = icp.registration_icp(src_f, tgt_f, r, T0, max_iteration=100)
    y = ref.registration_icp(src_f, tgt_f, r, T0, max_iteration=100)
    assert abs(res.fitness[0] - y["fitness"]) <= 2e-4
    np.testing.assert_allclose(res.transformation[0, :3, :3], y["transformation"][:3, :3], atol=1e-4)
    np.testing.assert_allclose(res.transformation[0, :3, 3], y["transformation"][:3, 3], atol=1e-3)
    assert res.fitness[0] > 0.8


def test_rank_deficient_pairs_give_a_rotation(icp):
    line = np.zeros((64, 3), np.float32)
    line[:, 0] = np.linspace(0, 1, 64)
    src = line + np.float32([0.0, 0.01, 0.0])
    res = icp.registration_icp(src, line, 0.1, np.eye(4), max_iteration=5)
    R = res.transformation[0, :3, :3]
    np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-9)
    assert np.linalg.det(R) == pytest.approx(1.0, abs=1e-9)
    one = np.zeros((1, 3), np.float32)
    res = icp.registration_icp(np.repeat(one, 5, 0), np.repeat(one, 3, 0), 0.5, np.eye(4), max_iteration=3)
    assert np.linalg.det(res.transformation[0, :3, :3]) == pytest.approx(1.0, abs=1e-9)


def test_inputs_unmodified(icp):
    src, tgt, _, _ = _realistic(13)
    dev = torch.device("cuda:0")
    S, Q = torch.tensor(src, device=dev), torch.tensor(tgt, device=dev)
    S0, Q0 = S.clone(), Q.clone()
    inits = np.stack([np.eye(4)] * 2)
    I0 = inits.copy()
    icp.registration_icp(S, Q, 0.1, inits, max_iteration=20)
    assert torch.equal(S, S0) and torch.equal(Q, Q0) and np.array_equal(inits, I0)


def test_argument_errors(icp):
    p = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError):
        icp.registration_icp(p, p, 0.0, np.eye(4))
    with pytest.raises(ValueError):
        icp.registration_icp(p, p, -1.0, np.eye(4))
    with pytest.raises(ValueError):
        icp.registration_icp(p[:0], p, 0.1, np.eye(4))
    with pytest.raises(ValueError):
        icp.registration_icp(p, p[:0], 0.1, np.eye(4))
    with pytest.raises(ValueError):
        icp.registration_icp(p, p, 0.1, np.eye(4), max_iteration=-1)
