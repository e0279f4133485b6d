"""Multi-start point-to-plane ICP on the GPU (scorp_icp_point_to_plane, scorp_amd/icp.py) against the float64 yardstick
tests/icp_plane_reference.py, on the fixtures of tests/icp_plane_fixtures.py (whose properties tests/test_icp_plane_cpu.py
shows with the yardstick alone and which are asserted again here).

One update: transformation = reference_update(reference pairs) @ T0 to the larger of 10x the yardstick's own sensitivity
to the order of its pairs (measured by shuffling them) and the floor 1e-13 (1 + extent), the rule of
tests/test_icp_search_gpu.py.  Runs of 0, 1 and 5 updates: the tolerances of
test_icp_gpu.test_margin_fixture_matches_yardstick.  The measured values are printed; DESIGN.md 4.10 holds them.

Measured in one MI355X run: one update at the block edges, |transformation - yardstick| 3.6e-17 - 3.1e-16 over the ten
sizes and two inits (largest at 65 536 points) against the bound 1.9e-13, the floor in every case (the yardstick's own
order sensitivity 0 - 3.1e-16); runs of 0 / 1 / 5 updates 0 / 8.3e-17 / 4.2e-17; rank-deficient systems 5.2e-18
(planar), 1.1e-16 (one source point), 1.2e-16 (one pair), 2.0e-14 against 1.0e-13 (64 identical points); the planted
pose in 4 updates from both inits against 7 and 6 point-to-point."""
import numpy as np
import pytest
import torch

from tests import icp_plane_fixtures as pfx
from tests import icp_plane_reference as pref
from tests import icp_probe_fixtures as fx
from tests import icp_reference as ref
from tests.test_icp_gpu import ROT64, _realistic

pytestmark = pytest.mark.gpu

FIELDS = ("transformation", "fitness", "inlier_rmse", "iterations")


@pytest.fixture(scope="module")
def icp():
    from scorp_amd import icp as m
    return m


def _plane(icp, src, tgt, nrm, r, inits, **kw):
    return icp.registration_icp(np.array(src), np.array(tgt), r, inits, estimation="point_to_plane",
                                target_normals=np.array(nrm), **kw)


def _one_update_bound(xs, qs, ns, ct, s, T0, extent, rng):
    """(the yardstick's transformation after one update, the bound on |GPU - yardstick|, the yardstick's own sensitivity to
    the order of its pairs)."""
    want = pref.reference_update(xs, qs, ns, ct, s) @ T0
    perm = rng.permutation(len(xs))
    own = float(np.abs(pref.reference_update(xs[perm], qs[perm], ns[perm], ct, s) @ T0 - want).max())
    return want, max(10.0 * own, 1e-13 * (1.0 + extent)), own


@pytest.mark.parametrize("ns", fx.AGGREGATE_NS)
def test_one_update_at_block_edges(icp, ns):
    src, tgt, r, inits, pairs = fx.aggregate_fixture(ns)
    nrm = pfx.aggregate_normals()
    assert pfx.poses_have_margin(src, tgt, list(inits), r, relative=False)        # the fixture property, again
    t64, s64, n64 = tgt.astype(np.float64), src.astype(np.float64), nrm.astype(np.float64)
    ct, s = pref.frame(tgt)
    extent = float(np.ptp(t64, axis=0).max())
    res0 = _plane(icp, src, tgt, nrm, r, inits, max_iteration=0)
    res1 = _plane(icp, src, tgt, nrm, r, inits, max_iteration=1, relative_fitness=0.0, relative_rmse=0.0)
    rng = np.random.default_rng(0)
    for j, (T0, (hit, idx)) in enumerate(zip(inits, pairs)):
        x = s64 @ T0[:3, :3].T + T0[:3, 3]
        xs, qs, ns_ = x[hit], t64[idx[hit]], n64[idx[hit]]
        c = len(xs)
        assert c > 0 and res0.iterations[j] == 0 and res1.iterations[j] == 1
        assert int(round(res0.fitness[j] * ns)) == c
        assert res0.fitness[j] == pytest.approx(c / ns, abs=1e-15)
        rmse = float(np.sqrt(((xs - qs) ** 2).sum() / c))
        assert res0.inlier_rmse[j] == pytest.approx(rmse, rel=1e-9)
        assert np.array_equal(res0.transformation[j], T0)
        _, lam = pref.reference_update(xs, qs, ns_, ct, s, return_eig=True)
        assert pref.eig_ratios_clear([lam])
        want, bound, own = _one_update_bound(xs, qs, ns_, ct, s, T0, extent, rng)
        d = float(np.abs(res1.transformation[j] - want).max())
        print(f"ns {ns} init {j}: {c} pairs, transformation to the yardstick {d:.3g} (bound {bound:.3g}, the yardstick's own "
              f"order sensitivity {own:.3g})")
        assert d <= bound


@pytest.mark.parametrize("max_iteration", [0, 1, 5])
def test_margin_fixture_matches_yardstick(icp, max_iteration):
    src, tgt, nrm, r, inits, runs = pfx.margin_fixture()
    assert pfx.poses_have_margin(src, tgt, [T for y in runs for T in y["poses"]], r)
    assert all(pref.eig_ratios_clear(y["eigenvalues"]) for y in runs)
    res = _plane(icp, src, tgt, nrm, r, inits, max_iteration=max_iteration, relative_fitness=0.0, relative_rmse=0.0)
    extent = float(np.ptp(tgt, axis=0).max())
    for j, T0 in enumerate(inits):
        y = pref.registration_icp(src, tgt, nrm, r, T0, max_iteration=max_iteration, relative_fitness=0.0, relative_rmse=0.0)
        assert res.iterations[j] == y["iterations"] == max_iteration
        assert int(round(res.fitness[j] * len(src))) == y["passes"][-1]
        assert res.fitness[j] == pytest.approx(y["fitness"], abs=1e-12)
        assert res.inlier_rmse[j] == pytest.approx(y["inlier_rmse"], rel=1e-6)
        np.testing.assert_allclose(res.transformation[j, :3, :3], y["transformation"][:3, :3], atol=1e-6)
        np.testing.assert_allclose(res.transformation[j, :3, 3], y["transformation"][:3, 3], atol=1e-6 * extent)
        print(f"max_iteration {max_iteration} init {j}: |T - yardstick| {np.abs(res.transformation[j] - y['transformation']).max():.3g}")


@pytest.mark.parametrize("name", sorted(pfx.RANK_DEFICIENT))
def test_rank_deficient_systems_take_the_minimum_norm_step(icp, name):
    src, tgt, nrm, r, y = pfx.rank_deficient(name)
    if name != "identical64":
        assert pfx.poses_have_margin(src, tgt, y["poses"], r)
    assert pref.eig_ratios_clear(y["eigenvalues"])
    res = _plane(icp, src, tgt, nrm, r, np.eye(4), max_iteration=1, relative_fitness=0.0, relative_rmse=0.0)
    T = res.transformation[0]
    assert np.isfinite(T).all() and res.iterations[0] == 1
    assert np.linalg.det(T[:3, :3]) == pytest.approx(1.0, abs=1e-9)
    assert int(round(res.fitness[0] * len(src))) == y["passes"][-1]
    # the yardstick's pairs of the first pass, from its own search
    t64, s64, n64 = tgt.astype(np.float64), src.astype(np.float64), nrm.astype(np.float64)
    i1, d1, _, _ = fx.brute_nearest(tgt, src)
    hit = d1 <= r
    assert hit.sum() == y["passes"][0]
    ct, s = pref.frame(tgt)
    want, bound, own = _one_update_bound(s64[hit], t64[i1[hit]], n64[i1[hit]], ct, s, np.eye(4),
                                         float(np.ptp(t64, axis=0).max()), np.random.default_rng(0))
    np.testing.assert_allclose(want, y["poses"][1], atol=1e-14)
    d = float(np.abs(T - want).max())
    print(f"{name}: {int(hit.sum())} pairs, transformation to the yardstick {d:.3g} (bound {bound:.3g}, own {own:.3g})")
    assert d <= bound
    if name == "planar":
        assert np.abs(T[:2, 3]).max() <= 1e-12 and np.abs(T[:3, :3] - np.eye(3)).max() <= 1e-12
        assert T[2, 3] == pytest.approx(-float(src[0, 2]), abs=1e-9)


def test_no_pairs_and_zero_normals_keep_the_init(icp):
    src, tgt, nrm, r, inits, _ = pfx.margin_fixture()
    T0 = np.array(inits[2])
    T0[:3, 3] += (5.0, 0.0, 0.0)
    res = _plane(icp, src, tgt, nrm, 1e-3, T0, max_iteration=30)
    assert res.fitness[0] == 0.0 and res.inlier_rmse[0] == 0.0
    assert np.array_equal(res.transformation[0], T0)
    res = _plane(icp, src, tgt, np.zeros_like(nrm), r, inits, max_iteration=7)
    assert np.array_equal(res.transformation, inits) and (res.fitness > 0.5).all() and (res.inlier_rmse > 0).all()


def test_deterministic_and_batch_independent(icp):
    src, tgt, nrm, r, R0, t0, _, _ = pfx.planted()
    rots = np.load(ROT64)["rotations"][:4]
    inits = ref.icp_inits(rots, tgt.mean(axis=0), src.mean(axis=0))
    a = _plane(icp, src, tgt, nrm, r, inits, max_iteration=40)
    b = _plane(icp, src, tgt, nrm, r, inits, max_iteration=40)
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert len(set(a.iterations.tolist())) > 1           # inits that stop at different passes
    for j in (0, 2, len(inits) - 1):
        s = _plane(icp, src, tgt, nrm, r, inits[j], max_iteration=40)
        for f in FIELDS:
            assert np.array_equal(getattr(s, f)[0], getattr(a, f)[j]), (f, j)


def test_inputs_unmodified(icp):
    src, tgt, nrm, r, inits, _ = pfx.margin_fixture()
    dev = torch.device("cuda:0")
    S, Q, N = (torch.tensor(np.array(a), device=dev) for a in (src, tgt, nrm))
    S0, Q0, N0, I0 = S.clone(), Q.clone(), N.clone(), inits.copy()
    icp.registration_icp(S, Q, r, inits, max_iteration=10, estimation="point_to_plane", target_normals=N)
    assert torch.equal(S, S0) and torch.equal(Q, Q0) and torch.equal(N, N0) and np.array_equal(inits, I0)


def test_planted_pose_in_fewer_updates_than_point_to_point(icp):
    src, tgt, nrm, r, R0, t0, yp, y2 = pfx.planted()
    assert yp["iterations"] < y2["iterations"]                      # the fixture property, by the yardsticks
    inits = np.stack([np.eye(4)] * 2)
    inits[1, :3, 3] = (0.004, -0.003, 0.002)
    n = pfx.PLANTED_MAX_ITERATION
    plane = _plane(icp, src, tgt, nrm, r, inits, max_iteration=n)
    point = icp.registration_icp(np.array(src), np.array(tgt), r, inits, max_iteration=n)
    print(f"planted pose: updates point-to-plane {plane.iterations.tolist()} (yardstick {yp['iterations']}), point-to-point "
          f"{point.iterations.tolist()} (yardstick {y2['iterations']})")
    for j in range(len(inits)):
        T = plane.transformation[j]
        assert np.abs(T[:3, :3] - R0).max() < 0.02 and np.abs(T[:3, 3] - t0).max() < 0.02
        if plane.iterations[j] < n and point.iterations[j] < n:
            assert plane.iterations[j] < point.iterations[j]
    assert plane.iterations[0] < n and point.iterations[0] < n


def test_far_from_origin(icp):
    src, tgt, nrm, r, R0, t0, _, _ = pfx.planted()
    off = np.array([1000.0, -1000.0, 1000.0])
    src_f = (src.astype(np.float64) + off).astype(np.float32)
    tgt_f = (tgt.astype(np.float64) + off).astype(np.float32)
    T0 = np.eye(4)
    T0[:3, 3] = (0.004, -0.003, 0.002)
    res = _plane(icp, src_f, tgt_f, nrm, r, T0, max_iteration=100)
    y = pref.registration_icp(src_f, tgt_f, nrm, r, T0, max_iteration=100)
    # the bounds test_icp_gpu.test_far_from_origin holds the point-to-point path to
    assert abs(res.fitness[0] - y["fitness"]) <= 2e-4
    np.testing.assert_allclose(res.transformation[0, :3, :3], y["transformation"][:3, :3], atol=1e-4)
    np.testing.assert_allclose(res.transformation[0, :3, 3], y["transformation"][:3, 3], atol=1e-3)
    assert res.fitness[0] > 0.8
    # and it is the unshifted result, shifted: it takes the shifted source where the unshifted result takes the source
    # (the translation column alone would multiply a rotation difference by |off|)
    near = _plane(icp, src, tgt, nrm, r, T0, max_iteration=100).transformation[0]
    np.testing.assert_allclose(res.transformation[0, :3, :3], near[:3, :3], atol=1e-4)
    p = src.astype(np.float64)
    moved = (p + off) @ res.transformation[0, :3, :3].T + res.transformation[0, :3, 3]
    np.testing.assert_allclose(moved, p @ near[:3, :3].T + near[:3, 3] + off, atol=1e-3)


def test_best_transformation_default_is_unchanged_and_plane_finds_the_pose(icp):
    src, tgt, R0, t0 = _realistic()
    rots = np.load(ROT64)["rotations"][:13]
    r = float(np.ptp(tgt, axis=0).mean() / 10 * 1.6)
    # today's output: the point-to-point batch at max_iteration = 400, the first init of the highest fitness
    inits = icp.icp_inits(rots, tgt.mean(axis=0), src.mean(axis=0))
    res = icp.registration_icp(src[icp.downsample_indices(len(tgt), len(src))], tgt, r, inits, max_iteration=400)
    today = res.transformation[int(np.argmax(res.fitness))]
    assert np.array_equal(icp.get_ICP_fitting_transformation_best(tgt, src, rots, r), today)
    assert np.array_equal(icp.get_ICP_fitting_transformation_best(tgt, src, rots, r, estimation="point_to_point"), today)
    best = icp.get_ICP_fitting_transformation_best(tgt, src, rots, r, estimation="point_to_plane")
    assert best.shape == (4, 4) and best.dtype == np.float64
    print(f"_realistic(): point-to-plane |R - R0| {np.abs(best[:3, :3] - R0).max():.3g}, |t - t0| {np.abs(best[:3, 3] - t0).max():.3g}")
    assert np.abs(best[:3, :3] - R0).max() < 0.02
    assert np.abs(best[:3, 3] - t0).max() < 0.02
