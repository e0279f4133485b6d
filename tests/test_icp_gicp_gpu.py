"""Multi-start generalized ICP on the GPU (scorp_icp_generalized, scorp_amd/icp.py) against the float64 yardstick
tests/icp_gicp_reference.py, on the fixtures of tests/icp_gicp_fixtures.py (whose properties tests/test_icp_gicp_cpu.py
shows with the yardstick alone and which are asserted again here).  It mirrors tests/test_icp_plane_gpu.py.

One update: transformation = reference_update(reference pairs) @ T0 to the largest of 10x the yardstick's own sensitivity
to the order of its pairs (measured by shuffling them), 10x its sensitivity to the inverse (cofactors against
np.linalg.inv) and the floor 1e-13 (1 + extent): icp_gicp_fixtures.one_update_bound, every term measured on the yardstick,
never on the code under test.  Runs of 0, 1 and 5 updates: the tolerances of
test_icp_gpu.test_margin_fixture_matches_yardstick.  The measured values are printed; DESIGN.md 4.10 holds them.

Measured in one MI355X run: one update at the block edges, |transformation - yardstick| 1.6e-17 - 6.0e-16 over the ten
sizes and two inits (largest at 66 561 points) against the bound 1.9e-13, the floor in every case (the yardstick's own
order sensitivity 0 - 1.1e-15, cofactor against numpy inverse 6.9e-18 - 1.4e-16); runs of 0 / 1 / 5 updates from the
three 40 degree inits 0 / 1.1e-16 / 1.1e-16; a quarter of the covariances zero 1.1e-16; one source point 3.1e-17, one pair
7.4e-17, 64 identical points 6.7e-13 against 3.0e-11 (10x the yardstick's own 3.0e-12); the planted pose in 4 updates from
both starts, the yardstick's count, against the yardsticks' 4 point-to-plane and 7 point-to-point."""
import numpy as np
import pytest
import torch

from tests import icp_gicp_fixtures as gfx
from tests import icp_gicp_reference as gref
from tests import icp_plane_fixtures as pfx
from tests import icp_plane_reference as pref
from tests import icp_probe_fixtures as fx
from tests import icp_reference as ref
from tests.test_icp_gpu import ROT64

pytestmark = pytest.mark.gpu

FIELDS = ("transformation", "fitness", "inlier_rmse", "iterations")


@pytest.fixture(scope="module")
def icp():
    from scorp_amd import icp as m
    return m


def _gicp(icp, src, Cp, tgt, Cq, r, inits, **kw):
    return icp.registration_icp(np.array(src), np.array(tgt), r, np.array(inits), estimation="generalized",
                                source_covariances=np.array(Cp), target_covariances=np.array(Cq), **kw)


def _check_one_update(what, T, src, Cp, tgt, Cq, r, T0, rng):
    """|T - yardstick| of one update from T0 under icp_gicp_fixtures.one_update_bound; returns the yardstick's transformation."""
    xs, qs, Cs, Ct = gfx.first_pass(src, Cp, tgt, Cq, r, T0)
    ct, s = pref.frame(tgt)
    extent = float(np.ptp(tgt.astype(np.float64), axis=0).max())
    _, lam = gref.reference_update(xs, qs, Cs, Ct, ct, s, return_eig=True)
    assert pref.eig_ratios_clear([lam])
    want, bound, own, inv = gfx.one_update_bound(xs, qs, Cs, Ct, ct, s, T0, extent, rng)
    d = float(np.abs(T - want).max())
    print(f"{what}: {len(xs)} pairs, transformation to the yardstick {d:.3g} (bound {bound:.3g}; the yardstick's own order "
          f"sensitivity {own:.3g}, cofactor against numpy inverse {inv:.3g})")
    assert d <= bound
    return want


@pytest.mark.parametrize("ns", fx.AGGREGATE_NS)
def test_one_update_at_block_edges(icp, ns):
    src, tgt, r, inits, pairs = fx.aggregate_fixture(ns)
    Cp, Cq = gfx.aggregate_source_covariances(ns), gfx.aggregate_target_covariances()
    assert pfx.poses_have_margin(src, tgt, list(inits), r, relative=False)        # the fixture property, again
    t64, s64 = tgt.astype(np.float64), src.astype(np.float64)
    res0 = _gicp(icp, src, Cp, tgt, Cq, r, inits, max_iteration=0)
    res1 = _gicp(icp, src, Cp, tgt, Cq, r, inits, max_iteration=1, relative_fitness=0.0, relative_rmse=0.0)
    rng = np.random.default_rng(0)
    for j, (T0, (hit, idx)) in enumerate(zip(inits, pairs)):
        x = s64 @ T0[:3, :3].T + T0[:3, 3]
        xs, qs = x[hit], t64[idx[hit]]
        c = len(xs)
        assert c > 0 and res0.iterations[j] == 0 and res1.iterations[j] == 1
        assert int(round(res0.fitness[j] * ns)) == c
        assert res0.fitness[j] == pytest.approx(c / ns, abs=1e-15)
        rmse = float(np.sqrt(((xs - qs) ** 2).sum() / c))
        assert res0.inlier_rmse[j] == pytest.approx(rmse, rel=1e-9)
        assert np.array_equal(res0.transformation[j], T0)
        _check_one_update(f"ns {ns} init {j}", res1.transformation[j], src, Cp, tgt, Cq, r, T0, rng)


@pytest.mark.parametrize("max_iteration", [0, 1, 5])
def test_margin_fixture_matches_yardstick(icp, max_iteration):
    src, Cp, tgt, Cq, r, inits, runs = gfx.margin_fixture()
    assert pfx.poses_have_margin(src, tgt, [T for y in runs for T in y["poses"]], r)
    assert all(pref.eig_ratios_clear(y["eigenvalues"]) for y in runs)
    assert all(gfx.rotation_angle_degrees(T[:3, :3]) >= 30.0 for T in inits)
    res = _gicp(icp, src, Cp, tgt, Cq, r, inits, max_iteration=max_iteration, relative_fitness=0.0, relative_rmse=0.0)
    extent = float(np.ptp(tgt, axis=0).max())
    for j, T0 in enumerate(inits):
        y = gref.registration_icp(src, tgt, Cp, Cq, r, T0, max_iteration=max_iteration, relative_fitness=0.0, relative_rmse=0.0)
        assert res.iterations[j] == y["iterations"] == max_iteration
        assert int(round(res.fitness[j] * len(src))) == y["passes"][-1]
        assert res.fitness[j] == pytest.approx(y["fitness"], abs=1e-12)
        assert res.inlier_rmse[j] == pytest.approx(y["inlier_rmse"], rel=1e-6)
        np.testing.assert_allclose(res.transformation[j, :3, :3], y["transformation"][:3, :3], atol=1e-6)
        np.testing.assert_allclose(res.transformation[j, :3, 3], y["transformation"][:3, 3], atol=1e-6 * extent)
        print(f"max_iteration {max_iteration} init {j}: |T - yardstick| {np.abs(res.transformation[j] - y['transformation']).max():.3g}")


def test_no_pairs_and_zero_covariances_keep_the_init(icp):
    src, Cp, tgt, Cq, r, inits, _ = gfx.margin_fixture()
    T0 = np.array(inits[2])
    T0[:3, 3] += (5.0, 0.0, 0.0)
    res = _gicp(icp, src, Cp, tgt, Cq, 1e-3, T0, max_iteration=30)
    assert res.fitness[0] == 0.0 and res.inlier_rmse[0] == 0.0
    assert np.array_equal(res.transformation[0], T0)
    res = _gicp(icp, src, np.zeros_like(Cp), tgt, np.zeros_like(Cq), r, inits, max_iteration=7)
    assert np.array_equal(res.transformation, inits) and (res.fitness > 0.5).all() and (res.inlier_rmse > 0).all()


def test_pairs_with_zero_covariances_count_but_add_nothing(icp):
    src, _, tgt, _, r, inits, _ = gfx.margin_fixture()
    Cp, Cq, hit = gfx.quarter_zero()
    res0 = _gicp(icp, src, Cp, tgt, Cq, r, inits, max_iteration=0)
    res1 = _gicp(icp, src, Cp, tgt, Cq, r, inits, max_iteration=1, relative_fitness=0.0, relative_rmse=0.0)
    rng = np.random.default_rng(0)
    for j, T0 in enumerate(inits):
        xs, si, _ = gfx.first_pairs(src, tgt, T0, r)
        assert len(hit[j]) > 30 and np.isin(hit[j], si).all()
        assert int(round(res0.fitness[j] * len(src))) == len(xs)          # the pairs with M = 0 still count
        _check_one_update(f"a quarter zero, init {j}", res1.transformation[j], src, Cp, tgt, Cq, r, T0, rng)


@pytest.mark.parametrize("name", gfx.RANK_DEFICIENT)
def test_degenerate_systems_take_the_minimum_norm_step(icp, name):
    src, Cp, tgt, Cq, r, y = gfx.rank_deficient(name)
    if name != "identical64":
        assert pfx.poses_have_margin(src, tgt, y["poses"], r)
    assert pref.eig_ratios_clear(y["eigenvalues"])
    res = _gicp(icp, src, Cp, tgt, Cq, r, np.eye(4), max_iteration=1, relative_fitness=0.0, relative_rmse=0.0)
    T = res.transformation[0]
    assert np.isfinite(T).all() and res.iterations[0] == 1
    assert np.linalg.det(T[:3, :3]) == pytest.approx(1.0, abs=1e-9)
    assert int(round(res.fitness[0] * len(src))) == y["passes"][-1]
    want = _check_one_update(name, T, src, Cp, tgt, Cq, r, np.eye(4), np.random.default_rng(0))
    np.testing.assert_allclose(want, y["poses"][1], atol=1e-14)


def test_planted_pose_from_the_identity_and_from_a_rotated_init(icp):
    p = gfx.planted()
    n = pfx.PLANTED_MAX_ITERATION
    for k, (src, Cp, T0, want, y) in enumerate(p["starts"]):
        assert y["iterations"] < n                                     # the yardstick converges from this start
        res = _gicp(icp, src, Cp, p["target"], p["target_covariances"], p["r"], T0, max_iteration=n)
        T = res.transformation[0]
        print(f"planted pose, start {k} ({gfx.rotation_angle_degrees(T0[:3, :3]):.0f} degrees): generalized "
              f"{res.iterations[0]} updates (yardstick {y['iterations']}); the yardsticks' point-to-plane "
              f"{p['plane']['iterations']}, point-to-point {p['point']['iterations']}; |T - planted| {np.abs(T - want)[:3].max():.3g}")
        assert res.iterations[0] == y["iterations"]
        assert np.abs(T[:3, :3] - want[:3, :3]).max() < 0.02 and np.abs(T[:3, 3] - want[:3, 3]).max() < 0.02


def test_deterministic_and_batch_independent(icp):
    p = gfx.planted()
    src, Cp = p["starts"][0][:2]
    tgt, Cq, r = p["target"], p["target_covariances"], p["r"]
    rots = np.load(ROT64)["rotations"][:4]
    inits = ref.icp_inits(rots, tgt.mean(axis=0), src.mean(axis=0))
    assert len(inits) == 7
    a = _gicp(icp, src, Cp, tgt, Cq, r, inits, max_iteration=40)
    b = _gicp(icp, src, Cp, tgt, Cq, r, inits, max_iteration=40)
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert len(set(a.iterations.tolist())) > 1           # inits that stop at different passes
    for j in (0, 2, len(inits) - 1):
        s = _gicp(icp, src, Cp, tgt, Cq, r, inits[j], max_iteration=40)
        for f in FIELDS:
            assert np.array_equal(getattr(s, f)[0], getattr(a, f)[j]), (f, j)


def test_inputs_unmodified(icp):
    src, Cp, tgt, Cq, r, inits, _ = gfx.margin_fixture()
    inits = np.array(inits)
    dev = torch.device("cuda:0")
    S, P, Q, C = (torch.tensor(np.array(a), device=dev) for a in (src, Cp, tgt, Cq))
    S0, P0, Q0, C0, I0 = S.clone(), P.clone(), Q.clone(), C.clone(), inits.copy()
    icp.registration_icp(S, Q, r, inits, max_iteration=10, estimation="generalized", source_covariances=P, target_covariances=C)
    assert torch.equal(S, S0) and torch.equal(P, P0) and torch.equal(Q, Q0) and torch.equal(C, C0) and np.array_equal(inits, I0)


def test_covariance_forms_and_defaults(icp):
    src, Cp, tgt, Cq, r, inits, _ = gfx.margin_fixture()
    a = _gicp(icp, src, Cp, tgt, Cq, r, inits, max_iteration=5)
    full_p, full_q = gref.unpack(Cp).astype(np.float32), gref.unpack(Cq).astype(np.float32)
    b = icp.registration_icp(np.array(src), np.array(tgt), r, np.array(inits), max_iteration=5, estimation="generalized",
                             source_covariances=full_p, target_covariances=torch.tensor(full_q, device="cuda:0"))
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    # None: estimate_covariances of the cloud
    p = gfx.planted()
    s, _, T0, _, _ = p["starts"][0]
    tgt, r = p["target"], p["r"]
    kw = dict(max_iteration=10, estimation="generalized")
    default = icp.registration_icp(np.array(s), np.array(tgt), r, T0, **kw)
    Ep, Eq = icp.estimate_covariances(np.array(s)), icp.estimate_covariances(np.array(tgt))
    assert Ep.shape == (len(s), 6) and Ep.dtype == torch.float32 and Ep.is_cuda
    explicit = icp.registration_icp(np.array(s), np.array(tgt), r, T0, source_covariances=Ep, target_covariances=Eq, **kw)
    half = icp.registration_icp(np.array(s), np.array(tgt), r, T0, target_covariances=Eq, **kw)
    for f in FIELDS:
        assert np.array_equal(getattr(default, f), getattr(explicit, f)), f
        assert np.array_equal(getattr(default, f), getattr(half, f)), f
    assert default.fitness[0] > 0.9


def test_argument_errors(icp):
    src, Cp, tgt, Cq, r, inits, _ = gfx.margin_fixture()
    for bad_p, bad_q in ((Cp[:-1], Cq), (Cp, Cq[:-1]), (Cp, gref.unpack(Cq)[:-1])):
        with pytest.raises(ValueError):
            _gicp(icp, src, bad_p, tgt, bad_q, r, inits)
    for v in (np.nan, np.inf):
        bad = np.array(Cq)
        bad[3, 4] = v
        with pytest.raises(ValueError):
            _gicp(icp, src, Cp, tgt, bad, r, inits)
    bad = gref.unpack(Cp).astype(np.float32)
    bad[5, 0, 2] += 1e-3 * np.abs(bad[5]).max()
    with pytest.raises(ValueError, match="symmetric"):
        _gicp(icp, src, bad, tgt, Cq, r, inits)
    with pytest.raises(ValueError):
        icp.registration_icp(src, tgt, r, inits, estimation="generalised")


def test_null_covariance_pointer_is_invalid(icp):
    from scorp_amd import _C
    src, Cp, tgt, Cq, r, inits, _ = gfx.margin_fixture()
    dev = torch.device("cuda:0")
    S, P, Q, C = (torch.tensor(np.array(a), device=dev) for a in (src, Cp, tgt, Cq))
    T_in = torch.tensor(np.array(inits[:1]), device=dev)
    T_out = torch.empty_like(T_in)
    fit, rmse = torch.empty(1, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.float64, device=dev)
    iters = torch.empty(1, dtype=torch.int32, device=dev)
    L = _C.lib()
    size = L.scorp_icp_generalized_workspace_bytes(len(src), len(tgt), 1)
    assert size % 256 == 0 and size >= L.scorp_icp_point_to_plane_workspace_bytes(len(src), len(tgt), 1) + len(src) * 24
    ws = torch.empty(size, dtype=torch.uint8, device=dev)

    def run(p, c, bytes_=size):
        return L.scorp_icp_generalized(S.data_ptr(), p, len(src), Q.data_ptr(), c, len(tgt), T_in.data_ptr(), 1, r, 1, 0.0, 0.0,
                                       T_out.data_ptr(), fit.data_ptr(), rmse.data_ptr(), iters.data_ptr(), ws.data_ptr(), bytes_,
                                       _C.current_stream_ptr())

    for p, c in ((None, C.data_ptr()), (P.data_ptr(), None)):
        assert run(p, c) == _C.ERR_INVALID
        assert b"NULL" in L.scorp_last_error()
    # the workspace of the point-to-plane call is too small: the sorted covariances come after it
    assert run(P.data_ptr(), C.data_ptr(), L.scorp_icp_point_to_plane_workspace_bytes(len(src), len(tgt), 1)) == _C.ERR_INVALID
    assert b"workspace" in L.scorp_last_error()
    assert run(P.data_ptr(), C.data_ptr()) == 0
    torch.cuda.synchronize()


def test_best_transformation_finds_the_planted_pose(icp):
    p = gfx.planted()
    src, Cp, _, want, _ = p["starts"][0]
    tgt, Cq, r = p["target"], p["target_covariances"], p["r"]
    rots = np.load(ROT64)["rotations"][:4]
    best = icp.get_ICP_fitting_transformation_best(np.array(tgt), np.array(src), rots, r, estimation="generalized",
                                                   source_covariances=np.array(Cp), target_covariances=np.array(Cq))
    assert best.shape == (4, 4) and best.dtype == np.float64
    print(f"planted pair, 4 rotations: generalized |R - R0| {np.abs(best[:3, :3] - p['R0']).max():.3g}, "
          f"|t - t0| {np.abs(best[:3, 3] - p['t0']).max():.3g}")
    assert np.abs(best[:3, :3] - p["R0"]).max() < 0.02 and np.abs(best[:3, 3] - p["t0"]).max() < 0.02
    # a refined cloud more than 4x the original: the source covariances are subsampled with their points
    few, Cfew = np.array(tgt)[::10], np.array(Cq)[::10]
    keep = icp.downsample_indices(len(few), len(src))
    assert len(keep) == len(src) // 2
    best = icp.get_ICP_fitting_transformation_best(few, np.array(src), rots, r, estimation="generalized",
                                                   source_covariances=torch.tensor(np.array(Cp)), target_covariances=Cfew)
    inits = icp.icp_inits(rots, few.mean(axis=0), np.array(src).mean(axis=0))
    res = _gicp(icp, np.array(src)[keep], np.array(Cp)[keep], few, Cfew, r, inits, max_iteration=400)
    assert np.array_equal(best, res.transformation[int(np.argmax(res.fitness))])
    with pytest.raises(ValueError):
        icp.get_ICP_fitting_transformation_best(np.array(tgt), np.array(src), rots, r, estimation="generalized",
                                                source_covariances=np.array(Cp)[:-1])
