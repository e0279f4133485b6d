"""The ICP neighbour search, sorts and reductions (scorp_amd/csrc/icp.hip) against a float64 brute force, per query.

Part 1, the probe: a source of ONE point at the origin and inits[j] = translation by x_j make registration_icp answer
per query.  With max_iteration = 0, fitness[j] says whether x_j found a target point within r and inlier_rmse[j] is its
float64 distance; with max_iteration = 1 and both relative criteria 0 the update of a single pair is R = I, t = q - x,
so transformation[j][:3, 3] is the chosen target point itself.  The reference is all pairwise d^2 in float64 on the fp32
values, argmin with ties to the lowest index (tests/icp_probe_fixtures.py).

The slack.  E = the largest |coordinate - target bounding-box centre| over targets and queries, delta = 2^-20 E.  The
search runs on fp32 roundings of x - c_t and q - c_t, each coordinate off by at most 2^-24 E, so each distance by at
most about 2 sqrt(3) 2^-24 E plus a few fp32 ulps of the d^2 arithmetic; 16 x 2^-24 E covers that and is still a 1e-6
relative slack.  Always: a hit has d_chosen <= r and d_chosen <= d1 + delta, a miss has d1 > r - delta, and
inlier_rmse is the float64 distance to the point the translation names, to 1e-12 relative.  Where the margin holds
(d2 - d1 > 2 delta and |d1 - r| > 2 delta; d2 the nearest point at another position) the chosen point and the hit flag
equal the reference's exactly.  At most 5 % of a fixture's queries may lack the margin (tests/test_icp_cpu.py holds
every fixture to that with the reference alone); in the exact-tie fixture the documented rule, the lowest original
index among the tied points, is asserted for every query instead.

Part 2, the aggregate path: multi-point sources whose every point has the margin, at the block edges of the pass and
solve kernels (1024 source points per block, 64 rows per trip of the solve's loop).  Pair count exact, inlier_rmse to
1e-9 relative, and after one update transformation = kabsch_update(reference pairs) @ T0 to 10x the yardstick's own
sensitivity to the order of the pairs (floor 1e-13 (1 + extent)), the rule of tests/test_pose_fit_gpu.py.

Measured in one MI355X run (printed by the tests; DESIGN.md 4.10 holds the figures too):
  Probe, the largest d_chosen - d1 over a fixture's hits: 0 delta in every fixture (cube, plane, line, two_clusters,
  big_r, tiny_r, elongated, few1, few2, few3, dup64, tiles255, tiles256, tiles257, tiles1025, three_pass, offset, both
  shuffles of ties): every hit was the float64 nearest point itself, also at the queries without the margin.
  Share of the queries without the margin (cap 0.05): elongated 0.0087, line 0.0056, two_clusters 0.0044, plane 0.0007,
  offset 0.0003, every other fixture 0.0000; ties 1.0 by construction (asserted exactly instead).
  Aggregate path, |transformation - yardstick| (bound; the yardstick's own order sensitivity), init 0 / init 1:
  ns 1: 0 / 0 (1.9e-13; 0); 255: 6.7e-16 / 7.8e-16 (1.9e-13; 6.7e-16 / 5.0e-16); 256: 6.7e-16 / 5.6e-16 (1.9e-13;
  5.6e-16 / 4.4e-16); 257: 5.6e-16 / 2.3e-16 (1.9e-13; 6.7e-16 / 3.9e-16); 1023: 5.6e-16 / 9.0e-16 (1.9e-13; 5.6e-16 /
  1.1e-15); 1024: 5.6e-16 / 7.7e-16 (1.9e-13; 5.6e-16 / 8.3e-16); 1025: 8.9e-16 / 6.4e-16 (1.9e-13; 4.5e-16 / 2.5e-16);
  4097: 3.3e-16 / 5.6e-16 (1.9e-13; 5.6e-16 / 1.8e-15); 65536: 6.7e-16 / 6.4e-15 (1.9e-13; 4.6e-16 / 8.9e-15);
  66561: 6.0e-16 / 2.1e-15 (1.9e-13; 4.4e-16 / 3.7e-15).  The floor 1e-13 (1 + extent) = 1.9e-13 was the bound in
  every case; pair counts equal and inlier_rmse within 1e-9 relative everywhere.
"""
import numpy as np
import pytest
from scipy.spatial import cKDTree

from tests import icp_probe_fixtures as fx
from tests import icp_reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def icp():
    from scorp_amd import icp as m
    return m


def _probe(icp, tgt, q, r):
    """(the max_iteration = 0 result, the max_iteration = 1 result) of one point at the origin under a translation
    by every query."""
    src = np.zeros((1, 3), np.float32)
    inits = np.tile(np.eye(4), (len(q), 1, 1))
    inits[:, :3, 3] = q
    tgt = np.array(tgt)                       # (the fixtures are read-only; the front end wants a writable array)
    a = icp.registration_icp(src, tgt, r, inits, max_iteration=0)
    b = icp.registration_icp(src, tgt, r, inits, max_iteration=1, relative_fitness=0.0, relative_rmse=0.0)
    return a, b


def _describe(j, tgt, q, r, chosen, i1, d_chosen, d1, d2, delta):
    """One failing query for the message: the pair the kernel chose, the true one, and where the query sits in the
    grid (restated from the kernel's documented formulas)."""
    g = fx.grid_of(tgt)
    return (f"query {j} at {q[j].tolist()}: chose target {chosen} at distance {d_chosen!r}, the nearest is {i1} at {d1!r} "
            f"(runner-up {d2!r}), r {r!r}, delta {delta!r}; query cell {fx.cell_of(g, q[j]).tolist()}, "
            f"dims {g['dims'].tolist()}, h {g['h']!r}")


def _judge(name, tgt, q, r, reference, a, b, exact_ties=False):
    """Every assertion of part 1 on one probe; returns the largest d_chosen - d1 over the hits, in units of delta."""
    i1, d1, d2, _ = reference
    t64, q64 = tgt.astype(np.float64), q.astype(np.float64)
    E, delta = fx.slack(tgt, q)
    n = len(q)
    assert np.isin(a.fitness, (0.0, 1.0)).all()
    assert (a.iterations == 0).all() and (b.iterations == 1).all()
    hit = a.fitness == 1.0
    assert np.array_equal(b.fitness == 1.0, hit)               # the same search, before and after the update
    np.testing.assert_allclose(b.transformation[:, :3, :3], np.broadcast_to(np.eye(3), (n, 3, 3)), atol=1e-12)
    assert np.array_equal(a.transformation[:, :3, 3], q64)
    assert np.array_equal(b.transformation[~hit, :3, 3], q64[~hit])        # no pair: the init stays
    assert (a.inlier_rmse[~hit] == 0.0).all()
    # the chosen point, from the translation: an exact nearest match
    _, lowest = fx.positions_of(tgt)
    dist, near = cKDTree(t64).query(b.transformation[:, :3, 3])
    assert (dist[hit] <= 1e-9 * E).all(), f"{name}: a translation names no target point (off by {dist[hit].max()!r})"
    chosen = np.where(hit, lowest[near], -1)
    d_chosen = np.linalg.norm(q64 - t64[near], axis=1)
    want = np.where(d1 <= r, lowest[i1], -1)
    excess = float(((d_chosen - d1)[hit] / delta).max()) if hit.any() else 0.0
    margin = fx.has_margin(d1, d2, r, delta)
    print(f"{name}: {n} queries, {int(hit.sum())} hits, largest d_chosen - d1 = {excess:.3g} delta, "
          f"{np.mean(~margin):.4f} of the queries without the margin")

    def fail(bad, what):
        j = int(np.flatnonzero(bad)[0])
        return f"{name}: {what} at {int(bad.sum())} queries; " + _describe(j, tgt, q, r, int(chosen[j]), int(i1[j]),
                                                                         float(d_chosen[j]), float(d1[j]), float(d2[j]), delta)

    bad = hit & (np.abs(a.inlier_rmse - d_chosen) > 1e-12 * d_chosen)
    assert not bad.any(), fail(bad, "inlier_rmse is not the distance to the chosen point")
    bad = hit & ((a.inlier_rmse > r) | (d_chosen > r * (1.0 + 1e-12)))     # (d_chosen: this file's own rounding of it)
    assert not bad.any(), fail(bad, "a pair beyond r")
    bad = hit & (d_chosen > d1 + delta)
    assert not bad.any(), fail(bad, "a pair that is not the nearest")
    bad = ~hit & (d1 <= r - delta)
    assert not bad.any(), fail(bad, "a neighbour within r was missed")
    if exact_ties:
        assert hit.all()
        bad = chosen != i1
        assert not bad.any(), fail(bad, "a tie did not go to the lowest original index")
    else:
        assert np.mean(~margin) <= fx.MARGIN_CAP
        bad = margin & (chosen != want)
        assert not bad.any(), fail(bad, "with the margin, another point or hit flag than the reference's")
    return excess


@pytest.mark.parametrize("name", fx.MARGIN_FIXTURES)
def test_probe_matches_brute_force(icp, name):
    tgt, q, r, reference = fx.fixture(name)
    a, b = _probe(icp, tgt, q, r)
    _judge(name, tgt, q, r, reference, a, b)
    if name == "big_r":
        assert (a.fitness == 1.0).all()          # r = 3 x the extent: the rings run until the grid is exhausted


@pytest.mark.parametrize("shuffle", [0, 1])
def test_exact_ties_go_to_the_lowest_original_index(icp, shuffle):
    tgt, q, r, reference, _ = fx.ties_fixture(shuffle)
    a, b = _probe(icp, tgt, q, r)
    _judge(f"ties[{shuffle}]", tgt, q, r, reference, a, b, exact_ties=True)


def test_probe_is_independent_of_the_batch_order(icp):
    tgt, q, r, _ = fx.fixture("cube")
    a, b = _probe(icp, tgt, q, r)
    ar, br = _probe(icp, tgt, q[::-1], r)
    for x, y in ((a, ar), (b, br)):
        for f in ("transformation", "fitness", "inlier_rmse", "iterations"):
            assert np.array_equal(getattr(x, f), getattr(y, f)[::-1]), f


@pytest.mark.parametrize("ns", fx.AGGREGATE_NS)
def test_aggregate_path_at_block_edges(icp, ns):
    src, tgt, r, inits, pairs = fx.aggregate_fixture(ns)
    t64, s64 = tgt.astype(np.float64), src.astype(np.float64)
    extent = float(np.ptp(t64, axis=0).max())
    res0 = icp.registration_icp(np.array(src), np.array(tgt), r, inits, max_iteration=0)
    res1 = icp.registration_icp(np.array(src), np.array(tgt), r, inits, max_iteration=1, relative_fitness=0.0,
                                relative_rmse=0.0)
    order = np.random.default_rng(0)
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
        want = ref.kabsch_update(xs, qs) @ T0
        perm = order.permutation(c)
        own = float(np.abs(ref.kabsch_update(xs[perm], qs[perm]) @ T0 - want).max())
        bound = max(10.0 * own, 1e-13 * (1.0 + extent))
        d = float(np.abs(res1.transformation[j] - want).max())
        print(f"ns {ns} init {j}: {c} pairs, transformation to the yardstick {d:.3g} (bound {bound:.3g}, the yardstick's own "
              f"order sensitivity {own:.3g})")
        assert d <= bound
