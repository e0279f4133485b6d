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


# ---- the fixtures of the search probe (tests/test_icp_search_gpu.py), held to their properties by the float64
# reference alone: a GPU test cannot pass by having excluded its hard cases ----

from tests import icp_probe_fixtures as fx   # noqa: E402


@pytest.mark.parametrize("name", fx.MARGIN_FIXTURES)
def test_probe_fixture_meets_the_margin_cap(name):
    tgt, q, r, _ = fx.fixture(name)
    assert tgt.dtype == q.dtype == np.float32 and not tgt.flags.writeable and not q.flags.writeable
    E, delta = fx.slack(tgt, q)
    assert delta == E * 2.0 ** -20
    if name != "dup64":
        assert len(np.unique(tgt, axis=0)) == len(tgt) and fx.min_separation(tgt) >= fx.MIN_SEPARATION * E
    _, d1, d2, _ = fx.tree_nearest(tgt, q) + (None,) if name in fx.TREE_REFERENCE else fx.brute_nearest(tgt, q)
    lack = float(np.mean(~fx.has_margin(d1, d2, r, delta)))
    print(f"{name}: nt {len(tgt)}, {len(q)} queries, {lack:.4f} without the margin, {np.mean(d1 <= r):.3f} within r")
    assert lack <= fx.MARGIN_CAP
    assert 2000 <= len(q) <= 4000 or (name.startswith("tiles") and len(q) == 1000)
    assert len(tgt) <= 2000 or name == "three_pass"


@pytest.mark.parametrize("name", [n for n in fx.MARGIN_FIXTURES if n not in fx.TREE_REFERENCE])
def test_brute_force_agrees_with_ckdtree(name):
    tgt, q, r, (i1, d1, d2, ties) = fx.fixture(name)
    j1, e1, e2 = fx.tree_nearest(tgt, q)
    np.testing.assert_allclose(e1, d1, rtol=1e-12, atol=0)
    if name == "dup64":
        assert np.isinf(d2).all() and (ties == 1).all() and (i1 == 0).all()      # one position: no rival
        return
    np.testing.assert_allclose(e2, d2, rtol=1e-12, atol=0)
    clear = d2 > d1 * (1.0 + 1e-12)
    assert clear.mean() > 0.99 and np.array_equal(i1[clear], j1[clear])


def test_probe_fixtures_reach_their_grids():
    """By the restated grid formulas (fx.grid_of): each fixture builds the grid, and sends its queries to the cells, it
    is in the suite for."""
    def grid(name):
        tgt, q, r, ref_ = fx.fixture(name)
        g = fx.grid_of(tgt)
        return tgt, q, r, ref_, g, fx.cell_of(g, q)

    tgt, q, r, (_, d1, _, _), g, c = grid("cube")
    assert g["grow"] == 0 and g["dims"].min() >= 10 and g["radix_passes"] == 2
    below, at, above = c == -1, (c >= 0) & (c < g["dims"]), c == g["dims"]
    seen = {tuple(k) for k in (above.astype(int) - below.astype(int))}
    assert len(seen) == 27                                  # inside, and outside every face, edge and corner
    lo, hi = tgt.min(axis=0).astype(np.float64), tgt.max(axis=0).astype(np.float64)
    box = np.linalg.norm(np.maximum(np.maximum(lo - q, q - hi), 0.0), axis=1)
    out = ~at.all(axis=1)
    assert (out & (box < 0.7 * r)).sum() > 300 and (out & (box > 1.04 * r)).sum() > 300       # below and above r
    assert (out & (d1 <= r)).sum() > 50 and (out & (box < r) & (d1 > r)).sum() > 50             # hits and misses there
    assert (box > r * 1.001).sum() > 500                    # the early reject on the distance to the grid box
    assert (at.all(axis=1) & (d1 <= r)).sum() > 300 and (at.all(axis=1) & (d1 > r)).sum() > 300

    _, _, _, _, g, c = grid("plane")
    assert g["dims"][2] == 1 and g["grow"] >= 1 and {-1, 1} <= set(c[:, 2]) <= {-1, 0, 1}
    _, _, _, _, g, c = grid("line")
    assert g["dims"][1] == g["dims"][2] == 1 and g["dims"][0] > 500
    assert {-1, 1} <= set(c[:, 1]) and {-1, 1} <= set(c[:, 2])
    tgt, q, r, (i1, d1, _, _), g, c = grid("two_clusters")
    occupied = len({tuple(k) for k in fx.cell_of(g, tgt)})
    assert g["dims"][0] > 100 and occupied < 0.1 * np.prod(g["dims"])             # long runs of empty cells
    assert (d1 <= r).all() and r > 1.0                                              # r is longer than the gap
    own = fx.cell_of(g, tgt)[i1]
    assert (np.abs(own - c).max(axis=1) > 30).sum() > 500                           # many rings before the first point
    tgt, q, r, (_, d1, _, _), g, c = grid("big_r")
    assert (d1 <= r).all() and r >= 3.0 * np.ptp(tgt, axis=0).max() * (1 - 1e-6)
    tgt, q, r, (_, d1, _, _), g, c = grid("tiny_r")
    assert np.mean(d1 > r) > 0.8 and (d1 <= r).sum() > 100
    _, _, _, _, g, c = grid("elongated")
    assert g["h"] == g["floor"] and list(g["dims"]) == [1024, 1, 1] and g["grow"] == 0    # the maxe / 1024 floor
    for name in ("few1", "dup64"):
        tgt, _, _, _, g, _ = grid(name)
        assert np.ptp(tgt, axis=0).max() == 0.0 and g["pad"] == 1e-6 * max(1.0, np.abs(g["ct"]).sum())   # maxe == 0
    assert len(fx.fixture("few2")[0]) == 2 and len(fx.fixture("few3")[0]) == 3
    for nt in (255, 256, 257, 1025):
        assert len(fx.fixture(f"tiles{nt}")[0]) == nt
    _, _, _, _, g, _ = grid("three_pass")
    assert g["cap"] > 65536 and g["radix_passes"] == 3
    tgt, q, _, _, g, _ = grid("offset")
    assert np.abs(g["ct"]).min() > 999.0 and fx.slack(tgt, q)[0] < 3.0                 # delta does not grow with the offset


def test_ties_fixture_is_exact():
    first = None
    for shuffle in (0, 1):
        tgt, q, r, (i1, d1, d2, ties), order = fx.ties_fixture(shuffle)
        assert np.array_equal(np.sort(order), np.arange(512)) and r == 2.0
        assert np.array_equal(tgt, np.rint(tgt)) and np.array_equal(2 * q, np.rint(2 * q))          # fp32-exact
        assert np.array_equal(fx.centre_of(tgt), [3.5, 3.5, 3.5])
        assert np.array_equal(np.bincount(ties), [0, 0, 1344, 0, 1176, 0, 0, 0, 343])             # edges, faces, cells
        assert np.array_equal(d1, np.sqrt(np.log2(ties) / 4.0))                                    # d^2 = 0.25, 0.5, 0.75
        # the lowest original index among the exactly tied points, restated without the brute force's argmin
        t64, q64 = tgt.astype(np.float64), q.astype(np.float64)
        for j in range(0, len(q), 37):
            dd = ((t64 - q64[j]) ** 2).sum(axis=1)
            assert i1[j] == np.flatnonzero(dd == dd.min())[0] and (dd == dd.min()).sum() == ties[j]
        lattice = order[i1]                                   # which lattice point won: depends on the shuffle
        if first is None:
            first = lattice
        else:
            assert np.mean(lattice != first) > 0.3


@pytest.mark.parametrize("ns", fx.AGGREGATE_NS)
def test_aggregate_fixture_has_the_margin_everywhere(ns):
    src, tgt, r, inits, pairs = fx.aggregate_fixture(ns)
    assert src.shape == (ns, 3) and src.dtype == np.float32 and len(inits) == 2 and len(tgt) == 1000
    assert np.array_equal(inits[0], np.eye(4)) and not np.array_equal(inits[1], np.eye(4))
    for T, (hit, idx) in zip(inits, pairs):
        x = src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]
        _, delta = fx.slack(tgt, x)
        i1, d1, d2 = fx.tree_nearest(tgt, x)
        assert fx.has_margin(d1, d2, r, delta).all()
        assert np.array_equal(i1, idx) and np.array_equal(d1 <= r, hit)
        assert hit.sum() >= 1 and (ns < 255 or (~hit).sum() >= 1)                # pairs, and points without one


def test_aggregate_sizes_reach_the_block_edges():
    blocks = [-(-ns // 1024) for ns in fx.AGGREGATE_NS]        # 1024 source points per pass block
    assert {1, 2, 5, 64, 66} <= set(blocks) and max(fx.AGGREGATE_NS) % 1024 != 0        # (a ragged last block)
    assert {255, 256, 257, 1023, 1024, 1025, 64 * 1024} <= set(fx.AGGREGATE_NS)
