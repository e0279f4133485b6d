"""Global registration without a GPU: the yardstick (tests/fpfh_reference.py) on hand-computed configurations, its
permutation equivariance, the margin cap on every fixture, orient_normals_away_from, the edge-length filter, the argument
checks of scorp_amd/global_registration.py, the binding, and the reference pipeline recovering the fixture's pose."""
import ctypes

import numpy as np
import pytest
import torch

from scorp_amd import global_registration as gr
from tests import fpfh_fixtures as fx
from tests import fpfh_reference as ref


def _row(**blocks):
    """a 33-vector with the given {bin: value} per block k0, k1, k2"""
    out = np.zeros(33)
    for k, name in enumerate(("k0", "k1", "k2")):
        for b, v in blocks.get(name, {}).items():
            out[11 * k + b] = v
    return out


def test_two_points_parallel_normals_perpendicular_to_dp():
    """dp = (1/4, 0, 0), both normals (0, 0, 1): a1 = a2 = 0, u = n_i, v = dp x u / |.| = (0, -1, 0), w = u x v = (1, 0, 0),
    f1 = atan2(0, 1) = 0, f2 = f3 = 0: bin floor(5.5) = 5 of each block.  m = 1, so spfh = 100 at those bins; the
    neighbour's row / d2 scaled to a total of 100 is 100 again: 200 at bins 5, 16 and 27."""
    P = np.array([[0, 0, 0], [0.25, 0, 0]], np.float32)
    N = np.array([[0, 0, 1], [0, 0, 1]], np.float32)
    r = ref.fpfh(P, N, 0.5, 4)
    assert r["neighbors"].tolist() == [[1, -1, -1, -1], [0, -1, -1, -1]] and r["degree"].tolist() == [1, 1]
    pf = ref.pair_features(P, N, np.array([0]), np.array([1]))
    assert pf["has"][0] and np.array_equal(pf["f"][0], [0.0, 0.0, 0.0]) and pf["bins"][0].tolist() == [5, 5, 5]
    assert np.all(np.abs(pf["margin"][0] - 0.5) < 1e-12) and pf["gap"][0] == 0.0
    want = _row(k0={5: 1}, k1={5: 1}, k2={5: 1})
    assert np.array_equal(r["count"], np.stack([want, want]).astype(np.int32))
    assert np.array_equal(r["feature"], np.stack([200.0 * want, 200.0 * want]))


def test_neighbour_along_the_normal_has_no_feature_but_counts_in_m():
    """Point 1 lies along point 0's normal: dp x u = 0, no feature for (0, 1) or (1, 0), but m counts it.  Point 2 is the
    configuration of the test above relative to point 0.  m_0 = 2 with one feature: spfh_0 = 50 at the three bins 5."""
    P = np.array([[0, 0, 0], [0, 0, 0.25], [0.25, 0, 0]], np.float32)
    N = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1]], np.float32)
    r = ref.fpfh(P, N, 0.3, 4)
    assert r["neighbors"][0].tolist() == [1, 2, -1, -1]      # equal d2: the lower index first
    assert r["degree"].tolist() == [2, 1, 1]                 # (1 and 2 are sqrt(2) / 4 > 0.3 apart)
    pf = ref.pair_features(P, N, np.array([0, 1]), np.array([1, 0]))
    assert not pf["has"].any() and np.all(np.isinf(pf["margin"]))
    assert np.array_equal(r["count"][0], _row(k0={5: 1}, k1={5: 1}, k2={5: 1}))
    assert np.array_equal(r["spfh"][0], _row(k0={5: 50.0}, k1={5: 50.0}, k2={5: 50.0}))
    assert not r["count"][1].any() and np.array_equal(r["spfh"][1], np.zeros(33))
    # F5 for point 1: its only neighbour 0 gives spfh_0 / d2, scaled to 100 per block; its own row is zero
    assert np.array_equal(r["feature"][1], _row(k0={5: 100.0}, k1={5: 100.0}, k2={5: 100.0}))


def test_duplicate_point_is_a_member_without_a_feature():
    """Points 0 and 1 coincide: each is in the other's list (self is left out by index, not by distance), f4 = 0 gives no
    feature, and F5 skips the pair (d2 = 0).  Point 2 sees both at the same d2: index order."""
    P = np.array([[0, 0, 0], [0, 0, 0], [0.25, 0, 0]], np.float32)
    N = np.array([[0, 0, 1], [0, 1, 0], [0, 0, 1]], np.float32)
    r = ref.fpfh(P, N, 0.5, 4)
    assert r["neighbors"].tolist() == [[1, 2, -1, -1], [0, 2, -1, -1], [0, 1, -1, -1]]
    assert r["degree"].tolist() == [2, 2, 2]
    assert r["count"].sum(1).tolist() == [3, 3, 6]
    assert np.all(np.isfinite(r["feature"]))
    # point 0: own spfh = 50 at bin 5 of each block; F5 runs over point 2 alone (the duplicate has d2 = 0)
    s = r["spfh"][2] / 0.0625
    for k in range(3):
        t = 0.0
        for e in range(11):
            t = t + s[11 * k + e]
        s[11 * k:11 * k + 11] = s[11 * k:11 * k + 11] * (100.0 / t)
    assert np.array_equal(r["feature"][0], s + r["spfh"][0])


def test_isolated_point_gives_a_zero_row():
    P = np.array([[0, 0, 0], [0.25, 0, 0], [5, 5, 5]], np.float32)
    N = np.array([[0, 0, 1], [0, 0, 1], [1, 0, 0]], np.float32)
    r = ref.fpfh(P, N, 0.5, 4)
    assert r["degree"].tolist() == [1, 1, 0] and r["neighbors"][2].tolist() == [-1] * 4
    assert np.array_equal(r["feature"][2], np.zeros(33)) and not r["count"][2].any()
    one = ref.fpfh(P[:1], N[:1], 0.5, 4)
    assert one["feature"].shape == (1, 33) and not one["feature"].any() and one["pairs"] == 0


@pytest.mark.parametrize("name", ["sized_65", "lattice", "duplicates", "surface_nn64"])
def test_yardstick_is_permutation_equivariant_bit_for_bit(name):
    """Permuting the input permutes features, counts and degrees exactly, and relabels the lists.  (With exact d2 ties the
    index decides a list's order and, where max_nn truncates, its members: there only the untied fixtures can be
    compared list by list, the lattice's tied ones by what does not depend on the labels.)"""
    P, N, radius, max_nn = fx.cases()[name]
    a = fx.ref_fpfh(name)
    perm = np.random.default_rng(5).permutation(len(P))
    b = ref.fpfh(P[perm], N[perm], radius, max_nn)
    assert np.array_equal(b["degree"], a["degree"][perm])
    if name == "lattice":
        return
    assert np.array_equal(b["count"], a["count"][perm])
    if name != "duplicates":   # (a duplicate pair ties: its two members swap places in a list, and with them F5's order)
        assert np.array_equal(b["feature"], a["feature"][perm])
        relabelled = np.where(b["neighbors"] >= 0, perm[np.where(b["neighbors"] >= 0, b["neighbors"], 0)], -1)
        assert np.array_equal(relabelled, a["neighbors"][perm])


@pytest.mark.parametrize("name", sorted(fx.cases()))
def test_margin_cap_on_every_fixture(name):
    r = fx.ref_fpfh(name)
    n = len(fx.cases()[name][0])
    excluded = int(r["excluded"].sum())
    close = int((r["pair_margin"] < ref.MARGIN).sum())
    print(f"{name}: {n} points, {r['pairs']} pairs, {close} bin coordinates within {ref.MARGIN} of an edge, {excluded} points excluded, "
          f"smallest margin {r['pair_margin'].min():.3g}")
    assert excluded <= fx.MARGIN_CAP * n
    assert r["neighbors"].shape == (n, fx.cases()[name][3]) and r["feature"].shape == (n, 33)


def test_fixtures_hold_the_cases_they_are_for():
    deg = {k: fx.ref_fpfh(k)["degree"] for k in fx.cases()}
    assert (deg["sparse_257"] == 0).any() and (deg["sparse_257"] > 0).any()
    for name in ("sized_63", "sized_257", "surface_nn1", "surface_nn64", "lattice"):
        assert (deg[name] == fx.cases()[name][3]).any(), name           # max_nn truncates
    assert deg["surface_all"].max() <= 64 and (deg["surface_all"] < 64).any()
    lat = fx.ref_fpfh("lattice_wide")
    want = np.zeros(33, bool)
    want[[5, 16, 27]] = True
    assert np.all((lat["count"] > 0) == want)                            # every pair lands in bin 5
    d2 = ref.d2_all(fx.cases()["lattice"][0])
    assert all(len(np.unique(row)) <= len(row) - 20 for row in d2)      # exact ties abound: 64 distances, 44 values at most
    along = fx.ref_fpfh("along_normal")
    assert along["neighbors"][0, 0] >= 0 and 1 in along["neighbors"][0] and along["count"][0].sum() == 3 * (along["degree"][0] - 1)
    dup = fx.cases()["duplicates"][0]
    assert np.array_equal(dup[:6], dup[59:])


def test_orient_normals_away_from():
    P = torch.tensor([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0]])
    N = torch.tensor([[1.0, 0, 0], [1.0, 0, 0], [1.0, 0, 0], [0, 1.0, 0]])
    out = gr.orient_normals_away_from(P, N)                 # the mean is the origin
    assert out.dtype == N.dtype
    assert out.tolist() == [[1, 0, 0], [-1, 0, 0], [1, 0, 0], [0, -1, 0]]      # row 2: a zero dot leaves n unchanged
    out = gr.orient_normals_away_from(P.numpy(), N.numpy(), center=[2.0, 0, 0])
    assert out.tolist() == [[-1, 0, 0], [-1, 0, 0], [-1, 0, 0], [0, -1, 0]]
    assert np.array_equal(ref.orient_away(P.numpy(), N.numpy(), [2.0, 0, 0]), out.numpy())
    pair = fx.registration_pair()
    est = pair["target_normals"] * np.where(np.arange(700) % 3 == 0, -1.0, 1.0).astype(np.float32)[:, None]
    assert np.array_equal(gr.orient_normals_away_from(pair["target"].copy(), est).numpy(), pair["target_normals"])   # star-shaped
    with pytest.raises(ValueError, match="normals"):
        gr.orient_normals_away_from(P, N[:3])
    with pytest.raises(ValueError, match="center"):
        gr.orient_normals_away_from(P, N, center=[0.0, 0.0])


def test_edge_length_filter_on_known_triples():
    S = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [2, 0, 0]], np.float64)
    T = S.copy()
    T[3] = [0, 0, 0.85]          # the edges 0-3 shrink to 0.85 of their length: below 0.9
    T[4] = [1.8, 0, 0]           # 0-4: exactly 0.9 (inclusive); 1-4: 0.8
    tri = np.array([[0, 1, 2], [0, 1, 3], [0, 2, 4], [1, 2, 4], [0, 0, 1], [2, 1, 2]])
    for mask in (gr.edge_length_mask(torch.from_numpy(S), torch.from_numpy(T), torch.from_numpy(tri[:4]), 0.9).numpy(),
                 ref.edge_length_mask(S, T, tri[:4], 0.9)):
        assert mask.tolist() == [True, False, True, False]
    kept = gr.select_triples(torch.from_numpy(S), torch.from_numpy(T), torch.from_numpy(tri), 0.9)
    assert kept.tolist() == [[0, 1, 2], [0, 2, 4]]           # repeated indices dropped first, the order kept
    assert gr.select_triples(torch.from_numpy(S), torch.from_numpy(T), torch.from_numpy(tri), 0.0).tolist() == tri[:4].tolist()


def test_wrappers_raise_value_errors_without_a_gpu():
    P, N = (np.array(a) for a in fx.surface(65, 165))
    F = np.zeros((65, 33))
    bad = P.copy()
    bad[3, 1] = np.nan
    for r in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="radius"):
            gr.compute_fpfh_feature(P, N, r)
        with pytest.raises(ValueError, match="max_correspondence_distance"):
            gr.registration_ransac_based_on_feature_matching(P, P, F, F, r)
        with pytest.raises(ValueError, match="threshold"):
            gr.get_FPFH_fitting_transformation(P, P, r)
        with pytest.raises(ValueError, match="voxel_size"):
            gr.get_FPFH_fitting_transformation(P, P, 0.1, voxel_size=r)
    for k in (0, 65, -1, 2.5):
        with pytest.raises(ValueError, match="max_nn"):
            gr.compute_fpfh_feature(P, N, 0.3, k)
    with pytest.raises(ValueError, match="normals"):
        gr.compute_fpfh_feature(P, N[:10], 0.3)
    with pytest.raises(ValueError, match="NaN"):
        gr.compute_fpfh_feature(P, bad, 0.3)
    with pytest.raises(ValueError, match="NaN"):
        gr.compute_fpfh_feature(bad, N, 0.3)
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        gr.compute_fpfh_feature(P[:, :2], N[:, :2], 0.3)
    with pytest.raises(ValueError, match="empty"):
        gr.compute_fpfh_feature(P[:0], N[:0], 0.3)
    for call in (lambda f: gr.match_features(f, F), lambda f: gr.match_features(F, f, mutual_filter=True)):
        with pytest.raises(ValueError, match=r"\[n, 33\]"):
            call(F[:, :32])
        with pytest.raises(ValueError, match=r"\[n, 33\]"):
            call(F[:0])
        with pytest.raises(ValueError, match="Inf"):
            call(np.where(np.arange(33) == 2, np.inf, F))
    ransac = gr.registration_ransac_based_on_feature_matching
    with pytest.raises(ValueError, match=r"source must be \[n, 3\]"):
        ransac(P[:, :2], P, F, F, 0.1)
    with pytest.raises(ValueError, match="target_feature"):
        ransac(P, P, F, F[:10], 0.1)
    with pytest.raises(ValueError, match="NaN"):
        ransac(P, bad, F, F, 0.1)
    with pytest.raises(ValueError, match="edge_length_threshold"):
        ransac(P, P, F, F, 0.1, edge_length_threshold=1.5)
    for h in (0, 65536, 2.5):
        with pytest.raises(ValueError, match="n_hypotheses"):
            ransac(P, P, F, F, 0.1, n_hypotheses=h)
    with pytest.raises(ValueError, match="samples"):
        ransac(P, P, F, F, 0.1, samples=np.zeros((4, 2), np.int64))
    with pytest.raises(ValueError, match="pc_xyz_refined"):
        gr.get_FPFH_fitting_transformation(P, P[:2], 0.1)
    with pytest.raises(ValueError, match="NaN"):
        gr.get_FPFH_fitting_transformation(bad, P, 0.1)


def test_binding_and_host_checks():
    """The new names are bound, the sizes are host arithmetic, the tile constant of the Python side is the library's, and
    the argument checks that need no device answer SCORP_ERR_INVALID before any HIP call (the dummy pointers are never
    dereferenced)."""
    from scorp_amd import _C
    names = ("scorp_cloud_fpfh_workspace_bytes", "scorp_cloud_fpfh", "scorp_feature_match_tile_rows", "scorp_feature_match_split_rows",
             "scorp_feature_match_workspace_bytes", "scorp_feature_match")
    assert all(n in _C.EXPORTS for n in names)
    L = _C.lib()
    assert L.scorp_feature_match_tile_rows() == gr.MATCH_TILE
    assert L.scorp_cloud_fpfh_workspace_bytes(1000, 64) >= L.scorp_cloud_workspace_bytes(1000) + 1000 * (64 + 1 + 33) * 4
    assert L.scorp_cloud_fpfh_workspace_bytes(1000, 1) < L.scorp_cloud_fpfh_workspace_bytes(1000, 64)
    for ns, nt in ((1, 1), (300, 300), (100000, 100000), (20000, 129)):
        rows = gr.match_split_rows(ns, nt)
        splits = -(-nt // rows)
        assert rows % gr.MATCH_TILE == 0 and rows >= gr.MATCH_TILE
        assert L.scorp_feature_match_workspace_bytes(ns, nt) >= ns * splits * 12
    assert gr.match_split_rows(300, 300) == gr.MATCH_TILE          # few source rows: one tile per split
    assert gr.match_split_rows(1 << 20, 300) > 300                 # enough source rows: one split
    dummy, f64 = 0x10000, ctypes.c_double
    size = L.scorp_cloud_fpfh_workspace_bytes(10, 8)

    def fpfh(points=dummy, normals=dummy, n=10, radius=0.1, max_nn=8, out=dummy, ws=dummy, ws_bytes=size):
        return L.scorp_cloud_fpfh(points, normals, n, f64(radius), max_nn, out, None, None, None, ws, ws_bytes, None)

    for kw in (dict(n=0), dict(n=-3), dict(n=(1 << 30) + 1), dict(radius=0.0), dict(radius=-1.0), dict(radius=float("inf")),
               dict(radius=float("nan")), dict(max_nn=0), dict(max_nn=65), dict(points=None), dict(normals=None), dict(out=None),
               dict(ws=None), dict(ws_bytes=size - 1), dict(ws=dummy + 8)):
        assert fpfh(**kw) == _C.ERR_INVALID, kw
        assert L.scorp_last_error()
    msize = L.scorp_feature_match_workspace_bytes(10, 10)

    def match(src=dummy, ns=10, tgt=dummy, nt=10, index=dummy, d2=dummy, ws=dummy, ws_bytes=msize):
        return L.scorp_feature_match(src, ns, tgt, nt, index, d2, ws, ws_bytes, None)

    for kw in (dict(ns=0), dict(nt=0), dict(ns=(1 << 30) + 1), dict(nt=(1 << 30) + 1), dict(src=None), dict(tgt=None), dict(index=None),
               dict(d2=None), dict(ws=None), dict(ws_bytes=msize - 1), dict(ws=dummy + 8)):
        assert match(**kw) == _C.ERR_INVALID, kw


def test_reference_match_rule():
    src, tgt = fx.integer_features(5, 9, straddle=(4,))
    index, d2 = ref.match(src, tgt)
    assert index[0] == 3 and d2[0] == 0.0                          # rows 3 and 4 are equal: the lower index
    brute = ((src[:, None, :].astype(np.float64) - tgt[None].astype(np.float64)) ** 2).sum(2)
    assert np.array_equal(d2, brute.min(1)) and np.array_equal(index, brute.argmin(1))   # integers: any order of the sum
    i2, _, mutual = ref.match_mutual(src, tgt)
    back, _ = ref.match(tgt, src)
    assert np.array_equal(mutual, back[i2] == np.arange(5)) and mutual[0]


def test_reference_pipeline_recovers_the_fixture_pose():
    """FPFH with the fixture's analytic normals, mutual matches, RANSAC on fixed triples: the float64 pipeline finds the
    120-degree pose well inside the GPU test's bound of 1 degree and 1 % of the diagonal."""
    pair = fx.registration_pair()
    fs, ft = fx.pair_features()
    index, _, mutual = ref.match_mutual(fs, ft)
    right = index == pair["subset"]
    samples, out = fx.pair_ransac()
    ang, dt = ref.pose_error(out["transformation"], pair["truth"])
    print(f"{int(right.sum())} of 500 nearest-feature matches right, {int(mutual.sum())} mutual ({int((right & mutual).sum())} right); "
          f"{len(out['counts'])} of {len(samples)} triples kept; winner {out['inlier_count']} inliers of {len(out['correspondences'])}; "
          f"rotation error {ang:.3f} deg, translation error {dt:.2e} on a diagonal of {pair['diagonal']:.3f}")
    assert right.sum() >= 250 and mutual.sum() >= 250
    assert out["inlier_count"] >= 200
    assert ang < 0.5 and dt < 0.005 * pair["diagonal"]
