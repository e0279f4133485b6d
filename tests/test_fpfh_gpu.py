"""The global-registration kernels (csrc/cloud_fpfh.hip, csrc/feature_match.hip through scorp_amd/global_registration.py)
on the GPU against the float64 brute force of tests/fpfh_reference.py.  Neighbour lists and degrees are asserted EQUAL;
the SPFH counts EQUAL on every point not margin-excluded (a pair of its own list has a bin coordinate within 1e-9 of an
integer, where atan2's last place may decide the bin); the descriptor BIT FOR BIT on every point that is not excluded and
whose own list and whose neighbours' lists hold no excluded point.  Matches: indices EQUAL, D2 bit for bit.

Left out by the margin rule, as printed by these tests on an MI355X: 0 points of every fixture."""
import ctypes
import os

import numpy as np
import pytest
import torch

from scorp_amd import global_registration as gr
from tests import fpfh_fixtures as fx
from tests import fpfh_reference as ref

pytestmark = pytest.mark.gpu

ROT64 = os.path.join(os.path.dirname(__file__), "golden", "rotations_64.npz")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need a GPU"
    from scorp_amd import _C
    _C.lib()
    return torch.device("cuda:0")


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def fpfh_abi(P, N, radius, max_nn, dev, optional=True, fill=None):
    """scorp_cloud_fpfh through the C ABI: (feature, count, neighbors, degree) as numpy arrays, the last three None when
    `optional` is off (NULL pointers)."""
    from scorp_amd import _C
    P = torch.from_numpy(np.array(P)).to(dev)
    N = torch.from_numpy(np.array(N)).to(dev)
    n = P.shape[0]
    feature = torch.full((n, 33), -7.0, dtype=torch.float64, device=dev)
    count = torch.full((n, 33), -7, dtype=torch.int32, device=dev) if optional else None
    nb = torch.full((n, max_nn), -7, dtype=torch.int32, device=dev) if optional else None
    deg = torch.full((n,), -7, dtype=torch.int32, device=dev) if optional else None
    size = _C.lib().scorp_cloud_fpfh_workspace_bytes(n, max_nn)
    workspace = torch.empty(size, dtype=torch.uint8, device=dev)
    if fill is not None:
        workspace.fill_(fill)
    _C.call("scorp_cloud_fpfh", P, N, n, float(radius), int(max_nn), feature, count, nb, deg, workspace, size)
    torch.cuda.synchronize()
    return tuple(None if t is None else _np(t) for t in (feature, count, nb, deg))


@pytest.mark.parametrize("name", sorted(fx.cases()))
def test_fpfh_equals_the_reference(name, dev):
    P, N, radius, max_nn = fx.cases()[name]
    r = fx.ref_fpfh(name)
    feature, count, nb, deg = fpfh_abi(P, N, radius, max_nn, dev)
    assert nb.dtype == np.int32 and nb.shape == (len(P), max_nn) and feature.dtype == np.float64 and feature.shape == (len(P), 33)
    np.testing.assert_array_equal(nb, r["neighbors"])
    np.testing.assert_array_equal(deg, r["degree"])
    keep = ~r["excluded"]
    ok = r["feature_ok"]
    count_diff = int((count != r["count"]).any(1).sum())
    print(f"fpfh {name}: {len(P)} points, {r['pairs']} pairs; left out of the count check {int((~keep).sum())}, of the descriptor check "
          f"{int((~ok).sum())}; rows whose counts differ {count_diff}, descriptor rows bit-equal "
          f"{int((_bits(feature) == _bits(r['feature'])).all(1).sum())}")
    np.testing.assert_array_equal(count[keep], r["count"][keep])
    bad = np.nonzero((_bits(feature) != _bits(r["feature"])).any(1) & ok)[0]
    assert len(bad) == 0, (f"{len(bad)} descriptor rows with equal counts differ in their bits (the order of a sum is wrong): first {bad[:5]}, "
                           f"largest difference {np.abs(feature[bad] - r['feature'][bad]).max():.3g}")


@pytest.mark.parametrize("name", ["sized_257", "surface_nn64", "lattice"])
def test_fpfh_twice_the_same_bits_and_null_outputs(name, dev):
    """Two calls give the same bits whatever the workspace held before, and with the optional outputs NULL the descriptor
    is the same (neighbour list, degrees and counts then live in the workspace)."""
    P, N, radius, max_nn = fx.cases()[name]
    a = fpfh_abi(P, N, radius, max_nn, dev, fill=0)
    b = fpfh_abi(P, N, radius, max_nn, dev, fill=255)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    c = fpfh_abi(P, N, radius, max_nn, dev, optional=False, fill=255)
    assert c[1] is None and c[2] is None and c[3] is None
    assert np.array_equal(_bits(c[0]), _bits(a[0]))


def test_fpfh_python_wrapper_and_permutation(dev):
    """compute_fpfh_feature returns what the C ABI returns, and permuting the input permutes the output exactly."""
    P, N, radius, max_nn = fx.cases()["surface_all"]
    f, nb, deg, cnt = gr.compute_fpfh_feature(np.array(P), torch.from_numpy(np.array(N)), radius, max_nn, return_neighbors=True)
    assert f.is_cuda and f.dtype == torch.float64 and nb.dtype == torch.int32
    r = fx.ref_fpfh("surface_all")
    np.testing.assert_array_equal(_np(nb), r["neighbors"])
    np.testing.assert_array_equal(_np(deg), r["degree"])
    only = gr.compute_fpfh_feature(torch.from_numpy(np.array(P)).to(dev), np.array(N), radius, max_nn)
    assert np.array_equal(_bits(_np(only)), _bits(_np(f)))
    perm = np.random.default_rng(9).permutation(len(P))
    g, _, gdeg, gcnt = gr.compute_fpfh_feature(P[perm], N[perm], radius, max_nn, return_neighbors=True)
    np.testing.assert_array_equal(_np(gdeg), _np(deg)[perm])
    np.testing.assert_array_equal(_np(gcnt), _np(cnt)[perm])
    assert np.array_equal(_bits(_np(g)), _bits(_np(f)[perm]))


def test_fpfh_invalid_arguments(dev):
    from scorp_amd import _C
    L = _C.lib()
    n, max_nn = 65, 7
    P = torch.from_numpy(np.array(fx.cases()["sized_65"][0])).to(dev)
    N = torch.from_numpy(np.array(fx.cases()["sized_65"][1])).to(dev)
    out = torch.empty(n, 33, dtype=torch.float64, device=dev)
    size = L.scorp_cloud_fpfh_workspace_bytes(n, max_nn)
    ws = torch.empty(size + 256, dtype=torch.uint8, device=dev)
    base = (ws.data_ptr() + 255) // 256 * 256
    good = dict(points=P.data_ptr(), normals=N.data_ptr(), n=n, radius=0.3, max_nn=max_nn, out=out.data_ptr(), ws=base, ws_bytes=size)

    def call(**kw):
        a = {**good, **kw}
        return L.scorp_cloud_fpfh(a["points"], a["normals"], a["n"], ctypes.c_double(a["radius"]), a["max_nn"], a["out"], None, None, None,
                                  a["ws"], a["ws_bytes"], None)

    assert call() == 0
    for kw in (dict(n=0), dict(n=-1), dict(n=(1 << 30) + 1), dict(radius=0.0), dict(radius=-0.3), dict(radius=float("inf")),
               dict(radius=float("nan")), dict(max_nn=0), dict(max_nn=65), dict(points=None), dict(normals=None), dict(out=None),
               dict(ws=None), dict(ws_bytes=size - 1), dict(ws=base + 16)):
        assert call(**kw) == _C.ERR_INVALID, kw
        assert L.scorp_last_error()
    torch.cuda.synchronize()


# ---- match ----

def check_match(src, tgt, dev):
    index, d2, mutual = gr.match_features(torch.from_numpy(np.array(src)).to(dev), np.array(tgt), mutual_filter=True)
    assert index.dtype == torch.int32 and d2.dtype == torch.float64 and mutual.dtype == torch.bool
    ri, rd, rm = ref.match_mutual(src, tgt)
    np.testing.assert_array_equal(_np(index), ri)
    assert np.array_equal(_bits(_np(d2)), _bits(rd))
    np.testing.assert_array_equal(_np(mutual), rm)
    i2, d22 = gr.match_features(src, tgt)
    np.testing.assert_array_equal(_np(i2), ri)
    assert np.array_equal(_bits(_np(d22)), _bits(rd))


@pytest.mark.parametrize("ns", [1, 63, 64, 65, 300])
def test_match_integer_features_lower_index_wins(ns, dev):
    """Integer-valued rows with duplicated target rows; a duplicate pair sits across every tile edge, which for so few
    source rows is a split edge too (one tile per split)."""
    tile = gr.MATCH_TILE
    for nt in (1, tile - 1, tile, tile + 1, 2 * tile + 1, 300):
        assert gr.match_split_rows(ns, nt) == tile
        src, tgt = fx.integer_features(ns, nt, straddle=(tile, 2 * tile, 4 * tile))
        check_match(src, tgt, dev)


def _integer_match(src, tgt):
    """M1 for integer-valued rows by exact integer arithmetic (every D2 is an integer far below 2^53, so the order of the
    sum cannot matter): |a|^2 + |b|^2 - 2 a.b in float64, chunked."""
    S, T = src.astype(np.float64), tgt.astype(np.float64)
    index, best = np.empty(len(S), np.int32), np.empty(len(S))
    t2 = (T * T).sum(1)
    for lo in range(0, len(S), 8192):
        D = (S[lo:lo + 8192] ** 2).sum(1)[:, None] + t2[None] - 2.0 * (S[lo:lo + 8192] @ T.T)
        arg = D.argmin(1)
        index[lo:lo + 8192], best[lo:lo + 8192] = arg, D[np.arange(len(arg)), arg]
    return index, best


@pytest.mark.parametrize("ns, nt", [(153600, 129), (76800, 449)])
def test_match_many_source_rows_several_tiles_per_split(ns, nt, dev):
    """Enough source rows that a split of the target holds several tiles (153 600 rows: one split of three tiles; 76 800:
    three splits of three tiles), with a duplicate pair across every tile edge and so across every split edge."""
    tile = gr.MATCH_TILE
    rows = gr.match_split_rows(ns, nt)
    assert rows == 3 * tile
    edges = tuple(range(tile, nt, tile))
    src, tgt = fx.integer_features(ns, nt, straddle=edges)
    assert any(e % rows == 0 for e in edges) or nt <= rows
    index, d2 = gr.match_features(torch.from_numpy(np.array(src)).to(dev), torch.from_numpy(np.array(tgt)).to(dev))
    ri, rd = _integer_match(src, tgt)
    np.testing.assert_array_equal(_np(index), ri)
    np.testing.assert_array_equal(_np(d2), rd)
    for k, e in enumerate(edges):
        assert _np(index)[k] == e - 1 and _np(d2)[k] == 0.0


def test_match_real_fpfh_rows(dev):
    fs, ft = fx.pair_features()
    check_match(fs, ft, dev)
    check_match(ft, fs, dev)
    check_match(fs[:1], ft, dev)


def test_match_invalid_arguments(dev):
    from scorp_amd import _C
    L = _C.lib()
    S = torch.zeros(10, 33, device=dev)
    index = torch.empty(10, dtype=torch.int32, device=dev)
    d2 = torch.empty(10, dtype=torch.float64, device=dev)
    size = L.scorp_feature_match_workspace_bytes(10, 10)
    ws = torch.empty(size + 256, dtype=torch.uint8, device=dev)
    base = (ws.data_ptr() + 255) // 256 * 256
    good = dict(src=S.data_ptr(), ns=10, tgt=S.data_ptr(), nt=10, index=index.data_ptr(), d2=d2.data_ptr(), ws=base, ws_bytes=size)

    def call(**kw):
        a = {**good, **kw}
        return L.scorp_feature_match(a["src"], a["ns"], a["tgt"], a["nt"], a["index"], a["d2"], a["ws"], a["ws_bytes"], None)

    assert call() == 0
    for kw in (dict(ns=0), dict(nt=0), dict(ns=-1), dict(ns=(1 << 30) + 1), dict(nt=(1 << 30) + 1), dict(src=None), dict(tgt=None),
               dict(index=None), dict(d2=None), dict(ws=None), dict(ws_bytes=size - 1), dict(ws=base + 16)):
        assert call(**kw) == _C.ERR_INVALID, kw
    torch.cuda.synchronize()
    assert _np(index).tolist() == [0] * 10 and not _np(d2).any()      # ten equal rows: the lowest index


# ---- registration ----

def test_ransac_registration_on_the_fixture_pair(dev):
    """Analytic normals, the GPU's own descriptors, fixed triples: the correspondences EQUAL the reference's, and the pose
    is within 1 degree and 1 % of the bounding-box diagonal of the truth (the float64 reference pipeline:
    0.21 degrees and 2.8e-3 on a diagonal of 2.48; the GPU gave the same figures)."""
    pair = fx.registration_pair()
    samples, want = fx.pair_ransac()
    fs = gr.compute_fpfh_feature(np.array(pair["source"]), np.array(pair["source_normals"]), fx.SURFACE_RADIUS, fx.SURFACE_MAX_NN)
    ft = gr.compute_fpfh_feature(np.array(pair["target"]), np.array(pair["target_normals"]), fx.SURFACE_RADIUS, fx.SURFACE_MAX_NN)
    out = gr.registration_ransac_based_on_feature_matching(np.array(pair["source"]), np.array(pair["target"]), fs, ft, fx.RANSAC_DISTANCE,
                                                           samples=np.array(samples))
    np.testing.assert_array_equal(out.correspondences, want["correspondences"])
    ang, dt = ref.pose_error(out.transformation, pair["truth"])
    print(f"ransac: {len(out.correspondences)} correspondences, {len(out.counts)} triples kept, winner {out.inlier_count} inliers "
          f"(reference {want['inlier_count']}), rotation error {ang:.3f} deg, translation error {dt:.2e} of diagonal {pair['diagonal']:.3f}")
    assert len(out.counts) == len(want["counts"])
    assert out.inlier_mask.sum() == out.inlier_count and out.fitness == out.inlier_count / len(out.correspondences)
    assert ang < 1.0 and dt < 0.01 * pair["diagonal"]
    seeded = gr.registration_ransac_based_on_feature_matching(np.array(pair["source"]), np.array(pair["target"]), fs, ft,
                                                              fx.RANSAC_DISTANCE, seed=4)
    ang, dt = ref.pose_error(seeded.transformation, pair["truth"])
    assert ang < 1.0 and dt < 0.01 * pair["diagonal"]
    with pytest.raises(ValueError, match="No inliers"):
        gr.registration_ransac_based_on_feature_matching(np.array(pair["source"]), np.array(pair["target"]), fs, ft, 1e-7,
                                                         samples=np.array(samples))
    with pytest.raises(ValueError, match="no sample triple"):
        gr.registration_ransac_based_on_feature_matching(np.array(pair["source"]), np.array(pair["target"]), fs, ft, fx.RANSAC_DISTANCE,
                                                         samples=np.array([[0, 0, 1], [2, 1, 2]]))


def test_fpfh_fitting_transformation_on_the_fixture_pair(dev):
    """The whole route with ESTIMATED normals (voxel grid, estimate_normals + orientation, FPFH, RANSAC, one ICP run): after
    its ICP the pose is within 0.5 degrees and 0.5 % of the diagonal of the truth, and its ICP fitness is at least that of
    the 67-start sweep with the rotations_64 table on the same pair, minus 0.01."""
    from scorp_amd import icp
    pair = fx.registration_pair()
    orig, refined = np.array(pair["target"]), np.array(pair["source"])
    threshold = float(np.ptp(orig, axis=0).mean() * 0.16)              # the alignment script's ICP radius
    T, res = gr.get_FPFH_fitting_transformation(orig, refined, threshold, return_icp=True)
    assert T.shape == (4, 4) and T.dtype == np.float64
    ang, dt = ref.pose_error(T, pair["truth"])
    sweep = icp.get_ICP_fitting_transformation_best(orig, refined, np.load(ROT64)["rotations"], threshold)
    fit = [float(icp.registration_icp(refined, orig, threshold, M, max_iteration=0).fitness[0]) for M in (T, sweep)]
    sang, sdt = ref.pose_error(sweep, pair["truth"])
    print(f"global route: rotation error {ang:.4f} deg, translation error {dt:.2e} of diagonal {pair['diagonal']:.3f}, ICP fitness "
          f"{fit[0]:.4f} after {int(res.iterations[0])} updates; sweep: {sang:.4f} deg, {sdt:.2e}, fitness {fit[1]:.4f}")
    assert ang < 0.5 and dt < 0.005 * pair["diagonal"]
    assert fit[0] >= fit[1] - 0.01
    assert abs(fit[0] - float(res.fitness[0])) < 0.01
