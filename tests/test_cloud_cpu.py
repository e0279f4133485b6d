"""The cloud module without a GPU: the yardstick (tests/cloud_reference.py) against scikit-learn's brute-force DBSCAN and
scipy's cKDTree on the fixtures, the properties the GPU tests rely on, the argument checks of scorp_amd/cloud.py,
keep_largest_clusters, and the binding."""
import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree
from sklearn.cluster import DBSCAN

from tests import cloud_fixtures as fx
from tests import cloud_reference as ref

# (fixture key, the offset that centring removes exactly, eps, min_points)
DBSCAN_CASES = {
    "blobs+100": (("blobs", 100.0), 100.0, fx.EPS, fx.MIN_POINTS),
    "blobs+4096": (("blobs", 4096.0), 4096.0, fx.EPS, fx.MIN_POINTS),
    "bridge": (("bridge",), 0.0) + fx.bridge()[1:],
    "chain": (("chain",), 20.0) + fx.chain()[1:],
}


def _radius_margin(P, radius):
    """the smallest |d2 - r^2| / r^2 over all pairs"""
    r2 = np.float64(radius) * np.float64(radius)
    return min(float(np.abs(ref.d2_rows(P, lo, hi) - r2).min()) for lo, hi in ref._chunks(len(P))) / r2


@pytest.mark.parametrize("name", sorted(DBSCAN_CASES))
def test_yardstick_dbscan_equals_sklearn(name):
    """Core flags, the partition of the core points and the noise set equal scikit-learn's DBSCAN(algorithm="brute").  It
    gets the float64 coordinates minus the fixture's offset - an exact subtraction, the same point set - because its
    distances come from |x|^2 + |y|^2 - 2 x.y, which loses the small differences of far-away points; no pair lies within
    1e-9 of eps^2, so its roundings decide nothing."""
    key, offset, eps, min_points = DBSCAN_CASES[name]
    P = fx.cloud(key)
    assert _radius_margin(P, eps) > 1e-9
    count, core, labels, num = fx.ref_dbscan(key, eps, min_points)
    sk = DBSCAN(eps=eps, min_samples=min_points, algorithm="brute").fit(P.astype(np.float64) - offset)
    sk_core = np.zeros(len(P), bool)
    sk_core[sk.core_sample_indices_] = True
    assert np.array_equal(core, sk_core)
    pairs = set(zip(labels[core].tolist(), sk.labels_[core].tolist()))
    assert len(pairs) == len(set(labels[core].tolist())) == len(set(sk.labels_[core].tolist())) == num
    assert np.array_equal(labels < 0, sk.labels_ < 0)
    # numbered in ascending order of the smallest core index
    firsts = [int(np.nonzero(core & (labels == c))[0][0]) for c in range(num)]
    assert firsts == sorted(firsts)


@pytest.mark.parametrize("key", [("blobs", 100.0), ("blobs", 4096.0), ("sized", 257), ("degenerate", "dense_cell")])
@pytest.mark.parametrize("k", [1, 20])
def test_yardstick_knn_means_agree_with_ckdtree(key, k):
    P = fx.cloud(key)
    mean, nb = fx.ref_knn(key, k)
    P64 = P.astype(np.float64)
    dd, _ = cKDTree(P64).query(P64, k=k)
    tree = dd.reshape(len(P), k)
    s = np.zeros(len(P))
    for a in range(k):
        s = s + tree[:, a]
    tree_mean = s / k
    assert np.all(np.abs(mean - tree_mean) <= (k + 2) * 2.0 ** -52 * np.maximum(mean, tree_mean))
    assert (nb[:, 0] <= np.arange(len(P))).all()   # d2 = 0 first: the point itself, or a duplicate of lower index


def test_fixture_properties():
    assert len(fx.blobs()) == 517 and fx.blobs().dtype == np.float32
    count, core, labels, num = fx.ref_dbscan(("blobs", 100.0), fx.EPS, fx.MIN_POINTS)
    assert num == 2 and (labels < 0).any() and ((labels >= 0) & ~core).any()          # two blobs, noise, border points
    # what an fp32 d2 would decide wrongly: nothing on the 517 points themselves (at +4096 it cannot: see blobs_fp32_traps),
    # every planted pair of the traps fixture - an fp32 implementation fails there
    r2 = np.float64(fx.EPS) * np.float64(fx.EPS)
    for key in (("blobs", 100.0), ("blobs", 4096.0), ("traps",)):
        P = fx.cloud(key)
        truth = ref.d2_rows(P, 0, len(P)) <= r2
        for fused in (False, True):
            wrong = (fx.d2_fp32(P[:, None, :], P[None, :, :], fused) <= np.float32(r2)) != truth
            print(f"{key}: {int(wrong.sum()) // 2} pairs an fp32 d2 (fused {fused}) decides wrongly")
            if key == ("traps",):
                rows = np.nonzero(wrong.any(1))[0]
                assert len(rows) == 16 and (rows >= 517).all()
    assert (fx.ref_count(("traps",), fx.EPS)[517:] == 1).all()      # in float64 every planted pair is just outside eps
    # the planted pair sits exactly on the radius
    for offset in (100.0, 4096.0):
        P = fx.blobs_exact_pair(offset)
        d2 = ref.d2_rows(P, len(P) - 2, len(P) - 1)[0, len(P) - 1]
        assert d2 == np.float64(fx.EXACT_RADIUS) * np.float64(fx.EXACT_RADIUS) == 25.0 / 4096.0
        assert fx.ref_count(("exact", offset), fx.EXACT_RADIUS)[-2:].tolist() == [2, 2]
    # the lattice: 19 neighbours inside
    c = fx.ref_count(("lattice",), np.sqrt(2.0)).reshape(16, 16, 16)
    assert (c[1:-1, 1:-1, 1:-1] == 19).all() and c[0, 0, 0] == 7
    # bridge: two clusters, the bridge point a border point; chain: one cluster
    P, eps, mp = fx.bridge()
    count, core, labels, num = fx.ref_dbscan(("bridge",), eps, mp)
    assert num == 2 and core[:-1].all() and not core[-1] and count[-1] == 3 and labels[-1] >= 0
    P, eps, mp = fx.chain()
    assert fx.ref_dbscan(("chain",), eps, mp)[3] == 1 and fx.ref_dbscan(("chain",), eps, mp)[1].all()
    # tie: the border point is exactly eps from a core point of each cube, and the lower core index wins
    for order, winner in (("ab", 0), ("ba", 0)):
        P, eps, mp = fx.tie(order)
        d2 = ref.d2_rows(P, len(P) - 1, len(P))[0]
        near = np.nonzero(d2 <= eps * eps)[0]
        assert len(near) == 3 and d2[near[0]] == d2[near[1]] == 2.25
        count, core, labels, num = fx.ref_dbscan(("tie", order), eps, mp)
        assert num == 2 and not core[-1] and labels[-1] == labels[near[0]] == winner
    # degenerate clouds
    assert len(np.unique(fx.degenerate("identical"), axis=0)) == 1
    assert fx.degenerate("plane")[:, 2].std() == 0.0
    dense = fx.degenerate("dense_cell")
    assert len(dense) == 2100 and dense[:2000].std(0).max() < 2e-3
    assert max(len(fx.cloud(("sized", n))) for n in fx.SIZES) <= 4200


@pytest.mark.parametrize("key, k, ratio", [(("blobs", 100.0), 20, 2.0), (("blobs", 4096.0), 20, 2.0), (("degenerate", "dense_cell"), 8, 1.0)])
def test_statistical_threshold_has_a_margin(key, k, ratio):
    """No k-nearest mean lies within 1e-9 of the outlier threshold: the last bits of the means and of the device's sums do
    not decide which points are kept."""
    mean, _ = fx.ref_knn(key, k)
    ind, thr, margin = ref.statistical_keep(mean, ratio)
    print(f"{key}: {len(mean) - len(ind)} outliers, margin {margin:.3g}")
    assert margin > 1e-9 and 0 < len(ind) < len(mean)


def test_argument_checks():
    from scorp_amd import cloud
    P = fx.blobs()
    bad = P.copy()
    bad[3, 1] = np.nan
    for call in (lambda p: cloud.knn_mean_distance(p), lambda p: cloud.radius_neighbor_count(p, 0.1),
                 lambda p: cloud.cluster_dbscan(p, 0.1, 4), lambda p: cloud.voxel_down_sample(p, 0.1),
                 lambda p: cloud.remove_statistical_outlier(p), lambda p: cloud.remove_radius_outlier(p, 4, 0.1)):
        with pytest.raises(ValueError, match="NaN"):
            call(bad)
        with pytest.raises(ValueError, match=r"\[n, 3\]"):
            call(P[:, :2])
        with pytest.raises(ValueError, match="empty"):
            call(P[:0])
    for k in (0, 33, -1, 2.5):
        with pytest.raises(ValueError, match="nb_neighbors"):
            cloud.knn_mean_distance(P, k)
    for r in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="radius"):
            cloud.radius_neighbor_count(P, r)
        with pytest.raises(ValueError, match="radius"):
            cloud.remove_radius_outlier(P, 4, r)
        with pytest.raises(ValueError, match="eps"):
            cloud.cluster_dbscan(P, r, 4)
        with pytest.raises(ValueError, match="voxel_size"):
            cloud.voxel_down_sample(P, r)
    with pytest.raises(ValueError, match="min_points"):
        cloud.cluster_dbscan(P, 0.1, 0)
    with pytest.raises(ValueError, match="nb_points"):
        cloud.remove_radius_outlier(P, -1, 0.1)
    with pytest.raises(ValueError, match="std_ratio"):
        cloud.remove_statistical_outlier(P, 20, np.nan)
    with pytest.raises(ValueError, match="colors"):
        cloud.voxel_down_sample(P, 0.1, colors=P[:10])
    with pytest.raises(ValueError, match="unknown method"):
        cloud.clean_gaussians(object(), method="hdbscan")
    with pytest.raises(TypeError, match="GaussianModel"):
        cloud.clean_gaussians(object(), method="dbscan", eps=0.1, min_points=4)


def test_keep_largest_clusters():
    from scorp_amd.cloud import keep_largest_clusters
    labels = torch.tensor([2, 0, 0, -1, 1, 1, 2, 2, -1, 3], dtype=torch.int32)
    assert keep_largest_clusters(labels).tolist() == [l == 2 for l in labels.tolist()]
    assert keep_largest_clusters(labels, 2).tolist() == [l in (2, 0) for l in labels.tolist()]      # 0 and 1 tie: the lower label
    assert keep_largest_clusters(labels, 3).tolist() == [l in (2, 0, 1) for l in labels.tolist()]
    assert keep_largest_clusters(labels, 9).tolist() == [l >= 0 for l in labels.tolist()]           # noise is never kept
    assert keep_largest_clusters(np.array([-1, -1])).tolist() == [False, False]
    assert keep_largest_clusters(torch.zeros(0, dtype=torch.int32)).tolist() == []
    assert keep_largest_clusters(labels).dtype == torch.bool
    with pytest.raises(ValueError, match="cluster_to_keep"):
        keep_largest_clusters(labels, 0)
    with pytest.raises(ValueError, match="integer tensor"):
        keep_largest_clusters(torch.zeros(4))


def test_binding_and_host_checks():
    """The new names are bound, the workspace grows with n, and the argument checks that need no device answer
    SCORP_ERR_INVALID before any HIP call (the dummy pointers are never dereferenced)."""
    from scorp_amd import _C
    names = ("scorp_cloud_workspace_bytes", "scorp_cloud_knn_distance", "scorp_cloud_radius_count", "scorp_cloud_dbscan")
    assert all(n in _C.EXPORTS for n in names)
    L = _C.lib()
    size = L.scorp_cloud_workspace_bytes(1000)
    assert 1000 * (16 + 16 + 16 + 13) <= size < L.scorp_cloud_workspace_bytes(100000)
    p = 0x10000   # non-zero, 256-byte aligned
    knn = lambda n=1000, k=20, pts=p, out=p, ws=p, sz=size: L.scorp_cloud_knn_distance(pts, n, k, out, None, ws, sz, None)
    count = lambda r=0.1, out=p: L.scorp_cloud_radius_count(p, 1000, r, out, p, size, None)
    scan = lambda eps=0.1, mp=4, labels=p, num=p: L.scorp_cloud_dbscan(p, 1000, eps, mp, labels, None, None, num, p, size, None)
    for reason, call in ((b"empty", lambda: knn(n=0)), (b"2^30", lambda: knn(n=2 ** 30 + 1, sz=2 ** 40)), (b"knn", lambda: knn(k=0)),
                         (b"knn", lambda: knn(k=33)), (b"NULL", lambda: knn(pts=None)), (b"NULL", lambda: knn(out=None)),
                         (b"workspace", lambda: knn(ws=None)), (b"workspace", lambda: knn(sz=size - 1)), (b"workspace", lambda: knn(ws=p + 64)),
                         (b"radius", lambda: count(r=0.0)), (b"radius", lambda: count(r=float("inf"))), (b"radius", lambda: count(r=float("nan"))),
                         (b"NULL", lambda: count(out=None)), (b"eps", lambda: scan(eps=-1.0)), (b"min_points", lambda: scan(mp=0)),
                         (b"NULL", lambda: scan(labels=None)), (b"NULL", lambda: scan(num=None))):
        assert call() == _C.ERR_INVALID and reason in L.scorp_last_error(), (reason, L.scorp_last_error())
