"""The cloud kernels (csrc/cloud_filter.hip through scorp_amd/cloud.py) on the GPU against the float64 brute force of
tests/cloud_reference.py: counts, neighbour lists, core flags, labels and cluster counts are asserted EQUAL, the k-nearest
means within (k + 2) 2^-52 relative - k additions and the square roots at half an ulp each, plus slack."""
import numpy as np
import pytest
import torch

from tests import cloud_fixtures as fx
from tests import cloud_reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need a GPU"
    from scorp_amd import _C
    _C.lib()
    return torch.device("cuda:0")


def _np(t):
    return t.cpu().numpy()


def check_knn(key, k, dev):
    from scorp_amd import cloud
    P = fx.cloud(key)
    mean_ref, nb_ref = fx.ref_knn(key, k)
    mean, nb = cloud.knn_mean_distance(torch.from_numpy(P.copy()).to(dev), k, return_neighbors=True)
    mean, nb = _np(mean), _np(nb)
    assert nb.dtype == np.int32 and nb.shape == (len(P), k) and mean.dtype == np.float64
    np.testing.assert_array_equal(nb, nb_ref)
    scale = np.maximum(np.abs(mean_ref), np.abs(mean))
    worst = float((np.abs(mean - mean_ref) / np.where(scale > 0, scale, 1.0)).max())
    print(f"knn {key} k={k}: means bit-equal {np.array_equal(mean, mean_ref)}, worst relative deviation {worst:.3g}")
    assert np.all(np.abs(mean - mean_ref) <= (min(k, len(P)) + 2) * 2.0 ** -52 * scale)


def check_count(key, radius, dev):
    from scorp_amd import cloud
    count = _np(cloud.radius_neighbor_count(fx.cloud(key).copy(), radius))   # (a numpy array goes in as it is)
    assert count.dtype == np.int32
    np.testing.assert_array_equal(count, fx.ref_count(key, radius))
    return count


def check_dbscan(key, eps, min_points, dev):
    """labels, core flags, counts and the number of clusters, through the C ABI so that every output is looked at"""
    from scorp_amd import _C
    P = torch.from_numpy(fx.cloud(key).copy()).to(dev)
    n = P.shape[0]
    count_ref, core_ref, labels_ref, num_ref = fx.ref_dbscan(key, eps, min_points)
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    core = torch.empty(n, dtype=torch.uint8, device=dev)
    count = torch.empty(n, dtype=torch.int32, device=dev)
    num = torch.full((1,), -7, dtype=torch.int32, device=dev)
    size = _C.lib().scorp_cloud_workspace_bytes(n)
    workspace = torch.empty(size, dtype=torch.uint8, device=dev)
    _C.call("scorp_cloud_dbscan", P, n, float(eps), int(min_points), labels, core, count, num, workspace, size)
    np.testing.assert_array_equal(_np(count), count_ref)
    np.testing.assert_array_equal(_np(core).astype(bool), core_ref)
    np.testing.assert_array_equal(_np(labels), labels_ref)
    assert int(num) == num_ref
    return _np(labels), _np(core).astype(bool), int(num)


# ---- sizes at the edges ----

@pytest.mark.parametrize("n", fx.SIZES)
def test_sizes_knn(n, dev):
    for k in fx.KNNS:                      # (k > n pads with -1: n = 1, 2, 3 meet it at k = 2, 20, 32)
        check_knn(("sized", n), k, dev)


@pytest.mark.parametrize("n", fx.SIZES)
def test_sizes_count_and_dbscan(n, dev):
    radius = fx.sized(n)[1]
    check_count(("sized", n), radius, dev)
    check_dbscan(("sized", n), radius, fx.SIZED_MIN_POINTS, dev)


def test_knn_above_n_pads(dev):
    from scorp_amd import cloud
    P = fx.cloud(("sized", 3))
    mean, nb = cloud.knn_mean_distance(P, 20, return_neighbors=True)
    assert (_np(nb)[:, 3:] == -1).all() and (_np(nb)[:, :3] >= 0).all()
    assert cloud.knn_mean_distance(P, 20, return_neighbors=False).shape == (3,)


# ---- precision ----

@pytest.mark.parametrize("offset", [100.0, 4096.0])
def test_precision_blobs(offset, dev):
    """the 517 points far from the origin: the grid files them by coarse fp32 coordinates relative to the box centre, the
    decisions are float64 on the original ones (what an fp32 d2 gets wrong is test_precision_fp32_traps's)"""
    key = ("blobs", offset)
    check_count(key, fx.EPS, dev)
    check_knn(key, 20, dev)
    labels, core, num = check_dbscan(key, fx.EPS, fx.MIN_POINTS, dev)
    assert num == 2


def test_precision_fp32_traps(dev):
    """8 planted pairs whose d2 an fp32 evaluation, plain or fused, puts on the wrong side of eps^2 (asserted on the fixture in
    tests/test_cloud_cpu.py): an implementation that decides on an fp32 d2 fails here"""
    key = ("traps",)
    count = check_count(key, fx.EPS, dev)
    assert (count[517:] == 1).all()            # (an fp32 d2 counts 2)
    check_knn(key, 2, dev)
    labels, core, num = check_dbscan(key, fx.EPS, 2, dev)
    assert not core[517:].any() and (labels[517:] == -1).all()


@pytest.mark.parametrize("offset", [100.0, 4096.0])
def test_radius_is_inclusive(offset, dev):
    key = ("exact", offset)
    P = fx.cloud(key)
    r = fx.EXACT_RADIUS
    assert ref.d2_rows(P, len(P) - 2, len(P) - 1)[0, -1] == np.float64(r) * np.float64(r)   # the product, on the CPU
    count = check_count(key, r, dev)
    assert count[-2:].tolist() == [2, 2]
    labels, core, num = check_dbscan(key, r, 2, dev)
    assert core[-2:].all() and labels[-1] == labels[-2] >= 0


# ---- lattice ----

def test_lattice(dev):
    key = ("lattice",)
    count = check_count(key, np.sqrt(2.0), dev).reshape(16, 16, 16)
    assert (count[1:-1, 1:-1, 1:-1] == 19).all()
    check_knn(key, 20, dev)                            # 6 ties at d2 = 1, 12 at d2 = 2: the order is by index
    check_knn(key, 32, dev)
    # corners (7 neighbours) and edges (10) are border points tied between core neighbours; faces and the interior are core
    labels, core, num = check_dbscan(key, np.sqrt(2.0), 14, dev)
    assert num == 1 and not core.reshape(16, 16, 16)[0, 0, 0] and (labels >= 0).all()
    check_dbscan(key, 1.0, 7, dev)                      # only the interior is core; a corner has no core neighbour: noise


# ---- degenerate clouds ----

@pytest.mark.parametrize("name", fx.DEGENERATE)
def test_degenerate(name, dev):
    key = ("degenerate", name)
    r = fx.DEGENERATE_RADIUS[name]
    count = check_count(key, r, dev)
    if name == "identical":
        assert (count == 300).all()
    for k in (1, 20, 32):
        check_knn(key, k, dev)
    check_dbscan(key, r, 5, dev)


def test_radius_above_and_below_every_distance(dev):
    key = ("degenerate", "uniform")
    P = fx.cloud(key)
    assert (check_count(key, 10.0, dev) == len(P)).all()
    nearest = np.sqrt(min(float(np.where(ref.d2_rows(P, lo, hi) > 0.0, ref.d2_rows(P, lo, hi), np.inf).min()) for lo, hi in ref._chunks(len(P))))
    assert (check_count(key, 0.5 * nearest, dev) == 1).all()
    check_dbscan(key, 10.0, len(P), dev)               # one cluster of everything, every count n
    check_dbscan(key, 0.5 * nearest, 2, dev)           # nothing but noise


# ---- DBSCAN ----

def test_dbscan_chain(dev):
    P, eps, mp = fx.chain()
    labels, core, num = check_dbscan(("chain",), eps, mp, dev)
    assert num == 1 and core.all() and (labels == 0).all()
    labels, core, num = check_dbscan(("shuffled", ("chain",), 3), eps, mp, dev)
    assert num == 1


def test_dbscan_bridge_point_does_not_join(dev):
    P, eps, mp = fx.bridge()
    labels, core, num = check_dbscan(("bridge",), eps, mp, dev)
    assert num == 2 and not core[-1] and set(labels[:27]) == {0} and set(labels[27:54]) == {1} and labels[-1] in (0, 1)


@pytest.mark.parametrize("order", ["ab", "ba"])
def test_dbscan_equidistant_border_goes_to_the_lower_core_index(order, dev):
    P, eps, mp = fx.tie(order)
    labels, core, num = check_dbscan(("tie", order), eps, mp, dev)
    assert num == 2 and not core[-1] and labels[-1] == 0      # the cube listed first holds the lower core index


def test_dbscan_min_points_edges(dev):
    key = ("blobs", 100.0)
    labels, core, num = check_dbscan(key, fx.EPS, 1, dev)      # every point is core
    assert core.all() and (labels >= 0).all()
    labels, core, num = check_dbscan(key, fx.EPS, 518, dev)    # min_points > n: every point is noise
    assert num == 0 and not core.any() and (labels == -1).all()


@pytest.mark.parametrize("seed", [1, 2])
def test_dbscan_numbering_of_a_shuffled_input(seed, dev):
    key = ("shuffled", ("blobs", 100.0), seed)
    labels, core, num = check_dbscan(key, fx.EPS, fx.MIN_POINTS, dev)
    firsts = [int(np.nonzero(core & (labels == c))[0][0]) for c in range(num)]
    assert firsts == sorted(firsts)
    # the same partition as the unshuffled input's, renumbered
    base = fx.ref_dbscan(("blobs", 100.0), fx.EPS, fx.MIN_POINTS)[2][fx.permutation(key)]
    assert len(set(zip(base.tolist(), labels.tolist()))) == num + 1


def test_public_dbscan_and_keep_largest(dev):
    from scorp_amd import cloud
    P = fx.blobs()
    count_ref, core_ref, labels_ref, num_ref = fx.ref_dbscan(("blobs", 100.0), fx.EPS, fx.MIN_POINTS)
    labels, core = cloud.cluster_dbscan(P, fx.EPS, fx.MIN_POINTS, return_core=True)
    assert labels.dtype == torch.int32 and core.dtype == torch.bool and labels.device.type == "cuda"
    np.testing.assert_array_equal(_np(labels), labels_ref)
    np.testing.assert_array_equal(_np(core), core_ref)
    assert torch.equal(cloud.cluster_dbscan(P, fx.EPS, fx.MIN_POINTS), labels)
    sizes = np.bincount(labels_ref[labels_ref >= 0])
    np.testing.assert_array_equal(_np(cloud.keep_largest_clusters(labels)), labels_ref == int(np.argmax(sizes)))


# ---- determinism ----

def test_two_calls_give_equal_bits_and_a_permutation_permutes(dev):
    from scorp_amd import cloud
    key = ("sized", 4099)
    P, radius = fx.sized(4099)
    a = cloud.knn_mean_distance(P, 20, return_neighbors=True)
    b = cloud.knn_mean_distance(P, 20, return_neighbors=True)
    assert torch.equal(a[0].view(torch.int64), b[0].view(torch.int64)) and torch.equal(a[1], b[1])
    la, lb = cloud.cluster_dbscan(P, radius, fx.SIZED_MIN_POINTS), cloud.cluster_dbscan(P, radius, fx.SIZED_MIN_POINTS)
    assert torch.equal(la, lb)
    ca = cloud.radius_neighbor_count(P, radius)
    perm = np.random.default_rng(9).permutation(len(P))
    pm = cloud.knn_mean_distance(P[perm], 20)
    assert torch.equal(pm.view(torch.int64), a[0][torch.from_numpy(perm).to(dev)].view(torch.int64))
    assert torch.equal(cloud.radius_neighbor_count(P[perm], radius), ca[torch.from_numpy(perm).to(dev)])


# ---- outlier removal ----

@pytest.mark.parametrize("key, k, ratio", [(("blobs", 100.0), 20, 2.0), (("blobs", 4096.0), 20, 2.0), (("degenerate", "dense_cell"), 8, 1.0)])
def test_remove_statistical_outlier(key, k, ratio, dev):
    from scorp_amd import cloud
    P = fx.cloud(key)
    ind_ref, thr, margin = ref.statistical_keep(fx.ref_knn(key, k)[0], ratio)
    assert margin > 1e-9
    kept, ind = cloud.remove_statistical_outlier(P, k, ratio)
    assert ind.dtype == torch.int64 and kept.device.type == "cuda"
    np.testing.assert_array_equal(_np(ind), ind_ref)
    np.testing.assert_array_equal(_np(kept), P[ind_ref])


@pytest.mark.parametrize("key, nb, radius", [(("blobs", 100.0), 8, fx.EPS), (("exact", 4096.0), 1, fx.EXACT_RADIUS), (("lattice",), 18, np.sqrt(2.0))])
def test_remove_radius_outlier(key, nb, radius, dev):
    from scorp_amd import cloud
    P = fx.cloud(key)
    ind_ref = np.nonzero(fx.ref_count(key, radius) > nb)[0]
    kept, ind = cloud.remove_radius_outlier(torch.from_numpy(P.copy()), nb, radius)
    assert ind.dtype == torch.int64
    np.testing.assert_array_equal(_np(ind), ind_ref)
    np.testing.assert_array_equal(_np(kept), P[ind_ref])


# ---- voxel grid ----

@pytest.mark.parametrize("name", ["blobs", "faces"])
def test_voxel_down_sample(name, dev):
    from scorp_amd import cloud
    from tests.mesh_simplify_reference import ulp_error
    P, col, h = fx.voxel_cloud(name)
    cell_ref, pos_ref, col_ref, count_ref = ref.voxel_grid(P, h, col)
    pos, colours, inverse = cloud.voxel_down_sample(P, h, colors=col, return_inverse=True)
    assert inverse.dtype == torch.int64 and pos.dtype == torch.float32
    np.testing.assert_array_equal(_np(inverse), cell_ref)                                   # membership and numbering
    np.testing.assert_array_equal(np.bincount(_np(inverse), minlength=len(count_ref)), count_ref)
    assert pos.shape == pos_ref.shape and colours.shape == col_ref.shape
    print(f"voxel {name}: {len(count_ref)} cells, position error {ulp_error(_np(pos), pos_ref):.3g} ulp, colour {ulp_error(_np(colours), col_ref):.3g} ulp")
    assert ulp_error(_np(pos), pos_ref) <= 1.0 and ulp_error(_np(colours), col_ref) <= 1.0
    only = cloud.voxel_down_sample(P, h)
    assert isinstance(only, torch.Tensor) and ulp_error(_np(only), pos_ref) <= 1.0
    pos2, inv2 = cloud.voxel_down_sample(P, h, return_inverse=True)
    assert torch.equal(inv2, inverse)
    with pytest.raises(ValueError, match="2\\^21 cells"):
        cloud.voxel_down_sample(P, 1e-8)


# ---- Gaussian models ----

@pytest.mark.parametrize("kind", ["3d", "2d"])
@pytest.mark.parametrize("method", ["dbscan", "statistical", "radius"])
def test_clean_gaussians_drops_the_planted_floaters(kind, method, dev, tmp_path):
    import math
    from scorp_amd import cloud
    from scorp_amd.gaussian_model import GaussianModel
    from scorp_amd.renderer2d import GaussianModel2D
    from scorp_amd.segment import apply_mask3d
    from scorp_amd.synthetic import make_gaussians
    N, planted = 1500, np.array([7, 400, 1499])
    raw = make_gaussians(N, 1, 3, log_scale_mean=math.log(0.02), scale_dims=3 if kind == "3d" else 2)
    rng = np.random.default_rng(21)
    raw["xyz"] = rng.uniform(-0.5, 0.5, (N, 3)).astype(np.float32)          # an object of side 1: spacing about 0.09
    raw["xyz"][planted] = np.array([[3.0, 0.0, 0.0], [0.0, -4.0, 1.0], [2.0, 2.0, 2.0]], np.float32)
    g = (GaussianModel if kind == "3d" else GaussianModel2D).from_raw(raw, 1, device=dev)
    g.active_sh_degree = 1
    kw = {"dbscan": dict(eps=0.2, min_points=5), "statistical": dict(nb_neighbors=10, std_ratio=3.0),
          "radius": dict(nb_points=3, radius=0.2)}[method]
    mask = cloud.clean_gaussians(g, method=method, **kw)
    assert mask.dtype == torch.bool and mask.shape == (N,) and mask.device.type == "cuda"
    expected = np.ones(N, bool)
    expected[planted] = False
    np.testing.assert_array_equal(_np(mask), expected)
    clone = apply_mask3d(g, mask, str(tmp_path / "clean.ply"), return_clone_gs=True)
    assert clone.get_xyz.shape[0] == N - len(planted)
    assert float(clone.get_xyz.detach().abs().max()) <= 0.5
