"""Consistent orientation of normals on the GPU (csrc/cloud_orient.hip through scorp_amd/global_registration.py) against
the float64 yardstick of tests/orient_reference.py: flips, labels, component count and the sorted forest are asserted EQUAL,
the normals BIT FOR BIT, on every fixture of tests/orient_fixtures.py, through the C ABI and through the wrapper."""
import ctypes

import numpy as np
import pytest
import torch

from scorp_amd import global_registration as gr
from tests import fpfh_fixtures as ffx
from tests import fpfh_reference as fref
from tests import orient_fixtures as fx
from tests import orient_reference as ref

pytestmark = pytest.mark.gpu

SIGNS = {"majority_away": 0, "first": 1}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need a GPU"
    from scorp_amd import _C
    _C.lib()
    return torch.device("cuda:0")


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _sorted_tree(tree):
    t = tree[tree[:, 0] >= 0].astype(np.int64)
    assert (tree[tree[:, 0] < 0] == -1).all()
    return t[np.lexsort((t[:, 1], t[:, 0]))]


def orient_abi(P, N, nb, center, component_sign, dev, optional=True, fill=None):
    """scorp_cloud_orient_normals through the C ABI: (normals, flip, label, sorted tree, counts) as numpy arrays, flip / label
    / tree None when `optional` is off (NULL pointers)."""
    from scorp_amd import _C
    P, N, nb = (torch.from_numpy(np.array(a)).to(dev) for a in (P, N, nb))
    n, k = nb.shape
    out = torch.full((n, 3), -7.0, dtype=torch.float32, device=dev)
    flip = torch.full((n,), 7, dtype=torch.uint8, device=dev) if optional else None
    label = torch.full((n,), -7, dtype=torch.int32, device=dev) if optional else None
    tree = torch.full((n, 2), -7, dtype=torch.int32, device=dev) if optional else None
    counts = torch.full((2,), -7, dtype=torch.int32, device=dev)
    size = _C.lib().scorp_cloud_orient_workspace_bytes(n, k)
    workspace = torch.empty(size, dtype=torch.uint8, device=dev)
    if fill is not None:
        workspace.fill_(fill)
    c = None if center is None else (ctypes.c_double * 3)(*np.asarray(center, np.float64).tolist())
    _C.call("scorp_cloud_orient_normals", P, N, nb, n, k, c, SIGNS[component_sign], out, flip, label, tree, counts, workspace, size)
    torch.cuda.synchronize()
    return (_np(out), None if flip is None else _np(flip), None if label is None else _np(label),
            None if tree is None else _sorted_tree(_np(tree)), _np(counts))


def check_against(r, normals, flip, label, tree, n_components):
    np.testing.assert_array_equal(np.asarray(flip).astype(bool), r["flip"])
    np.testing.assert_array_equal(label, r["label"])
    assert n_components == r["n_components"]
    np.testing.assert_array_equal(tree, r["tree"])
    assert np.array_equal(_bits(normals), _bits(r["normals"]))


@pytest.mark.parametrize("component_sign", ["majority_away", "first"])
@pytest.mark.parametrize("name", sorted(fx.cases()))
def test_orient_equals_the_reference_through_the_c_abi(name, component_sign, dev):
    P, N, nb, center = fx.cases()[name]
    r = fx.reference(name, component_sign)
    out, flip, label, tree, counts = orient_abi(P, N, nb, center, component_sign, dev)
    assert out.dtype == np.float32 and out.shape == (len(P), 3) and flip.dtype == np.uint8 and label.dtype == np.int32
    assert set(np.unique(flip).tolist()) <= {0, 1}
    check_against(r, out, flip, label, tree, int(counts[0]))
    assert int(counts[1]) == len(r["tree"]) == len(P) - r["n_components"]


@pytest.mark.parametrize("name", sorted(fx.cases()))
def test_orient_equals_the_reference_through_the_wrapper(name, dev):
    P, N, nb, center = fx.cases()[name]
    r = fx.reference(name)
    out, info = gr.orient_normals_consistent_tangent_plane(np.array(P), torch.from_numpy(np.array(N)).to(dev), neighbors=np.array(nb),
                                                           center=center, return_info=True)
    assert out.is_cuda and out.dtype == torch.float32 and info["flip"].dtype == torch.bool and info["label"].dtype == torch.int32
    assert info["tree"].dtype == torch.int64 and info["tree"].shape == (len(r["tree"]), 2)
    check_against(r, _np(out), _np(info["flip"]), _np(info["label"]), info["tree"].numpy(), info["n_components"])
    only = gr.orient_normals_consistent_tangent_plane(torch.from_numpy(np.array(P)), np.array(N, np.float64),
                                                      neighbors=torch.from_numpy(np.array(nb)).to(dev), center=center)
    assert not only.is_cuda and only.dtype == torch.float64                   # the normals' own dtype and device
    assert np.array_equal(only.numpy(), np.array(r["normals"]).astype(np.float64))
    assert np.array_equal(np.signbit(only.numpy()), np.signbit(np.array(r["normals"])))


@pytest.mark.parametrize("name", ["sized_257", "plane_of_ties", "chain", "two_components"])
def test_orient_twice_the_same_bits_and_null_outputs(name, dev):
    """Two calls give the same bits whatever the workspace held before, and with the optional outputs NULL the normals and
    the counts are the same."""
    P, N, nb, center = fx.cases()[name]
    a = orient_abi(P, N, nb, center, "majority_away", dev, fill=0)
    b = orient_abi(P, N, nb, center, "majority_away", dev, fill=255)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    assert np.array_equal(_bits(a[0]), _bits(b[0]))
    c = orient_abi(P, N, nb, center, "majority_away", dev, optional=False, fill=255)
    assert c[1] is None and c[2] is None and c[3] is None
    assert np.array_equal(_bits(c[0]), _bits(a[0]))
    np.testing.assert_array_equal(c[4], a[4])


@pytest.mark.parametrize("name", ["two_components", "sized_65", "cup"])
def test_orient_center_given_against_default(name, dev):
    """The default centre is the fixed-order float64 mean of O5; a given centre is used as it is (two_components
    brings its own, about which its pair ties; the other two cases have none)."""
    P, N, nb, center = fx.cases()[name]
    r = fx.reference(name, default_center=True)
    out, flip, label, tree, counts = orient_abi(P, N, nb, None, "majority_away", dev)
    check_against(r, out, flip, label, tree, int(counts[0]))
    moved = np.array([0.3, -2.0, 0.7]) if center is None else np.asarray(center) + [0.3, -2.0, 0.7]
    want = ref.orient(P, N, nb, moved)
    got = orient_abi(P, N, nb, moved, "majority_away", dev)
    check_against(want, got[0], got[1], got[2], got[3], int(got[4][0]))
    again = orient_abi(P, N, nb, r["center"], "majority_away", dev)          # the default, handed in: the same result
    assert np.array_equal(_bits(again[0]), _bits(out))
    w = gr.orient_normals_consistent_tangent_plane(np.array(P), np.array(N), neighbors=np.array(nb))
    assert np.array_equal(_bits(w.numpy()), _bits(r["normals"]))


@pytest.mark.parametrize("name", ["sized_257", "plane_of_ties", "one_sided", "two_components"])
def test_orient_permuted_input_equals_the_reference_on_it(name, dev):
    """Relabelling the points changes O3's tie-break and the component's smallest index, so the result is held to the
    reference run on the permuted input (where no weights tie the forest is the same set of edges, relabelled)."""
    P, N, nb, center = fx.cases()[name]
    n = len(P)
    perm = np.random.default_rng(9).permutation(n)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    nb2 = np.where(nb[perm] >= 0, inv[np.maximum(nb[perm], 0)], -1).astype(np.int32)
    want = ref.orient(P[perm], N[perm], nb2, center)
    got = orient_abi(P[perm], N[perm], nb2, center, "majority_away", dev)
    check_against(want, got[0], got[1], got[2], got[3], int(got[4][0]))
    if name == "sized_257":
        base = fx.reference(name)
        relabelled = np.sort(inv[base["tree"]], axis=1)
        np.testing.assert_array_equal(relabelled[np.lexsort((relabelled[:, 1], relabelled[:, 0]))], want["tree"])


def test_orient_default_list_and_the_lists_of_the_other_kernels(dev):
    """Without `neighbors` the list is the exact k + 1 nearest with the point itself; the lists of estimate_normals and of
    compute_fpfh_feature, and their first columns, are taken as they are.  Each result equals the reference on that list."""
    from scorp_amd import cloud, icp
    P, N, _, _ = fx.cases()["sized_257"]
    Pd, Nd = torch.from_numpy(np.array(P)).to(dev), torch.from_numpy(np.array(N)).to(dev)
    lists = {"default": None,
             "estimate_normals": icp.estimate_normals(Pd, knn=30, return_neighbors=True)[1],
             "fpfh": gr.compute_fpfh_feature(Pd, Nd, 0.3, 64, return_neighbors=True)[1]}
    lists["estimate_normals_12"] = lists["estimate_normals"][:, :12]
    lists["fpfh_5"] = lists["fpfh"][:, :5]
    for name, nb in lists.items():
        out, info = gr.orient_normals_consistent_tangent_plane(Pd, Nd, k=12, neighbors=nb, return_info=True)
        if nb is None:
            nb = cloud.knn_mean_distance(Pd, 13, return_neighbors=True)[1]
            np.testing.assert_array_equal(_np(nb), ref.knn(P, 13))
        want = ref.orient(P, N, _np(nb))
        print(f"list {name}: {tuple(nb.shape)}, {want['n_components']} components")
        check_against(want, _np(out), _np(info["flip"]), _np(info["label"]), info["tree"].numpy(), info["n_components"])
    with pytest.raises(ValueError, match=">= n"):
        gr.orient_normals_consistent_tangent_plane(Pd, Nd, neighbors=torch.full((257, 3), 257, dtype=torch.int32))


def test_cup_end_to_end_on_the_gpu(dev):
    """estimate_normals(knn=12) on the thick-walled cup, then orientation over its own list: at least 99 % of the normals
    point outward against the analytic truth, with orient_normals_away_from fewer than 75 % (both caps are the CPU check's
    conditions, tests/test_orient_cpu.py).  Measured on an MI355X: 100 % and 67.55 %."""
    from scorp_amd import icp
    P, truth = fx.cup()
    N, nb = icp.estimate_normals(np.array(P), knn=fx.CUP["knn"], return_neighbors=True)
    out, info = gr.orient_normals_consistent_tangent_plane(np.array(P), N, neighbors=nb, return_info=True)
    want = ref.orient(P, _np(N), _np(nb))
    check_against(want, _np(out), _np(info["flip"]), _np(info["label"]), info["tree"].numpy(), info["n_components"])
    good = fx.outward_fraction(_np(out), truth)
    away = fx.outward_fraction(_np(gr.orient_normals_away_from(torch.from_numpy(np.array(P)).to(dev), N)), truth)
    print(f"cup on the GPU: tangent-plane {good:.4f} outward in {info['n_components']} component(s), away-from-centroid {away:.4f}")
    assert good >= 0.99
    assert away < 0.75


def test_route_with_tangent_plane_orientation(dev):
    """get_FPFH_fitting_transformation(orientation="tangent_plane") on the fixture pair, held to the bounds of the existing
    route test (0.5 degrees, 0.5 % of the diagonal); the default orientation gives the bits of the route composed by hand
    from the calls it made before the option existed."""
    from scorp_amd import cloud, icp
    pair = ffx.registration_pair()
    orig, refined = np.array(pair["target"]), np.array(pair["source"])
    threshold = float(np.ptp(orig, axis=0).mean() * 0.16)
    T = gr.get_FPFH_fitting_transformation(orig, refined, threshold, orientation="tangent_plane")
    ang, dt = fref.pose_error(T, pair["truth"])
    default = gr.get_FPFH_fitting_transformation(orig, refined, threshold)
    dang, ddt = fref.pose_error(default, pair["truth"])
    print(f"route: tangent_plane {ang:.4f} deg, {dt:.2e}; away_from {dang:.4f} deg, {ddt:.2e}; diagonal {pair['diagonal']:.3f}")
    assert ang < 0.5 and dt < 0.005 * pair["diagonal"]
    voxel = gr.default_voxel_size(orig)
    down, feat = [], []
    for a in (refined, orig):
        Q = cloud.voxel_down_sample(a, voxel)
        M = gr.orient_normals_away_from(Q, icp.estimate_normals(Q, knn=min(30, max(3, Q.shape[0]))))
        down.append(Q)
        feat.append(gr.compute_fpfh_feature(Q, M, 5.0 * voxel, gr.MAX_NN))
    reg = gr.registration_ransac_based_on_feature_matching(down[0], down[1], feat[0], feat[1], 1.5 * voxel, seed=0)
    src = refined[icp.downsample_indices(len(orig), len(refined))]
    by_hand = icp.registration_icp(src, orig, threshold, reg.transformation, max_iteration=400).transformation[0]
    assert np.array_equal(default.view(np.uint64), np.ascontiguousarray(by_hand).view(np.uint64))
    explicit = gr.get_FPFH_fitting_transformation(orig, refined, threshold, orientation="away_from")
    assert np.array_equal(default.view(np.uint64), explicit.view(np.uint64))


def test_route_on_a_concave_object(dev):
    """A mug (tests/orient_fixtures.py: the thick-walled cup plus a block as a handle, 4600 points; 3200 of them jittered and
    moved by the 120-degree pose).  The float64 reference pipeline of tests/fpfh_reference.py (PCA normals of 12 neighbours,
    the orientation of tests/orient_reference.py, FPFH at radius 0.3, 4096 fixed triples at distance 0.08, no ICP;
    scripts/mug_reference_probe.py) recovers the pose with tangent-plane normals to 0.360 degrees and 6.4e-4 of the
    diagonal, inside the route test's bounds, so the GPU route is held to them: under 0.5 degrees and 0.5 % of the diagonal
    after its ICP.  With away-from-centroid normals the reference gave 0.366 degrees and 5.2e-4: that rule signs 71 % of the
    mug outward, but the same 71 % in both clouds, so the descriptors still match; what `away_from` gives on the GPU is printed
    beside the asserted figures."""
    pair = fx.mug_pair()
    orig, refined = np.array(pair["target"]), np.array(pair["source"])
    threshold = float(np.ptp(orig, axis=0).mean() * 0.16)
    got = {}
    for orientation in ("tangent_plane", "away_from"):
        T = gr.get_FPFH_fitting_transformation(orig, refined, threshold, orientation=orientation)
        got[orientation] = fref.pose_error(T, pair["truth"])
    print(f"mug route: tangent_plane {got['tangent_plane'][0]:.4f} deg, {got['tangent_plane'][1] / pair['diagonal']:.2e} of the diagonal; "
          f"away_from {got['away_from'][0]:.4f} deg, {got['away_from'][1] / pair['diagonal']:.2e}")
    ang, dt = got["tangent_plane"]
    assert ang < 0.5 and dt < 0.005 * pair["diagonal"]


def test_orient_invalid_arguments(dev):
    from scorp_amd import _C
    L = _C.lib()
    P, N, nb = (torch.from_numpy(np.array(a)).to(dev) for a in fx.cases()["sized_65"][:3])
    n, k = nb.shape
    out = torch.empty(n, 3, dtype=torch.float32, device=dev)
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    size = L.scorp_cloud_orient_workspace_bytes(n, k)
    ws = torch.empty(size + 256, dtype=torch.uint8, device=dev)
    base = (ws.data_ptr() + 255) // 256 * 256
    good = dict(points=P.data_ptr(), normals=N.data_ptr(), nb=nb.data_ptr(), n=n, k=k, center=None, sign=0, out=out.data_ptr(),
                counts=counts.data_ptr(), ws=base, ws_bytes=size)

    def call(**kw):
        a = {**good, **kw}
        return L.scorp_cloud_orient_normals(a["points"], a["normals"], a["nb"], a["n"], a["k"], a["center"], a["sign"], a["out"], None,
                                            None, None, a["counts"], a["ws"], a["ws_bytes"], None)

    assert call() == 0
    for kw in (dict(n=0), dict(n=-1), dict(n=(1 << 30) + 1), dict(k=0), dict(k=65), dict(points=None), dict(normals=None), dict(nb=None),
               dict(out=None), dict(counts=None), dict(ws=None), dict(ws_bytes=size - 1), dict(ws=base + 16), dict(sign=2),
               dict(center=(ctypes.c_double * 3)(0.0, float("inf"), 0.0))):
        assert call(**kw) == _C.ERR_INVALID, kw
        assert L.scorp_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(_np(out)), _bits(fx.reference("sized_65")["normals"]))
