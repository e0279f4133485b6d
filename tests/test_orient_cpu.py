"""The yardstick of the normal orientation (tests/orient_reference.py, rules O1 - O6 of include/scorp_gs.h) against scipy's
minimum spanning tree and against hand-made cases, the properties the fixtures of tests/orient_fixtures.py are built for,
what the rule achieves on the thick-walled cup where orientation away from the centroid cannot, and the checks of the
Python wrapper and of the C entry point that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from scorp_amd import global_registration as gr
from tests import orient_fixtures as fx
from tests import orient_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIE_FREE = ("sized_63", "sized_257", "chain", "one_sided")


@pytest.mark.parametrize("name", TIE_FREE + ("cup",))
def test_forest_weight_equals_scipy(name):
    """The forest is a minimum spanning forest: its total weight is scipy's, and on a case without tied weights - where the
    forest is unique whatever the order - its edges are scipy's.  (scipy drops explicit zeros, so every weight is shifted by
    1; a forest of t edges then weighs t more.  The cup's PCA normals repeat, so its weights tie: total weight only.)"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import minimum_spanning_tree
    _, N, nb, _ = fx.cases()[name]
    tree, tdot, e, w = ref.forest(N, nb)
    assert (len(np.unique(w)) == len(w)) == (name in TIE_FREE)
    n = len(N)
    mst = minimum_spanning_tree(coo_matrix((w + 1.0, (e[:, 0], e[:, 1])), shape=(n, n)).tocsr())
    assert mst.nnz == len(tree)
    ours = float(np.sort(1.0 - np.abs(tdot)).sum())
    assert abs((mst.sum() - mst.nnz) - ours) <= 1e-9 * max(1.0, abs(ours))
    if name in TIE_FREE:
        got = {tuple(sorted(int(v) for v in p)) for p in zip(*mst.nonzero())}
        assert got == {tuple(p) for p in tree.tolist()}


@pytest.mark.parametrize("name", sorted(fx.cases()))
def test_forest_is_a_forest(name):
    """n - components edges, no cycle (a union-find over the tree never meets a joined pair), every edge an edge of the
    graph, labels the smallest member, rel(m) = 0, and along every tree edge the O4 signs agree with the dot."""
    P, N, nb, _ = fx.cases()[name]
    r = fx.reference(name)
    n = len(P)
    assert len(r["tree"]) == n - r["n_components"]
    all_edges = {tuple(p) for p in ref.edges(nb, n).tolist()}
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for a, b in r["tree"].tolist():
        assert (a, b) in all_edges and a < b
        ra, rb = find(a), find(b)
        assert ra != rb
        parent[ra] = rb
        assert (r["rel"][a] != r["rel"][b]) == (ref.dot(N, a, b) < 0.0)
    roots = np.array([find(x) for x in range(n)])
    for m in np.unique(r["label"]):
        members = np.nonzero(r["label"] == m)[0]
        assert members.min() == m and not r["rel"][m] and len(np.unique(roots[members])) == 1
    assert len(np.unique(roots)) == r["n_components"]
    flipped = np.array(r["normals"]).view(np.uint32) != np.ascontiguousarray(N).view(np.uint32)
    assert (flipped.all(1) == r["flip"]).all() and (flipped.any(1) == r["flip"]).all()


def test_hand_made_chain():
    """0 - 1 - 2 - 3 with dots +, -, 0: signs (0, 0, 1, 1), a dot of exactly 0 is no flip; `first` keeps point 0, the votes
    about a centre far below flip the whole component back."""
    P = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0]], np.float32)
    N = np.array([[0, 0, 1], [0, 0, 1], [0, 0, -1], [0, 1, 0]], np.float32)
    nb = np.array([[1], [2], [3], [-1]], np.int32)
    r = ref.orient(P, N, nb, component_sign="first")
    assert r["rel"].tolist() == [False, False, True, True] and r["flip"].tolist() == [False, False, True, True]
    assert r["tree"].tolist() == [[0, 1], [1, 2], [2, 3]] and r["n_components"] == 1
    assert r["normals"].tolist() == [[0, 0, 1], [0, 0, 1], [0, 0, 1], [0, -1, 0]]
    up = ref.orient(P, N, nb, center=[1.5, 0, -5.0])
    assert up["votes"] == {0: 3} and up["flip"].tolist() == r["flip"].tolist()
    down = ref.orient(P, N, nb, center=[1.5, 0, 5.0])
    assert down["votes"] == {0: -3} and down["flip"].tolist() == [True, True, False, False]


def test_order_decides_between_equal_weights():
    """A triangle of equal normals: all three weights are 0, (lo, hi) decides - (0, 1) and (0, 2) are taken, (1, 2) is not."""
    N = np.tile(np.array([0, 0, 1], np.float32), (3, 1))
    r = ref.orient(np.eye(3, dtype=np.float32), N, np.array([[1, 2], [2, 0], [0, 1]], np.int32), component_sign="first")
    assert r["tree"].tolist() == [[0, 1], [0, 2]]


def test_mean_center_rule():
    P = np.random.default_rng(2).normal(0, 1, (40000, 3)).astype(np.float32)
    c = ref.mean_center(P)
    assert np.abs(c - P.astype(np.float64).mean(0)).max() < 1e-12
    g = 5
    s = 0.0
    for v in P[g::ref.CENTER_LANES, 0].astype(np.float64).tolist():
        s = s + v
    padded = np.zeros((3 * ref.CENTER_LANES, 3))
    padded[:40000] = P
    assert np.cumsum(padded.reshape(3, ref.CENTER_LANES, 3), axis=0)[-1][g, 0] == s


def test_fixtures_hold_the_cases_they_are_for():
    c = fx.cases()
    for n in (1, 2, 3):
        assert (c[f"sized_{n}"][2][:, n:] == -1).all() and c[f"sized_{n}"][2].shape[1] == fx.SIZED_K > n
    _, N, nb, _ = c["plane_of_ties"]
    _, _, w = ref.sorted_edges(N, nb)
    assert len(N) == 576 and nb.shape[1] == 8 and (w == 0.0).all() and (N[:, 2] < 0).sum() == 288
    assert fx.reference("plane_of_ties")["n_components"] == 1
    assert len(c["chain"][0]) == 700 and c["chain"][2].shape[1] == 2 and fx.reference("chain")["n_components"] == 1
    _, N, nb, _ = c["one_sided"]
    one = fx.one_sided_vertices(N, nb)
    listed = set(nb[nb >= 0].tolist())
    assert any(v < 40 for v in one), "no cluster point's smallest edge is listed from the far side only"
    assert not listed & set(range(40, 50)) and fx.reference("one_sided")["n_components"] == 1
    P, N, nb, center = c["two_components"]
    r = fx.reference("two_components")
    assert (nb[7] == -1).all() and (nb == 7).any() and r["label"][7] == 0
    assert r["n_components"] == 3 and sorted(np.unique(r["label"]).tolist()) == [0, 60, 120]
    assert r["votes"][0] > 0 > r["votes"][60] and r["votes"][120] == 0
    assert r["flip"][list(fx.TIE_PAIR)].tolist() == [False, True]            # the tie leaves O4's signs
    _, N, nb, _ = c["perpendicular"]
    e, d, w = ref.sorted_edges(N, nb)
    assert (d == 0.0).sum() >= 2 and (w < 0.0).any() and not N[4].any() and (nb[9] == 9).any()
    out = fx.reference("perpendicular", "first")["normals"]
    zero_flipped = fx.reference("perpendicular", "first")["flip"][4]
    assert np.signbit(out[4]).all() == bool(zero_flipped)


def test_cup_is_oriented_where_away_from_the_centroid_is_not():
    """The thick-walled cup, PCA normals of 12 neighbours done in numpy: propagation signs at least 99 % of the points
    outward (measured: 100 %), away-from-centroid fewer than 75 % (measured: 67.6 %; the inner wall and inner bottom)."""
    P, truth = fx.cup()
    N, nb = fx.cup_pca()
    good = fx.outward_fraction(fx.reference("cup")["normals"], truth)
    away = fx.outward_fraction(ref.away_from(P, N), truth)
    print(f"cup: tangent-plane {good:.4f} outward, away-from-centroid {away:.4f}")
    assert good >= 0.99
    assert away < 0.75


def test_wrapper_raises_value_errors_without_a_gpu():
    P, N, nb, _ = (np.array(a) if a is not None else None for a in fx.cases()["sized_65"])
    bad = P.copy()
    bad[3, 1] = np.nan
    orient = gr.orient_normals_consistent_tangent_plane
    with pytest.raises(ValueError, match="component_sign"):
        orient(P, N, component_sign="last")
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        orient(P[:, :2], N[:, :2])
    with pytest.raises(ValueError, match=r"\[n, 3\]"):
        orient(P[:0], N[:0])
    with pytest.raises(ValueError, match="normals"):
        orient(P, N[:10])
    for k in (0, 65, -1, 2.5):
        with pytest.raises(ValueError, match="k must"):
            orient(P, N, k=k)
    with pytest.raises(ValueError, match="neighbors"):
        orient(P, N, neighbors=nb[:10])
    with pytest.raises(ValueError, match="neighbors"):
        orient(P, N, neighbors=np.zeros((65, 65), np.int32))
    with pytest.raises(ValueError, match="neighbors"):
        orient(P, N, neighbors=np.zeros((65, 0), np.int32))
    with pytest.raises(ValueError, match="int32"):
        orient(P, N, neighbors=nb.astype(np.int64))
    with pytest.raises(ValueError, match="int32"):
        orient(P, N, neighbors=torch.from_numpy(nb).to(torch.int64))
    with pytest.raises(ValueError, match="center"):
        orient(P, N, center=[0.0, 1.0])
    with pytest.raises(ValueError, match="center"):
        orient(P, N, center=[0.0, np.inf, 0.0])
    with pytest.raises(ValueError, match="NaN"):
        orient(bad, N)
    with pytest.raises(ValueError, match="NaN"):
        orient(P, bad)
    with pytest.raises(ValueError, match="orientation"):
        gr.get_FPFH_fitting_transformation(P, P, 0.1, orientation="tangent")


def test_exports_and_host_checks():
    """The two names are in the header and bound in _C, the workspace size is host arithmetic, and the argument checks
    answer SCORP_ERR_INVALID with a message before any HIP call (the dummy pointers are never dereferenced)."""
    from scorp_amd import _C
    header = open(os.path.join(ROOT, "include", "scorp_gs.h")).read()
    for name in ("scorp_cloud_orient_workspace_bytes", "scorp_cloud_orient_normals"):
        assert name in _C.EXPORTS and re.search(rf"\b{name}\(", header)
    for rule in ("O1", "O2", "O3", "O4", "O5", "O6"):
        assert re.search(rf"\* {rule} ", header)
    assert (_C.ORIENT_MAJORITY_AWAY, _C.ORIENT_FIRST) == (0, 1)
    assert "#define SCORP_ORIENT_MAJORITY_AWAY 0" in header and "#define SCORP_ORIENT_FIRST 1" in header
    L = _C.lib()
    size = L.scorp_cloud_orient_workspace_bytes(1000, 12)
    assert size % 256 == 0 and size >= 1000 * 32 and L.scorp_cloud_orient_workspace_bytes(2000, 12) > size
    dummy = 0x10000
    good = dict(points=dummy, normals=dummy, nb=dummy, n=1000, k=12, center=None, sign=0, out=dummy, counts=dummy, ws=dummy, ws_bytes=size)

    def call(**kw):
        a = {**good, **kw}
        return L.scorp_cloud_orient_normals(a["points"], a["normals"], a["nb"], a["n"], a["k"], a["center"], a["sign"], a["out"], None,
                                            None, None, a["counts"], a["ws"], a["ws_bytes"], None)

    nan3 = (ctypes.c_double * 3)(0.0, float("nan"), 0.0)
    for kw in (dict(n=0), dict(n=-2), dict(n=(1 << 30) + 1), dict(k=0), dict(k=65), dict(points=None), dict(normals=None), dict(nb=None),
               dict(out=None), dict(counts=None), dict(ws=None), dict(ws_bytes=size - 1), dict(ws=dummy + 8), dict(sign=2), dict(sign=-1),
               dict(center=nan3)):
        assert call(**kw) == _C.ERR_INVALID, kw
        assert L.scorp_last_error()
