"""Normal estimation on the GPU (scorp_estimate_normals, scorp_amd.icp.estimate_normals) against the float64 brute force of
tests/icp_plane_reference.py, on the fixtures of tests/icp_plane_fixtures.py.

Neighbours: where the k-th and (k + 1)-th neighbour distances differ by more than 2 slack (slack = 2^-20 of the largest
|coordinate - bounding-box centre|, the fp32 search's rounding as in tests/test_icp_search_gpu.py) the neighbour SET
equals the brute force's; everywhere, the list is sorted by the search's own (d^2, index) and holds distinct points, the
point itself first.  On the integer lattice every d^2 is exact in fp32, so the whole ordered list is asserted.

Normals: |n x n_ref| <= 1e-9 + 2^-23 where the eigen-gap l_1 - l_0 >= 1e-3 l_2 holds too.  The float64 covariance of at
most 32 terms and the Jacobi sweeps perturb the matrix by about 1e-14 l_2; over a gap of at least 1e-3 l_2 that turns the
eigenvector by about 1e-11, taken with a 100x margin; 2^-23 is the rounding of the unit vector's components to fp32.  At
most 5 % of a fixture's points may lack the margins (tests/test_icp_plane_cpu.py holds every fixture to that).

Measured in one MI355X run: every neighbour set equal to the brute force's in every fixture, also at the 0.2 % of the
40 000-point rows without the margin (0 % elsewhere); largest |n x n_ref| under the gap 2.0e-8 - 4.5e-8 (bound 1.2e-7)."""
import numpy as np
import pytest
import torch

from tests import icp_plane_fixtures as pfx
from tests import icp_plane_reference as pref
from tests import icp_probe_fixtures as fx

pytestmark = pytest.mark.gpu

NORMAL_BOUND = 1e-9 + 2.0 ** -23


@pytest.fixture(scope="module")
def icp():
    from scorp_amd import icp as m
    return m


def _run(icp, pts, knn):
    n, nb = icp.estimate_normals(np.array(pts), knn=knn, return_neighbors=True)
    assert n.is_cuda and n.dtype == torch.float32 and nb.dtype == torch.int32 and tuple(nb.shape) == (len(pts), knn)
    return n.cpu().numpy(), nb.cpu().numpy()


@pytest.mark.parametrize("name", sorted(pfx.NORMALS))
def test_neighbours_and_normals_match_brute_force(icp, name):
    f = pfx.normals_fixture(name)
    pts, knn, rows = f["points"], f["knn"], f["rows"]
    k = min(knn, len(pts))
    assert np.mean(~f["margin"]) <= pfx.MARGIN_CAP and np.mean(~f["gap"]) <= pfx.MARGIN_CAP     # the fixture property, again
    nrm, nb = _run(icp, pts, knn)
    assert (nb[:, k:] == -1).all() and (nb[:, :k] >= 0).all() and (nb[:, :k] < len(pts)).all()
    assert (nb[:, 0] == np.arange(len(pts))).all()                                     # d^2 = 0: itself
    assert (np.sort(nb[:, :k], axis=1)[:, 1:] != np.sort(nb[:, :k], axis=1)[:, :-1]).all()     # distinct
    got = nb[rows, :k]
    same = (np.sort(got, axis=1) == np.sort(f["idx"], axis=1)).all(axis=1)
    assert same[f["margin"]].all(), f"{name}: {int((~same & f['margin']).sum())} neighbour sets differ where the margin holds"
    np.testing.assert_allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-6)
    assert (np.take_along_axis(nrm, np.abs(nrm).argmax(axis=1)[:, None], axis=1) > 0).all()      # the sign rule
    cross = np.linalg.norm(np.cross(nrm[rows].astype(np.float64), f["normals"]), axis=1)
    worst = float(cross[f["gap"]].max())
    print(f"{name}: n {len(pts)}, k {k}, {np.mean(~f['margin']):.4f} without the neighbour margin, {int((~same).sum())} sets differ "
          f"there, largest |n x n_ref| under the gap {worst:.3g} (bound {NORMAL_BOUND:.3g})")
    assert worst <= NORMAL_BOUND
    # where the largest component is not in doubt, the sign is the yardstick's too
    clear = f["gap"] & (np.sort(np.abs(f["normals"]), axis=1)[:, 2] - np.sort(np.abs(f["normals"]), axis=1)[:, 1] > 1e-6)
    assert (np.abs(nrm[rows][clear] - f["normals"][clear]).max(axis=1) <= 1e-6).all()


@pytest.mark.parametrize("shuffle", [0, 1])
def test_ties_go_to_the_lowest_indices(icp, shuffle):
    tgt, _, _, _, _ = fx.ties_fixture(shuffle)
    for knn in (7, 30):
        _, nb = _run(icp, tgt, knn)
        idx, _, _ = pref.knn_brute(tgt, knn)
        assert np.array_equal(nb, idx), f"knn {knn}: {int((nb != idx).any(axis=1).sum())} lists differ"


def test_special_clouds(icp):
    rng = np.random.default_rng(0)
    plane = np.column_stack([rng.random((300, 2)), np.full(300, 0.25)]).astype(np.float32)
    nrm, _ = _run(icp, plane, 10)
    np.testing.assert_allclose(nrm, np.tile([0.0, 0.0, 1.0], (300, 1)), atol=1e-6)          # +1: the sign rule
    tilted = np.column_stack([plane[:, 0], plane[:, 1], -0.5 * plane[:, 0]]).astype(np.float32)   # z = -x / 2: normal (1, 0, 2)
    nrm, _ = _run(icp, tilted, 10)
    np.testing.assert_allclose(nrm, np.tile(np.array([1.0, 0.0, 2.0]) / np.sqrt(5.0), (300, 1)), atol=1e-5)
    for n in (1, 2):
        nrm, nb = _run(icp, plane[:n], 30)
        assert np.array_equal(nrm, np.tile(np.float32([0, 0, 1]), (n, 1)))
        assert (nb[:, n:] == -1).all() and np.array_equal(np.sort(nb[:, :n], axis=1), np.tile(np.arange(n), (n, 1)))
    same = np.repeat(np.float32([[0.3, -0.2, 0.5]]), 64, axis=0)
    nrm, nb = _run(icp, same, 30)
    assert np.isfinite(nrm).all()
    np.testing.assert_allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-6)
    assert np.array_equal(nb, np.tile(np.arange(30), (64, 1)))          # every d^2 is 0: the lowest indices


def test_same_bits_on_two_calls_and_input_unmodified(icp):
    pts = pfx.normals_fixture("u257_k30")["points"]
    P = torch.tensor(np.array(pts), device="cuda:0")
    P0 = P.clone()
    a, na = icp.estimate_normals(P, knn=30, return_neighbors=True)
    b, nb = icp.estimate_normals(P, knn=30, return_neighbors=True)
    assert torch.equal(a, b) and torch.equal(na, nb) and torch.equal(P, P0)
    assert torch.equal(icp.estimate_normals(P, knn=30), a)              # without the neighbour output


def test_library_rejects_invalid_arguments(icp):
    from scorp_amd import _C
    L = _C.lib()
    P = torch.zeros(8, 3, device="cuda:0")
    out = torch.zeros(8, 3, device="cuda:0")
    ws = torch.zeros(int(L.scorp_estimate_normals_workspace_bytes(8)) + 256, dtype=torch.uint8, device="cuda:0")
    w = (ws.data_ptr() + 255) // 256 * 256
    nbytes = ws.numel() - 256
    args = lambda **k: [k.get("p", P.data_ptr()), k.get("n", 8), k.get("knn", 30), k.get("o", out.data_ptr()), None,
                        k.get("w", w), k.get("b", nbytes), None]
    assert L.scorp_estimate_normals(*args()) == 0
    for bad in (dict(knn=2), dict(knn=33), dict(n=0), dict(p=None), dict(o=None), dict(w=None), dict(w=w + 8), dict(b=nbytes // 2)):
        assert L.scorp_estimate_normals(*args(**bad)) == _C.ERR_INVALID, bad
    torch.cuda.synchronize()
