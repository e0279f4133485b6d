"""Colour gradients on the GPU (scorp_color_gradients, scorp_amd.icp.estimate_color_gradients) against the float64
yardstick of tests/icp_color_reference.py, on the gradient fixtures of tests/icp_color_fixtures.py.

The neighbour lists come from estimate_normals on the GPU; where a row's neighbour SET equals the yardstick's (everywhere
the neighbour margin of tests/test_normals_gpu.py holds) the gradient is held, per row, to the larger of 10x the
yardstick's own sensitivity to the order of that row (measured by shuffling it) and one fp32 ulp of the row's largest
component (the store rounds to fp32): icp_color_fixtures.gradient_bound, measured on the yardstick alone.  Where the rule
says zero the result is exactly zero.  The measured values are printed; DESIGN.md 4.10 holds them.

Measured in one MI355X run: every neighbour set equal to the brute force's on every fixture; |d - yardstick| at most 0.5 of
the bound, which is the fp32 ulp everywhere (3.0e-8 - 1.2e-7; the yardstick's order sensitivity is at most 1.7e-14)."""
import numpy as np
import pytest
import torch

from tests import icp_color_fixtures as cfx
from tests import icp_plane_reference as pref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def icp():
    from scorp_amd import icp as m
    return m


def _run(icp, f):
    g = icp.estimate_color_gradients(np.array(f["points"]), np.array(f["intensity"]), normals=np.array(f["normals"]), knn=f["knn"])
    assert g.is_cuda and g.dtype == torch.float32 and tuple(g.shape) == (len(f["points"]), 3)
    return g.cpu().numpy()


@pytest.mark.parametrize("name", cfx.GRADIENTS)
def test_gradients_match_the_yardstick(icp, name):
    f = cfx.gradient_fixture(name)
    assert np.mean(~f["margin"]) <= cfx.MARGIN_CAP and pref.eig_ratios_clear(list(f["eigenvalues"]))     # the fixture property, again
    rows, knn, want = f["rows"], f["knn"], f["gradients"]
    got = _run(icp, f)[rows].astype(np.float64)
    _, nb = icp.estimate_normals(np.array(f["points"]), knn=knn, return_neighbors=True)
    same = (np.sort(nb.cpu().numpy()[rows], axis=1) == np.sort(f["neighbors"], axis=1)).all(axis=1)
    assert same[f["margin"]].all()
    bound = cfx.gradient_bound(want, f["sensitivity"])
    err = np.abs(got - want).max(axis=1)
    worst = int(np.argmax(np.where(same, err / bound, 0.0)))
    print(f"{name}: {len(rows)} rows, {int((~same).sum())} neighbour sets differ, largest |d - yardstick| / bound {err[worst] / bound[worst]:.3g} "
          f"(|d - yardstick| {err[worst]:.3g}, bound {bound[worst]:.3g}, order sensitivity up to {f['sensitivity'].max():.3g})")
    assert (err[same] <= bound[same]).all()
    zero = ~want.any(axis=1)
    assert not got[zero].any()
    n = np.array(f["normals"])[rows].astype(np.float64)
    assert np.abs((got * n).sum(axis=1)).max() <= 1e-6 * max(1.0, np.abs(got).max())          # tangent


def test_exact_clouds_and_the_zero_rule(icp):
    f = cfx.gradient_fixture("plane_linear")
    got = _run(icp, f)
    assert np.array_equal(got[:, :2], np.tile(np.float32(f["slope"][:2]), (len(got), 1)))       # 1.5 and -0.75: exact after the store
    assert np.abs(got[:, 2]).max() <= 1e-14                                                     # the normal component is dropped
    f = cfx.gradient_fixture("line")
    np.testing.assert_allclose(_run(icp, f), np.tile(f["axis"] * (f["axis"] @ f["slope"]), (len(f["points"]), 1)), atol=2.0 ** -25, rtol=0)
    assert not _run(icp, cfx.gradient_fixture("one_neighbour")).any()           # fewer than two neighbours
    pts = np.repeat(np.float32([[0.3, -0.2, 0.5]]), 40, axis=0)                     # every e_j zero: l_max = 0
    g = icp.estimate_color_gradients(pts, np.random.default_rng(0).random(40).astype(np.float32), knn=10)
    assert not g.cpu().numpy().any()
    one = icp.estimate_color_gradients(np.float32([[0.0, 0.0, 0.0]]), np.float32([0.5]), knn=5)
    assert one.shape == (1, 3) and not one.cpu().numpy().any()


def test_same_bits_on_two_calls_and_inputs_unmodified(icp):
    f = cfx.gradient_fixture("u257")
    dev = torch.device("cuda:0")
    P, N, I = (torch.tensor(np.array(f[k]), device=dev) for k in ("points", "normals", "intensity"))
    _, nb = icp.estimate_normals(P, knn=30, return_neighbors=True)
    before = [t.clone() for t in (P, N, I, nb)]
    a = icp.color_gradients(P, N, I, nb)
    b = icp.color_gradients(P, N, I, nb)
    assert torch.equal(a, b) and all(torch.equal(t, t0) for t, t0 in zip((P, N, I, nb), before))
    assert torch.equal(a, icp.estimate_color_gradients(P, I, normals=N, knn=30))
    # a zero or non-finite normal projects nothing out: the yardstick's plain 3-D gradient
    from tests import icp_color_reference as cref
    for bad in (0.0, float("nan"), float("inf")):
        Nb = torch.full_like(N, bad)
        got = icp.color_gradients(P, Nb, I, nb).cpu().numpy().astype(np.float64)
        want = cref.color_gradients(f["points"], np.full((len(f["points"]), 3), bad), f["intensity"], nb.cpu().numpy())
        assert np.abs(got - want).max() <= 2.0 ** -22 * np.abs(want).max()


def test_library_rejects_invalid_arguments(icp):
    from scorp_amd import _C
    L = _C.lib()
    dev = torch.device("cuda:0")
    P, N, out = torch.rand(8, 3, device=dev), torch.zeros(8, 3, device=dev), torch.zeros(8, 3, device=dev)
    I = torch.rand(8, device=dev)
    nb = torch.arange(8, dtype=torch.int32, device=dev).repeat(8, 1)[:, :5].contiguous()
    args = lambda **k: [k.get("p", P.data_ptr()), k.get("nrm", N.data_ptr()), k.get("i", I.data_ptr()), k.get("nb", nb.data_ptr()),
                        k.get("n", 8), k.get("knn", 5), k.get("o", out.data_ptr()), None]
    assert L.scorp_color_gradients(*args()) == 0
    for bad in (dict(knn=2), dict(knn=33), dict(n=0), dict(p=None), dict(nrm=None), dict(i=None), dict(nb=None), dict(o=None)):
        assert L.scorp_color_gradients(*args(**bad)) == _C.ERR_INVALID, bad
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="index"):
        icp.color_gradients(P, N, I, torch.full((8, 5), 8, dtype=torch.int32, device=dev))
