"""Multi-start coloured ICP on the GPU (scorp_icp_colored, scorp_amd/icp.py) against the float64 yardstick
tests/icp_color_reference.py, on the fixtures of tests/icp_color_fixtures.py (whose properties tests/test_icp_color_cpu.py
shows with the yardstick alone and which are asserted again here).  It mirrors tests/test_icp_gicp_gpu.py.

One update: transformation = reference_update(reference pairs) @ T0 to the larger of 10x the yardstick's own sensitivity to
the order of its pairs (measured by shuffling them) and the floor 1e-13 (1 + extent): icp_color_fixtures.one_update_bound,
every term measured on the yardstick, never on the code under test.  Runs of 0, 1 and 5 updates: the tolerances of
test_icp_gpu.test_margin_fixture_matches_yardstick.  The textured sheet: an RMS alignment error of at most twice the
yardstick's plus 1e-6 x extent in the yardstick's number of updates, with point-to-plane on the same clouds left above ten
times that.  The measured values are printed; DESIGN.md 4.10 holds them.

Measured in one MI355X run: one update at the block edges, |transformation - yardstick| 3.5e-17 - 6.1e-16 over the ten sizes,
two inits and two lambdas against the bound 1.9e-13, the floor in every case (the yardstick's own order sensitivity
0 - 3.9e-16); runs of 0 / 1 / 5 updates 0 / 1.3e-16 / 2.2e-16; a quarter of the normals and a quarter of the gradients zero
at most 1.5e-16; one source point 1.3e-16, one pair 4.4e-16, the planar target 6.1e-17, 64 identical points 2.9e-13 against
4.1e-12 (10x the yardstick's own 4.1e-13); constant colour against the GPU's point-to-plane run at most 4.2e-17, lambda = 1
the same bits; the textured sheet 5.0e-5 / 5.8e-5 in 3 updates (the yardstick's figures), point-to-plane 3.1e-3 after 100."""
import numpy as np
import pytest
import torch

from tests import icp_color_fixtures as cfx
from tests import icp_color_reference as cref
from tests import icp_plane_fixtures as pfx
from tests import icp_plane_reference as pref
from tests import icp_probe_fixtures as fx
from tests import icp_reference as ref
from tests.test_icp_gpu import ROT64

pytestmark = pytest.mark.gpu

FIELDS = ("transformation", "fitness", "inlier_rmse", "iterations")


@pytest.fixture(scope="module")
def icp():
    from scorp_amd import icp as m
    return m


def _colored(icp, src, Ip, tgt, nrm, Iq, grad, r, inits, lam, **kw):
    return icp.registration_icp(np.array(src), np.array(tgt), r, np.array(inits), estimation="colored", source_colors=np.array(Ip),
                                target_colors=np.array(Iq), target_normals=np.array(nrm), target_gradients=np.array(grad),
                                lambda_geometric=lam, **kw)


def _plane(icp, src, tgt, nrm, r, inits, **kw):
    return icp.registration_icp(np.array(src), np.array(tgt), r, np.array(inits), estimation="point_to_plane",
                                target_normals=np.array(nrm), **kw)


def _check_one_update(what, T, pairs, tgt, T0, lam, rng):
    """|T - yardstick| of one update from T0 under icp_color_fixtures.one_update_bound; returns the yardstick's transformation."""
    ct, s = pref.frame(tgt)
    extent = float(np.ptp(tgt.astype(np.float64), axis=0).max())
    _, eig = cref.reference_update(*pairs, lam, ct, s, return_eig=True)
    assert pref.eig_ratios_clear([eig])
    want, bound, own = cfx.one_update_bound(pairs, lam, ct, s, T0, extent, rng)
    d = float(np.abs(T - want).max())
    print(f"{what}: {len(pairs[0])} pairs, transformation to the yardstick {d:.3g} (bound {bound:.3g}; the yardstick's own order "
          f"sensitivity {own:.3g})")
    assert d <= bound
    return want


def _close(res, j, want, extent):
    """The tolerances of test_icp_gpu.test_margin_fixture_matches_yardstick, against a dict or another ICPResult's row."""
    assert res.fitness[j] == pytest.approx(want["fitness"], abs=1e-12)
    assert res.inlier_rmse[j] == pytest.approx(want["inlier_rmse"], rel=1e-6)
    np.testing.assert_allclose(res.transformation[j, :3, :3], want["transformation"][:3, :3], atol=1e-6)
    np.testing.assert_allclose(res.transformation[j, :3, 3], want["transformation"][:3, 3], atol=1e-6 * extent)


@pytest.mark.parametrize("ns", fx.AGGREGATE_NS)
def test_one_update_at_block_edges(icp, ns):
    src, tgt, r, inits, pairs = fx.aggregate_fixture(ns)
    Ip, (Iq, grad), nrm = cfx.aggregate_source_intensity(ns), cfx.aggregate_target_attributes(), pfx.aggregate_normals()
    assert pfx.poses_have_margin(src, tgt, list(inits), r, relative=False)        # the fixture property, again
    assert ns < 2 or len(np.unique(Ip)) > 0.99 * ns
    first = [cfx.first_pass(src, Ip, tgt, nrm, Iq, grad, r, T0) for T0 in inits]
    rng = np.random.default_rng(0)
    for lam in cfx.LAMBDAS:
        res0 = _colored(icp, src, Ip, tgt, nrm, Iq, grad, r, inits, lam, max_iteration=0)
        res1 = _colored(icp, src, Ip, tgt, nrm, Iq, grad, r, inits, lam, max_iteration=1, relative_fitness=0.0, relative_rmse=0.0)
        for j, (T0, (hit, idx)) in enumerate(zip(inits, pairs)):
            xs, qs = first[j][:2]
            c = len(xs)
            assert c == hit.sum() > 0 and res0.iterations[j] == 0 and res1.iterations[j] == 1
            assert int(round(res0.fitness[j] * ns)) == c
            assert res0.fitness[j] == pytest.approx(c / ns, abs=1e-15)
            rmse = float(np.sqrt(((xs - qs) ** 2).sum() / c))
            assert res0.inlier_rmse[j] == pytest.approx(rmse, rel=1e-9)           # Euclidean: no colour in it
            assert np.array_equal(res0.transformation[j], T0)
            _check_one_update(f"ns {ns} lambda {lam} init {j}", res1.transformation[j], first[j], tgt, T0, lam, rng)


@pytest.mark.parametrize("lam", cfx.LAMBDAS)
@pytest.mark.parametrize("max_iteration", [0, 1, 5])
def test_margin_fixture_matches_yardstick(icp, max_iteration, lam):
    src, Ip, tgt, nrm, Iq, grad, r, inits, runs = cfx.margin_fixture()
    assert pfx.poses_have_margin(src, tgt, [T for y in runs[lam] for T in y["poses"]], r)
    assert all(pref.eig_ratios_clear(y["eigenvalues"]) for y in runs[lam])
    res = _colored(icp, src, Ip, tgt, nrm, Iq, grad, r, inits, lam, max_iteration=max_iteration, relative_fitness=0.0, relative_rmse=0.0)
    extent = float(np.ptp(tgt, axis=0).max())
    for j, T0 in enumerate(inits):
        y = cref.registration_icp(src, Ip, tgt, nrm, Iq, grad, r, T0, lam, max_iteration=max_iteration, relative_fitness=0.0,
                                  relative_rmse=0.0)
        assert res.iterations[j] == y["iterations"] == max_iteration
        assert int(round(res.fitness[j] * len(src))) == y["passes"][-1]
        _close(res, j, y, extent)
        print(f"lambda {lam} max_iteration {max_iteration} init {j}: |T - yardstick| {np.abs(res.transformation[j] - y['transformation']).max():.3g}")


def test_constant_colour_and_lambda_one_give_the_point_to_plane_result(icp):
    src, Ip, tgt, nrm, Iq, grad, r, inits, _ = cfx.margin_fixture()
    extent = float(np.ptp(tgt, axis=0).max())
    flat_p, flat_q, zero = np.full(len(src), 0.4, np.float32), np.full(len(tgt), 0.4, np.float32), np.zeros_like(grad)
    for n in (0, 1, 5):
        kw = dict(max_iteration=n, relative_fitness=0.0, relative_rmse=0.0)
        want = _plane(icp, src, tgt, nrm, r, inits, **kw)
        cases = [(f"constant colour, lambda {lam}", _colored(icp, src, flat_p, tgt, nrm, flat_q, zero, r, inits, lam, **kw))
                 for lam in cfx.LAMBDAS]
        cases.append(("lambda 1", _colored(icp, src, Ip, tgt, nrm, Iq, grad, r, inits, 1.0, **kw)))
        for what, res in cases:
            assert np.array_equal(res.iterations, want.iterations)
            for j in range(len(inits)):
                _close(res, j, {f: getattr(want, f)[j] for f in FIELDS}, extent)
            print(f"{what}, {n} updates: |T - GPU point-to-plane| {np.abs(res.transformation - want.transformation).max():.3g}")


def test_no_pairs_and_no_constraint_keep_the_init(icp):
    src, Ip, tgt, nrm, Iq, grad, r, inits, _ = cfx.margin_fixture()
    T0 = np.array(inits[2])
    T0[:3, 3] += (5.0, 0.0, 0.0)
    res = _colored(icp, src, Ip, tgt, nrm, Iq, grad, 1e-3, T0, 0.968, max_iteration=30)
    assert res.fitness[0] == 0.0 and res.inlier_rmse[0] == 0.0
    assert np.array_equal(res.transformation[0], T0)
    res = _colored(icp, src, Ip, tgt, np.zeros_like(nrm), Iq, np.zeros_like(grad), r, inits, 0.5, max_iteration=7)
    assert np.array_equal(res.transformation, inits) and (res.fitness > 0.5).all() and (res.inlier_rmse > 0).all()


def test_pairs_with_one_term_zero_count_and_add_the_other(icp):
    src, _, tgt, _, Iq, _, r, inits, _ = cfx.margin_fixture()
    Ip, nrm, grad, no_normal, no_gradient = cfx.quarter_zero()
    rng = np.random.default_rng(0)
    for lam in cfx.LAMBDAS:
        res0 = _colored(icp, src, Ip, tgt, nrm, Iq, grad, r, inits, lam, max_iteration=0)
        res1 = _colored(icp, src, Ip, tgt, nrm, Iq, grad, r, inits, lam, max_iteration=1, relative_fitness=0.0, relative_rmse=0.0)
        for j, T0 in enumerate(inits):
            xs, si, ti = cfx.first_pairs(src, tgt, T0, r)
            assert np.isin(ti, no_normal).sum() > 30 and np.isin(ti, no_gradient).sum() > 30
            assert int(round(res0.fitness[j] * len(src))) == len(xs)          # the pairs with a zero term still count
            _check_one_update(f"a quarter without normals, a quarter without gradients, lambda {lam} init {j}",
                              res1.transformation[j], cfx.first_pass(src, Ip, tgt, nrm, Iq, grad, r, T0), tgt, T0, lam, rng)


@pytest.mark.parametrize("name", cfx.RANK_DEFICIENT)
def test_degenerate_systems_take_the_minimum_norm_step(icp, name):
    src, Ip, tgt, nrm, Iq, grad, r, y = cfx.rank_deficient(name)
    lam = cfx.LAMBDAS[0]
    if name != "identical64":
        assert pfx.poses_have_margin(src, tgt, y["poses"], r)
    assert pref.eig_ratios_clear(y["eigenvalues"])
    res = _colored(icp, src, Ip, tgt, nrm, Iq, grad, r, np.eye(4), lam, max_iteration=1, relative_fitness=0.0, relative_rmse=0.0)
    T = res.transformation[0]
    assert np.isfinite(T).all() and res.iterations[0] == 1
    assert np.linalg.det(T[:3, :3]) == pytest.approx(1.0, abs=1e-9)
    assert int(round(res.fitness[0] * len(src))) == y["passes"][-1]
    want = _check_one_update(name, T, cfx.first_pass(src, Ip, tgt, nrm, Iq, grad, r, np.eye(4)), tgt, np.eye(4), lam,
                             np.random.default_rng(0))
    np.testing.assert_allclose(want, y["poses"][1], atol=1e-14)


@pytest.mark.parametrize("lam", cfx.LAMBDAS)
def test_textured_sheet_is_fixed_by_its_colour(icp, lam):
    s = cfx.textured_sheet()
    src, Ip, tgt, nrm, Iq, grad, r = (s[k] for k in ("source", "source_intensity", "target", "normals", "target_intensity",
                                                     "gradients", "r"))
    y = s["colored"][lam]
    assert pfx.poses_have_margin(src, tgt, y["poses"], r, relative=False) and pref.eig_ratios_clear(y["eigenvalues"])
    extent = float(np.ptp(tgt.astype(np.float64), axis=0).max())
    ey = cfx.rms_alignment_error(y["transformation"], src)
    assert ey < 0.1 * cfx.rms_alignment_error(s["plane"]["transformation"], src)
    res = _colored(icp, src, Ip, tgt, nrm, Iq, grad, r, np.eye(4), lam, max_iteration=cfx.SHEET_MAX_ITERATION)
    plane = _plane(icp, src, tgt, nrm, r, np.eye(4), max_iteration=cfx.SHEET_MAX_ITERATION)
    ec, ep = cfx.rms_alignment_error(res.transformation[0], src), cfx.rms_alignment_error(plane.transformation[0], src)
    print(f"textured sheet, lambda {lam}: start {s['start']:.3g}; coloured {ec:.3g} in {res.iterations[0]} updates (yardstick {ey:.3g} "
          f"in {y['iterations']}); point-to-plane {ep:.3g} in {plane.iterations[0]}")
    assert ec <= 2.0 * ey + 1e-6 * extent
    assert res.iterations[0] == y["iterations"]
    assert ep > 10.0 * ec


def _textured_planted():
    """icp_plane_fixtures.planted()'s clouds with a smooth texture of position as their colours [n, 3]."""
    src, tgt, nrm, r, R0, t0, _, _ = pfx.planted()

    def colours(p):
        i = cfx.smooth_texture(p)
        return np.stack([i, 0.5 * i + 0.25, 1.0 - i], axis=1).astype(np.float32)

    return src, colours(src.astype(np.float64) @ R0.T + t0), tgt, colours(tgt), nrm, r, R0, t0


def test_deterministic_and_batch_independent(icp):
    src, Cp, tgt, Cq, nrm, r, _, _ = _textured_planted()
    rots = np.load(ROT64)["rotations"][:4]
    inits = ref.icp_inits(rots, tgt.mean(axis=0), src.mean(axis=0))
    assert len(inits) == 7
    G = icp.estimate_color_gradients(np.array(tgt), Cq, normals=np.array(nrm))
    run = lambda T: icp.registration_icp(np.array(src), np.array(tgt), r, T, max_iteration=40, estimation="colored", source_colors=Cp,
                                         target_colors=Cq, target_normals=np.array(nrm), target_gradients=G)
    a, b = run(inits), run(inits)
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert len(set(a.iterations.tolist())) > 1           # inits that stop at different passes
    for j in (0, 2, len(inits) - 1):
        s = run(inits[j])
        for f in FIELDS:
            assert np.array_equal(getattr(s, f)[0], getattr(a, f)[j]), (f, j)


def test_inputs_unmodified(icp):
    src, Ip, tgt, nrm, Iq, grad, r, inits, _ = cfx.margin_fixture()
    inits = np.array(inits)
    dev = torch.device("cuda:0")
    tensors = [torch.tensor(np.array(a), device=dev) for a in (src, Ip, tgt, nrm, Iq, grad)]
    before = [t.clone() for t in tensors]
    I0 = inits.copy()
    S, P, Q, N, C, G = tensors
    icp.registration_icp(S, Q, r, inits, max_iteration=10, estimation="colored", source_colors=P, target_colors=C, target_normals=N,
                         target_gradients=G)
    assert all(torch.equal(t, t0) for t, t0 in zip(tensors, before)) and np.array_equal(inits, I0)


def test_colour_forms_and_defaults(icp):
    src, Ip, tgt, nrm, Iq, grad, r, inits, _ = cfx.margin_fixture()
    a = _colored(icp, src, Ip, tgt, nrm, Iq, grad, r, inits, 0.968, max_iteration=5)
    rgb_p, rgb_q = np.repeat(np.array(Ip)[:, None], 3, axis=1), torch.tensor(np.repeat(np.array(Iq)[:, None], 3, axis=1), device="cuda:0")
    b = icp.registration_icp(np.array(src), np.array(tgt), r, np.array(inits), max_iteration=5, estimation="colored", source_colors=rgb_p,
                             target_colors=rgb_q, target_normals=np.array(nrm), target_gradients=torch.tensor(np.array(grad)))
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    I = icp.intensities(np.array([[0.25, 0.5, 0.75], [1.0, 0.0, 0.5]]))
    assert I.is_cuda and I.dtype == torch.float32 and I.tolist() == [0.5, 0.5]
    assert torch.equal(icp.intensities(torch.tensor(np.array(Iq))), torch.tensor(np.array(Iq), device="cuda:0"))
    # None: estimate_normals of the target, estimate_color_gradients on them
    s, Cp, tgt, Cq, _, r, _, _ = _textured_planted()
    kw = dict(max_iteration=10, estimation="colored", source_colors=Cp, target_colors=Cq)
    default = icp.registration_icp(np.array(s), np.array(tgt), r, np.eye(4), **kw)
    N, G = icp.estimate_normals(np.array(tgt), knn=30), icp.estimate_color_gradients(np.array(tgt), Cq)
    assert G.shape == (len(tgt), 3) and G.dtype == torch.float32 and G.is_cuda
    assert torch.equal(G, icp.estimate_color_gradients(np.array(tgt), Cq, normals=N))
    explicit = icp.registration_icp(np.array(s), np.array(tgt), r, np.eye(4), target_normals=N, target_gradients=G, **kw)
    only_normals = icp.registration_icp(np.array(s), np.array(tgt), r, np.eye(4), target_normals=N, **kw)
    only_gradients = icp.registration_icp(np.array(s), np.array(tgt), r, np.eye(4), target_gradients=G, **kw)
    for f in FIELDS:
        for other in (explicit, only_normals, only_gradients):
            assert np.array_equal(getattr(default, f), getattr(other, f)), f
    assert default.fitness[0] > 0.9


def test_argument_errors(icp):
    src, Ip, tgt, nrm, Iq, grad, r, inits, _ = cfx.margin_fixture()
    for bad_p, bad_q in ((Ip[:-1], Iq), (Ip, Iq[:-1]), (Ip, np.zeros((len(tgt), 2), np.float32))):
        with pytest.raises(ValueError):
            _colored(icp, src, bad_p, tgt, nrm, bad_q, grad, r, inits, 0.968)
    for v in (np.nan, np.inf):
        bad = np.array(Iq)
        bad[3] = v
        with pytest.raises(ValueError):
            _colored(icp, src, Ip, tgt, nrm, bad, grad, r, inits, 0.968)
    with pytest.raises(ValueError):
        _colored(icp, src, Ip, tgt, nrm[:-1], Iq, grad, r, inits, 0.968)
    with pytest.raises(ValueError):
        _colored(icp, src, Ip, tgt, nrm, Iq, grad, r, inits, 1.0 + 1e-9)


def test_null_pointers_and_lambda_are_invalid(icp):
    from scorp_amd import _C
    src, Ip, tgt, nrm, Iq, grad, r, inits, _ = cfx.margin_fixture()
    dev = torch.device("cuda:0")
    S, P, Q, N, C, G = (torch.tensor(np.array(a), device=dev) for a in (src, Ip, tgt, nrm, Iq, grad))
    T_in = torch.tensor(np.array(inits[:1]), device=dev)
    T_out = torch.empty_like(T_in)
    fit, rmse = torch.empty(1, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.float64, device=dev)
    iters = torch.empty(1, dtype=torch.int32, device=dev)
    L = _C.lib()
    size = L.scorp_icp_colored_workspace_bytes(len(src), len(tgt), 1)
    assert size % 256 == 0 and size >= L.scorp_icp_point_to_plane_workspace_bytes(len(src), len(tgt), 1) + len(src) * 4
    ws = torch.empty(size, dtype=torch.uint8, device=dev)

    def run(p=P.data_ptr(), n=N.data_ptr(), c=C.data_ptr(), g=G.data_ptr(), lam=0.968, bytes_=size):
        return L.scorp_icp_colored(S.data_ptr(), p, len(src), Q.data_ptr(), n, c, g, len(tgt), T_in.data_ptr(), 1, r, 1, 0.0, 0.0, lam,
                                   T_out.data_ptr(), fit.data_ptr(), rmse.data_ptr(), iters.data_ptr(), ws.data_ptr(), bytes_,
                                   _C.current_stream_ptr())

    for bad in (dict(p=None), dict(n=None), dict(c=None), dict(g=None)):
        assert run(**bad) == _C.ERR_INVALID, bad
        assert b"NULL" in L.scorp_last_error()
    for lam in (-1e-9, 1.0 + 1e-9, float("nan"), float("inf")):
        assert run(lam=lam) == _C.ERR_INVALID, lam
        assert b"lambda" in L.scorp_last_error()
    # the workspace of the point-to-plane call is too small: the sorted intensities come after it
    assert run(bytes_=L.scorp_icp_point_to_plane_workspace_bytes(len(src), len(tgt), 1)) == _C.ERR_INVALID
    assert b"workspace" in L.scorp_last_error()
    for lam in (0.0, 1.0, 0.968):
        assert run(lam=lam) == 0
    torch.cuda.synchronize()


def test_best_transformation_uses_the_colours(icp):
    src, Cp, tgt, Cq, nrm, r, R0, t0 = _textured_planted()
    rots = np.load(ROT64)["rotations"][:4]
    best = icp.get_ICP_fitting_transformation_best(np.array(tgt), np.array(src), rots, r, estimation="colored", source_colors=Cp,
                                                   target_colors=Cq, target_normals=np.array(nrm))
    assert best.shape == (4, 4) and best.dtype == np.float64
    print(f"planted pair, 4 rotations: coloured |R - R0| {np.abs(best[:3, :3] - R0).max():.3g}, |t - t0| {np.abs(best[:3, 3] - t0).max():.3g}")
    assert np.abs(best[:3, :3] - R0).max() < 0.02 and np.abs(best[:3, 3] - t0).max() < 0.02
    # a refined cloud more than 4x the original: the source colours are subsampled with their points
    few, Cfew, nfew = np.array(tgt)[::10], Cq[::10], np.array(nrm)[::10]
    keep = icp.downsample_indices(len(few), len(src))
    assert len(keep) == len(src) // 2
    G = icp.estimate_color_gradients(few, Cfew, normals=nfew)
    best = icp.get_ICP_fitting_transformation_best(few, np.array(src), rots, r, estimation="colored", source_colors=torch.tensor(Cp),
                                                   target_colors=Cfew, target_normals=nfew, target_gradients=G, lambda_geometric=0.9)
    inits = icp.icp_inits(rots, few.mean(axis=0), np.array(src).mean(axis=0))
    res = icp.registration_icp(np.array(src)[keep], few, r, inits, max_iteration=400, estimation="colored", source_colors=Cp[keep],
                               target_colors=Cfew, target_normals=nfew, target_gradients=G, lambda_geometric=0.9)
    assert np.array_equal(best, res.transformation[int(np.argmax(res.fitness))])
