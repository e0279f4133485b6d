"""The pose fit on the GPU (scorp_pose_ransac, scorp_pose_adam_9dof; csrc/pose_fit.hip, svd3.hpp) against the float64
yardstick (tests/pose_fit_reference.py) at block edges, ties, early exits, reflections and degenerate fits, on the seeded
cases of tests/pose_fit_fixtures.py.  tests/test_pose_fit_edges_cpu.py checks, on the yardstick alone, that every case
has the margin, the conditioning and the structure these comparisons need.

RANSAC, exact comparison: ALL counts equal, the winner and its count equal, the mask equal to the yardstick's,
|dR|, |ds| <= 1e-9 and |dt| <= 1e-9 max(1, largest |coordinate|).  The degenerate samples (rank 1, rank 0) are compared by
properties only, because LAPACK's completion of a zero singular direction is arbitrary; each such test says which.

Adam: per array max(10 x the yardstick's own spread, 1e-9 max(1, largest |coordinate|)); the spread is the largest distance
among three yardstick runs (as given, pairs permuted, loss written about the centroids).  Cases that start from three equal
scales leave rotation_orthogonal undetermined (its gradient is rounding noise that Adam normalises): they hold rotation,
translation, scale and M, and rotation_orthogonal only through M.

Every bound here is the project's 1e-9 scaled by the data, a spread of the yardstick alone, or a structural fact (equal
counts, the first index, bit equality); no number comes from the kernel.  Each test prints what it measured.

Distances measured on an MI355X, the largest of each family (DESIGN.md 4.11 holds them too).  RANSAC, kernel to yardstick;
in every family all counts, the winner and the mask were equal:
  family (cases)                                        |dR|      |ds|      |dt|      bound on dR, ds / on dt
  block edges, n = 3 .. 3073, both methods (30)         2.9e-15   1.5e-15   5.0e-16   1e-9 / 1e-9 .. 1.7e-9
  hypothesis counts 1 .. 129 and 65 535 (7)             9.7e-16   2.2e-16   1.7e-16   1e-9 / 1e-9 .. 1.1e-9
  ties (6)                                              5.6e-16   0         1.1e-16   1e-9 / 1.4e-9
  early exits (6)                                       6.7e-16   1.1e-15   5.0e-16   1e-9 / 1.5e-9 .. 5.4e-8
  three inliers                                         3.8e-16   4.4e-16   1.1e-16   1e-9 / 3.9e-9
  reflection, both methods                              5.6e-16   1.1e-16   2.8e-16   1e-9 / 1.2e-9 .. 1.3e-9
  rank 2: plane, slab, three inliers                    1.9e-15   6.7e-16   1.1e-16   1e-9 / 1.2e-9 .. 6e-9
  coordinates x 1e-6 / x 1e6 / + 1e5                    6.7e-16   1.1e-15   3.2e-22 / 2.9e-10 / 1.6e-10   1e-9 / 1e-9, 1.6e-3, 1e-4
  non-finite pairs, both methods                        4.4e-16   4.4e-16   1.7e-16   1e-9 / 1.2e-9 .. 1.4e-9
  collinear inliers (by properties)                     |R R^T - I| 2.4e-16, det R - 1 = 0, worst inlier residual 3.7e-16 (threshold 1e-6)
Adam, kernel to yardstick (10x the yardstick's spread; the floor), the largest of each family:
  family                  rotation                    translation                 scale                       rotation_orthogonal          M
  sizes, equal scales     4.7e-14 (4.0e-13; 1.5e-9)   4.1e-15 (8.5e-14; 1.5e-9)   2.6e-13 (5.0e-12; 1.5e-9)   not held (9.5e-11)           3.5e-13 (4.5e-12; 1.5e-9)
  sizes, distinct scales  3.3e-16 (1.4e-15; 1.5e-9)   1.5e-16 (1.4e-16; 1.5e-9)   2.2e-16 (2.2e-15; 1.5e-9)   7.2e-16 (1.0e-14; 1.5e-9)    4.4e-16 (6.7e-15; 1.5e-9)
  outside = mid-point     1.2e-14 (1.5e-13; 1.2e-9)   3.5e-16 (2.9e-15; 1.2e-9)   7.4e-14 (6.9e-13; 1.2e-9)   not held (7.6e-12)           9.3e-14 (9.3e-13; 1.2e-9)
  other bounds            3.0e-16 (1.1e-15; 1.2e-9)   1.4e-16 (2.8e-16; 1.2e-9)   2.2e-16 (2.2e-15; 1.2e-9)   3.4e-15 (2.5e-13; 1.2e-9)    4.7e-16 (9.4e-15; 1.2e-9)
  regularisers (8)        1.7e-16 (1.4e-15; 1.2e-9)   3.0e-16 (5.6e-16; 1.2e-9)   4.4e-16 (2.2e-15; 1.2e-9)   2.6e-15 (9.0e-14; 1.2e-9)    1.1e-15 (1.1e-14; 1.2e-9)
  shifted by 100          8.3e-17 (4.9e-16; 1e-7)     3.1e-16 (1.0e-15; 1e-7)     0 (0; 1e-7)                 2.0e-16 (8.3e-16; 1e-7)      1.3e-16 (1.1e-15; 1e-7)
  shifted by 1e4          1.8e-16 (5.2e-16; 1e-5)     1.8e-15 (8.3e-15; 1e-5)     4.4e-16 (2.2e-15; 1e-5)     7.7e-16 (2.4e-15; 1e-5)      3.3e-16 (2.2e-15; 1e-5)
  one step                3.5e-18 (0; 1.2e-9)         0 (0; 1.2e-9)               0 (0; 1.2e-9)               4.3e-19 (0; 1.2e-9)          6.9e-18 (0; 1.2e-9)
  loss traces of the regulariser cases: largest relative distance 2.8e-11 (rtol 1e-9); zero iterations: 0 to the start.
In "sizes, distinct scales" the translation's 1.5e-16 is above 10x the spread (1.4e-16): the spread alone is no bound where
the yardstick's runs come out bit-equal, which is what the floor is for."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

from tests import pose_fit_fixtures as fx
from tests import pose_fit_reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pf():
    from scorp_amd import pose_fit as m
    return m


def run(pf, c, tri=None):
    return pf.ransac_fit(c.p, c.q, c.tri if tri is None else tri, c.thr, c.ratio, c.method)


def raw_ransac(pf, c):
    """scorp_pose_ransac through the C ABI, for the calls that end in ERR_NO_INLIERS: (code, winner, count, counts, the 16 doubles
    R, t and s are written into, -3 before the call)."""
    from scorp_amd import _C
    L, dev = _C.lib(), torch.device("cuda", torch.cuda.current_device())
    P, Q = pf._pairs(c.p, c.q, dev)
    tri = torch.as_tensor(np.ascontiguousarray(c.tri, dtype=np.int32), device=dev)
    n, nh = len(c.p), len(c.tri)
    out = torch.full((16,), -3.0, dtype=torch.float64, device=dev)
    win = torch.full((2,), -7, dtype=torch.int32, device=dev)
    counts = torch.full((nh,), -7, dtype=torch.int32, device=dev)
    mask = torch.zeros(n, dtype=torch.uint8, device=dev)
    ws, ws_ptr, ws_bytes = pf._workspace(L, n, nh, dev)
    code = L.scorp_pose_ransac(P.data_ptr(), Q.data_ptr(), n, tri.data_ptr(), nh, ctypes.c_double(c.thr), ctypes.c_double(c.ratio),
                               pf.METHODS[c.method], out.data_ptr(), out.data_ptr() + 72, out.data_ptr() + 96, win.data_ptr(),
                               counts.data_ptr(), mask.data_ptr(), ws_ptr, ws_bytes, _C.current_stream_ptr())
    torch.cuda.synchronize()
    return code, int(win[0]), int(win[1]), counts.cpu().numpy(), out.cpu().numpy()


def compare_exactly(c, fit, y, bound=fx.BOUND):
    """Every count, the winner, the mask, and R, t, s within the bound of the yardstick's fit over the mask."""
    assert np.array_equal(fit.counts, y["counts"])
    assert fit.winner == y["winner"] and fit.count == y["count"]
    assert np.array_equal(fit.mask, y["mask"])
    dR, dt, ds = np.abs(fit.R - y["R"]).max(), np.abs(fit.t - y["t"]).max(), abs(fit.s - y["s"])
    print(f"{c.name}: n {len(c.p)} nh {len(c.tri)} winner {fit.winner} count {fit.count} |dR| {dR:.3g} |ds| {ds:.3g} (bound {bound:.3g}) "
          f"|dt| {dt:.3g} (bound {bound * c.extent:.3g})")
    assert dR <= bound and ds <= bound and dt <= bound * c.extent
    assert abs(np.linalg.det(fit.R) - 1.0) <= 1e-12


# ---- RANSAC ----

@pytest.mark.parametrize("name", fx.EDGE_CASES + fx.NH_CASES)
def test_ransac_at_block_and_hypothesis_count_edges(pf, name):
    c = fx.ransac_case(name)
    compare_exactly(c, run(pf, c), fx.ransac_yardstick(name))


@pytest.mark.parametrize("name", fx.TIE_CASES)
def test_ties_go_to_the_lowest_slot(pf, name):
    c = fx.ransac_case(name)
    fit = run(pf, c)
    assert fit.winner == min(c.note["slots"])
    compare_exactly(c, fit, fx.ransac_yardstick(name))


@pytest.mark.parametrize("name", fx.EARLY_CASES)
def test_early_exit(pf, name):
    """before / at the global maximum, a ratio nothing exceeds, a count equal to ratio * n (not exceeded), ratio 1e-12."""
    c = fx.ransac_case(name)
    compare_exactly(c, run(pf, c), fx.ransac_yardstick(name))


@pytest.mark.parametrize("name", ["early-tiny-error", "count-2"])
def test_fewer_than_three_inliers_is_the_reference_error(pf, name):
    """The first hypothesis with any inlier has 1 or 2 (ratio 1e-12), or the best count is 2: ERR_NO_INLIERS / ValueError,
    with every count, the winner and its count written and equal to the yardstick's."""
    from scorp_amd import _C
    c, y = fx.ransac_case(name), fx.ransac_yardstick(name)
    with pytest.raises(ValueError, match="No inliers found in RANSAC."):
        run(pf, c)
    code, winner, count, counts, out = raw_ransac(pf, c)
    assert code == _C.ERR_NO_INLIERS
    assert np.array_equal(counts, y["counts"]) and winner == y["winner"] and count == y["count"] < 3
    assert (out == -3.0).all()                                                # R, t, s are left alone


def test_three_inliers_is_a_fit(pf):
    """The other side of the boundary: the fixture that differs from count-2 in one pair."""
    c = fx.ransac_case("count-3")
    fit = run(pf, c)
    assert fit.count == 3
    compare_exactly(c, fit, fx.ransac_yardstick("count-3"))


@pytest.mark.parametrize("name", fx.REFLECTION_CASES)
def test_reflection_takes_the_determinant_rule_at_full_rank(pf, name):
    c = fx.ransac_case(name)
    fit = run(pf, c)
    assert fit.count == len(c.p)
    compare_exactly(c, fit, fx.ransac_yardstick(name))                         # det R = +1 to 1e-12 in there; s with the same rule


@pytest.mark.parametrize("name", fx.RANK2_CASES)
def test_rank_two_final_fit(pf, name):
    """Planar inliers, a slab below svd3's rank threshold, exactly three inliers: the first two singular directions and the
    determinant fix the rotation, so the comparison is exact.  For the slab the plain 1e-9 applies: the yardstick's own
    answer moves by less than that under a permutation of the pairs (asserted in the CPU test)."""
    c = fx.ransac_case(name)
    compare_exactly(c, run(pf, c), fx.ransac_yardstick(name))


@pytest.mark.parametrize("name", fx.SCALE_CASES)
def test_scale_and_offset(pf, name):
    c, y = fx.ransac_case(name), fx.ransac_yardstick(name)
    fit = run(pf, c)
    assert np.array_equal(fit.counts, fx.ransac_yardstick("edge-1025-umeyama")["counts"])   # what the unscaled cloud counts
    compare_exactly(c, fit, y)


@pytest.mark.parametrize("name", fx.NONFINITE_CASES)
def test_non_finite_pairs_count_nothing(pf, name):
    c, y = fx.ransac_case(name), fx.ransac_yardstick(name)
    fit = run(pf, c)
    assert (fit.counts[list(c.note["hyps"])] == 0).all() and not fit.mask[list(c.note["pairs"])].any()
    compare_exactly(c, fit, y)                                                 # every other count, the mask, the fit over it


@pytest.mark.parametrize("method", fx.METHODS)
def test_degenerate_triples_by_properties(pf, method):
    """(i, i, j), three collinear pairs and (i, i, i) among ordinary triples.  LAPACK completes the zero singular directions
    of a rank-1 or rank-0 covariance arbitrarily, so the degenerate hypotheses have no unique count: they are held to the
    count of their own distinct sample pairs under the line-to-line map that any completion contains (fx.line_inliers), the
    ordinary ones to the exact comparison."""
    c = fx.ransac_case(f"degenerate-{method}")
    rep, col, same = c.note["hyps"]
    ordinary = np.setdiff1d(np.arange(len(c.tri)), c.note["hyps"])
    fit = run(pf, c)
    alone = run(pf, c, c.tri[ordinary])
    want = ref.ransac_counts(c.p, c.q, c.tri[ordinary], c.thr, method)
    assert np.array_equal(fit.counts[ordinary], alone.counts) and np.array_equal(alone.counts, want)
    for h in (rep, col, same):
        least = fx.line_inliers(c, h)[0]
        print(f"{method} degenerate hypothesis {h} {c.tri[h]}: count {fit.counts[h]}, its sample pairs under the line map {least}")
        if method == "umeyama" and h == same:
            assert fit.counts[h] == 0                                          # s = 0 / 0
        else:
            assert fit.counts[h] >= least
    assert fit.winner in ordinary and fit.winner == ordinary[alone.winner]
    assert np.isfinite(fit.R).all() and np.isfinite(fit.t).all() and np.isfinite(fit.s)
    assert np.array_equal(fit.R, alone.R) and np.array_equal(fit.t, alone.t) and fit.s == alone.s
    assert np.array_equal(fit.mask, alone.mask)


@pytest.mark.parametrize("method", fx.METHODS)
def test_collinear_inliers_by_properties(pf, method):
    """The winner's inliers lie on a line: the final covariance has rank 1 and the rotation about the line is free, so R is
    held to being a rotation that maps the inliers onto their targets, not to LAPACK's choice."""
    c = fx.ransac_case(f"collinear-winner-{method}")
    fit = run(pf, c)
    assert fit.winner == 7 and fit.count >= 40 and fit.mask[:40].all()
    orth, det = np.abs(fit.R @ fit.R.T - np.eye(3)).max(), np.linalg.det(fit.R)
    res = ref.residuals(c.p[fit.mask], c.q[fit.mask], fit.R, fit.t, fit.s)
    print(f"collinear-winner-{method}: |R R^T - I| {orth:.3g}, det R - 1 {det - 1:.3g}, worst inlier residual {res.max():.3g} (threshold {c.thr})")
    assert orth <= 1e-12 and abs(det - 1) <= 1e-12 and (res < c.thr).all()
    if method == "umeyama":
        assert abs(fit.s - 1.2) <= fx.BOUND


def test_batch_independence_at_the_edges(pf):
    c = fx.ransac_case("edge-1025-umeyama")
    tri = c.tri[:65]
    batch = run(pf, c, tri)
    for h in (0, 63, 64):                                                      # (through the C ABI: a lone count may be below 3)
        assert raw_ransac(pf, dataclasses.replace(c, tri=tri[h:h + 1]))[3][0] == batch.counts[h]
    alone = run(pf, c, tri[batch.winner:batch.winner + 1])
    assert np.array_equal(alone.R, batch.R) and np.array_equal(alone.t, batch.t) and alone.s == batch.s
    assert np.array_equal(alone.mask, batch.mask)
    again = run(pf, c, tri)
    assert np.array_equal(again.R, batch.R) and np.array_equal(again.t, batch.t) and np.array_equal(again.counts, batch.counts)


# ---- Adam ----

def run_adam(pf, c, **over):
    got = pf.adam_fit_9dof(c.p, c.q, **{**c.kw, **over})
    got["M"] = ref.compose(got["rotation"], got["scale"], got["rotation_orthogonal"])
    return got


def compare_adam(c, got, y, bound):
    held = [k for k in fx.ADAM_ARRAYS if c.holds_ro or k != "rotation_orthogonal"]
    for k in fx.ADAM_ARRAYS:
        d = np.abs(got[k] - y[k]).max()
        print(f"{c.name} {k}: kernel to yardstick {d:.3g}; 10x yardstick spread {bound[k][0]:.3g}, floor {bound[k][1]:.3g}"
              + ("" if k in held else "  (not held: undetermined from equal scales)"))
    for k in held:
        assert np.abs(got[k] - y[k]).max() <= max(bound[k][:2]), k


@pytest.mark.parametrize("name", fx.ADAM_SIZE_CASES + fx.ADAM_SCALE_CASES + fx.ADAM_FAR_CASES + ["one-step"])
def test_adam_matches_the_yardstick(pf, name):
    """Sizes at the block edges, start scales (equal, distinct, outside the bounds), other bounds, clouds far from the
    origin, and ONE step: Adam's first step is lr * sign(g), a sign check of the gradients (the CPU test shows 13 of the 14
    far from 0 there and the 14th, qo's along qo, identically 0)."""
    c = fx.adam_case(name)
    y, bound = fx.adam_yardstick(name)
    compare_adam(c, run_adam(pf, c), y, bound)


@pytest.mark.parametrize("name", fx.ADAM_REG_CASES)
def test_adam_regularisers_that_matter(pf, name):
    """Lambdas large enough that a 1 % error in any regulariser gradient term moves M or the scales by 100x the bound
    (tests/test_pose_fit_edges_cpu.py::test_regulariser_cases_can_see_one_per_cent)."""
    c = fx.adam_case(name)
    y, bound = fx.adam_yardstick(name)
    got = run_adam(pf, c)
    assert got["losses"].shape == y["losses"].shape == (20,)
    print(f"{name}: loss trace, largest relative distance {np.abs(got['losses'] / y['losses'] - 1).max():.3g} (rtol 1e-9)")
    compare_adam(c, got, y, bound)
    np.testing.assert_allclose(got["losses"], y["losses"], rtol=1e-9)
    assert abs(got["loss"] - y["loss"]) <= 1e-9 * abs(y["loss"])


def test_adam_start_scale_outside_the_bounds_is_the_mid_point(pf):
    a, b = run_adam(pf, fx.adam_case("outside")), run_adam(pf, fx.adam_case("midpoint"))
    for k in fx.ADAM_ARRAYS[:4]:
        assert np.array_equal(a[k], b[k]), k
    assert a["loss"] == b["loss"]


def test_adam_zero_iterations_returns_the_start(pf):
    c = fx.adam_case("n-1025-distinct")
    got = run_adam(pf, c, iterations=0)
    f32 = lambda v: torch.tensor(v, dtype=torch.float32).double()
    dR = np.abs(got["rotation"] - ref.quaternion_to_matrix(f32([0.9, 0.01, 0.01, 0.01])).numpy()).max()
    ds = np.abs(got["scale"] - np.array(fx.DISTINCT)).max()
    print(f"iterations = 0: rotation to the start quaternion's matrix {dR:.3g}, scale to the start scale {ds:.3g} (bound {fx.BOUND})")
    assert dR <= fx.BOUND and ds <= fx.BOUND                                   # two float64 evaluations; logit then sigmoid
    assert np.array_equal(got["rotation_orthogonal"], np.eye(3))              # qo = (1, 0, 0, 0): exact in any evaluation order
    assert np.array_equal(got["translation"], np.float64(np.float32([0.01] * 3)))
    assert got["loss"] == 0.0 and len(got["losses"]) == 0


@pytest.mark.parametrize("name", ["n-1025-distinct", "n-3-distinct"])
def test_adam_two_calls_give_the_same_bits(pf, name):
    c = fx.adam_case(name)
    a, b = run_adam(pf, c, loss_every=10), run_adam(pf, c, loss_every=10)
    for k in fx.ADAM_ARRAYS[:4] + ("losses",):
        assert np.array_equal(a[k], b[k]), k
    assert a["loss"] == b["loss"]


def test_adam_loss_trace_through_the_c_abi(pf):
    from scorp_amd import _C
    L, dev = _C.lib(), torch.device("cuda", torch.cuda.current_device())
    c = fx.adam_case("reg-0.3-0.3-0.01")
    P, Q = pf._pairs(c.p, c.q, dev, through_fp32=True)
    ws, ws_ptr, ws_bytes = pf._workspace(L, len(c.p), 1, dev)
    s0 = (ctypes.c_double * 3)(*fx.DISTINCT)
    f64 = ctypes.c_double

    def adam(iterations, every, capacity):
        out = torch.zeros(25, dtype=torch.float64, device=dev)
        trace = torch.full((64,), -7.0, dtype=torch.float64, device=dev)
        code = L.scorp_pose_adam_9dof(P.data_ptr(), Q.data_ptr(), len(c.p), iterations, f64(1e-2), f64(0.3), f64(0.3), f64(0.75),
                                      f64(1.5), s0, out.data_ptr(), trace.data_ptr(), every, capacity, ws_ptr, ws_bytes,
                                      _C.current_stream_ptr())
        assert code == 0
        torch.cuda.synchronize()
        return out.cpu().numpy(), trace.cpu().numpy()

    y = ref.adam_9dof(c.p, c.q, **{**c.kw, "iterations": 50, "loss_every": 1})["losses"]
    out, trace = adam(50, 10, 2)                                              # five entries due, room for two
    np.testing.assert_allclose(trace[:2], y[[9, 19]], rtol=1e-9)
    assert (trace[2:] == -7.0).all()
    out_all, trace = adam(50, 10, 64)
    np.testing.assert_allclose(trace[:5], y[9::10], rtol=1e-9)
    assert (trace[5:] == -7.0).all() and trace[4] == out_all[24]               # out[24]: the last iteration's loss
    assert np.array_equal(out_all, out)                                        # the trace does not change the run
    out, trace = adam(50, 1, 64)                                               # every iteration's loss
    np.testing.assert_allclose(trace[:50], y, rtol=1e-9)
    assert (trace[50:] == -7.0).all() and trace[49] == out[24]
    out, trace = adam(50, 51, 64)                                              # loss_every > iterations: nothing is due
    assert (trace == -7.0).all() and out[24] == out_all[24]
    out, trace = adam(47, 10, 64)                                              # the last iteration is not a due one
    assert (trace[4:] == -7.0).all() and abs(out[24] - y[46]) <= 1e-9 * y[46] and out[24] != trace[3]
