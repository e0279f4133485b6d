"""The pose fit on the GPU (scorp_pose_ransac, scorp_pose_adam_9dof; scorp_amd/pose_fit.py) against the results recorded
from the reference's own functions (tests/golden/pose_fit.npz) and the float64 yardstick tests/pose_fit_reference.py.

Distances measured on an MI355X (printed by the tests; DESIGN.md 4.11 holds them too):
  RANSAC, kernel to recorded reference: every count, winner and mask equal; |dR|, |dt|, |ds| <= 1.2e-15 (bound 1e-9).
  Adam, kernel to recorded fp32 reference (bound 4x the recorded spread): rotation 4.1e-7 (5.0e-6), translation 3.3e-7
  (4.2e-6), scale 3.5e-5 (4.4e-4), rotation_orthogonal 1.8e-6 (3.0e-5), M 3.0e-5 (3.8e-4).
  Adam, kernel to float64 yardstick (bound 10x the yardstick's own order sensitivity): rotation 6.9e-16 (6.1e-15),
  translation 5.9e-16 (5.3e-15), scale 6.2e-14 (5.5e-13), rotation_orthogonal 3.9e-15 (3.7e-14), M 5.3e-14 (4.7e-13)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import pose_fit_reference as ref

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "pose_fit.npz")
ARRAYS = ("rotation", "translation", "scale", "rotation_orthogonal", "M")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def pf():
    from scorp_amd import pose_fit as m
    return m


def _case(gold, case):
    method = "kabsch" if case == "kabsch" else "umeyama"
    ratio = float(gold["ransac_early_ratio"]) if case == "early" else -1.0
    return method, ratio


@pytest.mark.parametrize("case", ["umeyama", "kabsch", "early"])
def test_ransac_matches_the_recorded_reference(pf, gold, case):
    method, ratio = _case(gold, case)
    p, q, thr = gold["ransac_source"], gold["ransac_target"], float(gold["ransac_threshold"])
    fit = pf.ransac_fit(p, q, gold["ransac_triples"], thr, ratio, method)
    assert np.array_equal(fit.counts, gold[f"{method}_counts"])          # ALL 2 000 counts
    assert fit.winner == gold[f"{case}_winner"]                            # the first maximum / the first above the ratio
    assert fit.count == gold[f"{method}_counts"][fit.winner]
    R, t, s = ref.similarity_fit(p[gold["ransac_triples"][fit.winner]], q[gold["ransac_triples"][fit.winner]], method)
    assert np.array_equal(fit.mask, ref.residuals(p, q, R, t, s) < thr)
    assert fit.mask.sum() == fit.count
    dR, dt, ds = np.abs(fit.R - gold[f"{case}_R"]).max(), np.abs(fit.t - gold[f"{case}_t"]).max(), abs(fit.s - gold[f"{case}_s"])
    print(f"{case}: |dR| {dR:.3g} |dt| {dt:.3g} |ds| {ds:.3g}")
    assert dR <= 1e-9 and dt <= 1e-9 and ds <= 1e-9


def test_ransac_is_deterministic_and_batch_independent(pf, gold):
    p, q, thr, tri = gold["ransac_source"], gold["ransac_target"], float(gold["ransac_threshold"]), gold["ransac_triples"]
    a = pf.ransac_fit(p, q, tri, thr)
    b = pf.ransac_fit(p, q, tri, thr)
    for f in ("R", "t", "counts", "mask"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert a.s == b.s and a.winner == b.winner and a.count == b.count
    for h in (0, int(a.winner), 1999):
        one = pf.ransac_fit(p, q, tri[h:h + 1], thr)
        assert one.counts[0] == a.counts[h]
    alone = pf.ransac_fit(p, q, tri[a.winner:a.winner + 1], thr)
    assert np.array_equal(alone.R, a.R) and np.array_equal(alone.t, a.t) and alone.s == a.s and np.array_equal(alone.mask, a.mask)


@pytest.mark.parametrize("case", ["umeyama", "early"])
def test_pc_align_ransac_after_a_seed(pf, gold, case):
    method, ratio = _case(gold, case)
    p, q, thr, n_hyp = gold["ransac_source"], gold["ransac_target"], float(gold["ransac_threshold"]), len(gold["ransac_triples"])
    np.random.seed(0)
    R, t, s = pf.pc_align_ransac(p, q, threshold=thr, max_iterations=n_hyp, min_inlier_ratio=ratio, method=method)
    after = np.random.get_state()
    assert np.abs(R - gold[f"{case}_R"]).max() <= 1e-9 and np.abs(t - gold[f"{case}_t"]).max() <= 1e-9
    assert abs(s - gold[f"{case}_s"]) <= 1e-9
    np.random.seed(0)
    ref.pc_align_ransac(p, q, threshold=thr, max_iterations=n_hyp, min_inlier_ratio=ratio, method=method)   # the yardstick loop
    mine = np.random.get_state()
    assert after[0] == mine[0] and np.array_equal(after[1], mine[1]) and after[2:] == mine[2:]


def test_adam_matches_the_recorded_reference_and_the_yardstick(pf, gold):
    p, q, it = gold["adam_source"], gold["adam_target"], int(gold["adam_iterations"])
    got = pf.adam_fit_9dof(p, q, iterations=it)
    got["M"] = ref.compose(got["rotation"], got["scale"], got["rotation_orthogonal"])
    # the yardstick's own sensitivity to the order of the pairs, measured from the yardstick alone
    y0 = ref.adam_9dof(p, q, it)
    order = gold["adam_perms"][0]
    y1 = ref.adam_9dof(p[order], q[order], it)
    f32 = pf.adam_algorithm_3d3d_9dof(p, q, iterations=it, verbose_interval=0)
    assert all(a.dtype == np.float32 for a in f32)
    for k in ARRAYS:
        spread = float(gold[f"adam_spread_{k}"])
        d_ref = np.abs(got[k] - np.float64(gold[f"adam_{k}"])).max()
        own = np.abs(y0[k] - y1[k]).max()
        d_y = np.abs(got[k] - y0[k]).max()
        print(f"{k}: to the reference {d_ref:.3g} (4x spread {4 * spread:.3g}); to the yardstick {d_y:.3g} (10x its own {10 * own:.3g})")
    for k in ARRAYS:
        spread = float(gold[f"adam_spread_{k}"])
        assert np.abs(got[k] - np.float64(gold[f"adam_{k}"])).max() <= 4 * spread, k
        assert np.abs(got[k] - y0[k]).max() <= 10 * np.abs(y0[k] - y1[k]).max(), k
    for a, k in zip(f32, ARRAYS):
        assert np.array_equal(a, got[k].astype(np.float32))
    again = pf.adam_fit_9dof(p, q, iterations=it)
    for k in ARRAYS[:4]:
        assert np.array_equal(again[k], got[k]), k


def test_adam_loss_trace(pf, gold):
    p, q = gold["adam_source"], gold["adam_target"]
    got = pf.adam_fit_9dof(p, q, iterations=200, loss_every=50)
    y = ref.adam_9dof(p, q, 200, loss_every=50)
    assert got["losses"].shape == (4,)
    np.testing.assert_allclose(got["losses"], y["losses"], rtol=1e-9)
    for k in ARRAYS[:4]:   # two float64 statements of one formula; Adam's m / sqrt(v) magnifies rounding where a gradient is ~0 (qo)
        np.testing.assert_allclose(got[k], y[k], atol=1e-6)


def test_planted_pose_is_recovered_by_both_routes(pf):
    rng = np.random.default_rng(5)
    p = rng.normal(size=(1000, 3)) * 0.3
    R0, t0 = ref.rotation_about((0.2, 0.5, -0.8), 20.0), np.array([0.3, -0.11, 0.2])
    np.random.seed(1)
    R, t, s = pf.pc_align_ransac(p, 1.2 * p @ R0.T + t0, threshold=1e-6, max_iterations=50)
    assert np.abs(R - R0).max() < 1e-9 and np.abs(t - t0).max() < 1e-9 and abs(s - 1.2) < 1e-9
    R, t, s = pf.pc_align_ransac(p, p @ R0.T + t0, threshold=1e-6, max_iterations=50, method="kabsch")
    assert np.abs(R - R0).max() < 1e-9 and np.abs(t - t0).max() < 1e-9 and s == 1.0
    # the anisotropic route: M = R0 Ro^T diag(s) Ro, recovered as a product (Ro and s alone are not unique)
    Ro = ref.rotation_about((0.7, 0.1, 0.4), 30.0)
    M0 = R0 @ Ro.T @ np.diag([1.2, 0.8, 1.4]) @ Ro
    out = pf.adam_fit_9dof(p, p @ M0.T + t0, iterations=6000, lr=2e-3, lambda_reg_scale=0.0, lambda_reg_rot=0.0)
    M = ref.compose(out["rotation"], out["scale"], out["rotation_orthogonal"])
    assert np.abs(M - M0).max() < 1e-4 and np.abs(out["translation"] - t0).max() < 1e-4
    assert np.abs(np.sort(out["scale"]) - [0.8, 1.2, 1.4]).max() < 1e-4


def test_invalid_arguments(pf, gold):
    from scorp_amd import _C
    L = _C.lib()
    dev = torch.device("cuda:0")
    p = torch.zeros(8, 3, dtype=torch.float64, device=dev)
    tri = torch.tensor([[0, 1, 2]], dtype=torch.int32, device=dev)
    out = torch.zeros(64, dtype=torch.float64, device=dev)
    cnt = torch.full((4,), -7, dtype=torch.int32, device=dev)
    mask = torch.zeros(8, dtype=torch.uint8, device=dev)
    need = int(L.scorp_pose_fit_workspace_bytes(8, 1))
    ws = torch.empty(need + 512, dtype=torch.uint8, device=dev)
    wp = (ws.data_ptr() + 255) // 256 * 256
    f64 = ctypes.c_double

    def ransac(n=8, samples=tri.data_ptr(), nh=1, thr=0.1, method=0, src=p.data_ptr(), w=wp, wb=need):
        return L.scorp_pose_ransac(src, p.data_ptr(), n, samples, nh, f64(thr), f64(-1.0), method, out.data_ptr(), out.data_ptr() + 128,
                                   out.data_ptr() + 256, cnt.data_ptr() + 8, cnt.data_ptr(), mask.data_ptr(), w, wb, None)

    for kw in (dict(n=2), dict(thr=float("nan")), dict(thr=float("inf")), dict(src=None), dict(samples=None), dict(w=None),
               dict(wb=need - 1), dict(w=wp + 8), dict(nh=0), dict(nh=65536), dict(method=2)):
        assert ransac(**kw) == _C.ERR_INVALID, kw
    torch.cuda.synchronize()
    assert int(cnt[0]) == -7                                              # nothing was launched
    bad = torch.tensor([[0, 1, 8]], dtype=torch.int32, device=dev)
    assert ransac(samples=bad.data_ptr()) == _C.ERR_INVALID               # found by the fit kernel, which reads nothing for it
    assert b"sample index" in L.scorp_last_error()
    assert ransac() == _C.ERR_NO_INLIERS                                  # all-zero pairs: a valid call, a NaN scale, no inlier
    s0 = (ctypes.c_double * 3)(1.0, 1.0, 1.0)

    def adam(n=8, it=10, smin=0.75, smax=1.5, init=s0, w=wp, wb=need, lr=1e-3):
        return L.scorp_pose_adam_9dof(p.data_ptr(), p.data_ptr(), n, it, f64(lr), f64(0.0), f64(0.0), f64(smin), f64(smax), init,
                                      out.data_ptr(), None, 0, 0, w, wb, None)

    out.fill_(-3.0)
    for kw in (dict(n=2), dict(it=-1), dict(it=1_000_001), dict(smin=1.5), dict(init=None), dict(w=None), dict(wb=need - 1),
               dict(w=wp + 8), dict(lr=float("nan"))):
        assert adam(**kw) == _C.ERR_INVALID, kw
    torch.cuda.synchronize()
    assert float(out[0]) == -3.0
    x = gold["ransac_source"]
    with pytest.raises(ValueError, match="No inliers found in RANSAC."):
        pf.ransac_fit(x, x[::-1].copy(), gold["ransac_triples"][:10], 1e-9)
    with pytest.raises(ValueError):
        pf.adam_fit_9dof(x, x, iterations=1_000_001)
    with pytest.raises(NotImplementedError):
        pf.pc_align_ransac(x, x, method="umeyama_gen")
