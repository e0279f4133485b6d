"""The pose fit without a GPU: the float64 yardstick (tests/pose_fit_reference.py) against the results recorded from the
reference's own functions (tests/golden/pose_fit.npz, made by tests/golden/make_pose_fit_golden.py), and the host side of
scorp_amd/pose_fit.py with the kernel call replaced by the yardstick."""
import os

import numpy as np
import pytest
import torch

from tests import pose_fit_reference as ref

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "pose_fit.npz")
ARRAYS = ("rotation", "translation", "scale", "rotation_orthogonal", "M")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


@pytest.fixture()
def pose_fit(monkeypatch):
    """scorp_amd.pose_fit with both kernel calls answered by the yardstick (the points stay on the CPU)."""
    from scorp_amd import pose_fit as m

    def run_ransac(P, Q, samples, threshold, min_inlier_ratio, method):
        r = ref.ransac_fit(P.cpu().numpy(), Q.cpu().numpy(), samples.cpu().numpy(), threshold, min_inlier_ratio, method)
        return m.RansacFit(r["R"], r["t"], r["s"], r["winner"], r["count"], r["counts"], r["mask"])

    def run_adam(P, Q, iterations, lr, lambda_reg_scale, lambda_reg_rot, scale_min, scale_max, init_scale, loss_every):
        run_adam.init_scale = np.array(init_scale)
        r = ref.adam_9dof(P.cpu().numpy(), Q.cpu().numpy(), iterations, lr, lambda_reg_scale, lambda_reg_rot, scale_max, scale_min,
                          [float(v) for v in init_scale], loss_every=loss_every)
        r["loss"] = 0.0
        return r

    monkeypatch.setattr(m, "_run_ransac", run_ransac)
    monkeypatch.setattr(m, "_run_adam", run_adam)
    monkeypatch.setattr(m, "_device", lambda *a: torch.device("cpu"))
    m.run_adam = run_adam
    return m


def test_fixture_has_the_margins_the_exact_checks_need(gold):
    for method in ("umeyama", "kabsch"):
        assert gold[f"{method}_gap"] >= 1e-10 and gold[f"{method}_cond"] >= 1e-6
    counts = gold["umeyama_counts"]
    assert gold["umeyama_winner"] == np.argmax(counts)
    assert gold["early_winner"] != gold["umeyama_winner"] and gold["early_winner"] + 1 < len(counts)
    for k in ARRAYS:   # the Adam run is a stable map of its input: two float64 runs on permuted pairs agree far below fp32 rounding
        assert gold[f"adam_f64_order_{k}"] <= 1e-9 < gold[f"adam_spread_{k}"]
    assert os.path.getsize(GOLDEN) < 300 * 1024


@pytest.mark.parametrize("case", ["umeyama", "kabsch", "early"])
def test_yardstick_reproduces_the_recorded_ransac(gold, case):
    method = "kabsch" if case == "kabsch" else "umeyama"
    ratio = float(gold["ransac_early_ratio"]) if case == "early" else -1.0
    r = ref.ransac_fit(gold["ransac_source"], gold["ransac_target"], gold["ransac_triples"], float(gold["ransac_threshold"]),
                       ratio, method)
    assert np.array_equal(r["counts"], gold[f"{method}_counts"])          # every hypothesis's count
    assert r["winner"] == gold[f"{case}_winner"]
    assert r["count"] == gold[f"{method}_counts"][r["winner"]] == r["mask"].sum()
    # two float64 LAPACK paths on the same data
    assert np.abs(r["R"] - gold[f"{case}_R"]).max() <= 1e-12
    assert np.abs(r["t"] - gold[f"{case}_t"]).max() <= 1e-12
    assert abs(r["s"] - gold[f"{case}_s"]) <= 1e-12


def test_yardstick_adam_reproduces_the_recorded_run(gold):
    """fp32, the reference's own precision: inside the recorded spread of the reference's result; float64: within 4x."""
    it = int(gold["adam_iterations"])
    f32 = ref.adam_9dof(gold["adam_source"], gold["adam_target"], it, dtype=torch.float32)
    f64 = ref.adam_9dof(gold["adam_source"], gold["adam_target"], it)
    for k in ARRAYS:
        spread = float(gold[f"adam_spread_{k}"])
        assert spread > 0.0
        d32 = np.abs(f32[k] - np.float64(gold[f"adam_{k}"])).max()
        d64 = np.abs(f64[k] - np.float64(gold[f"adam_{k}"])).max()
        print(f"{k}: spread {spread:.3g}, fp32 yardstick {d32:.3g}, float64 yardstick {d64:.3g}")
        assert d32 <= spread, k
        assert d64 <= 4 * spread, k


def _state_equal(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("case", ["umeyama", "kabsch", "early"])
def test_pc_align_ransac_draws_and_leaves_the_generator_as_the_loop_does(gold, pose_fit, monkeypatch, case):
    method = "kabsch" if case == "kabsch" else "umeyama"
    ratio = float(gold["ransac_early_ratio"]) if case == "early" else -1.0
    p, q, n_hyp = gold["ransac_source"], gold["ransac_target"], len(gold["ransac_triples"])
    seen = {}
    inner = pose_fit._run_ransac
    monkeypatch.setattr(pose_fit, "_run_ransac", lambda P, Q, samples, *a: seen.setdefault("s", samples.cpu().numpy()) is None or inner(P, Q, samples, *a))
    np.random.seed(0)
    R, t, s = pose_fit.pc_align_ransac(p, q, threshold=float(gold["ransac_threshold"]), max_iterations=n_hyp,
                                       min_inlier_ratio=ratio, method=method)
    after = np.random.get_state()
    assert np.array_equal(seen["s"], gold["ransac_triples"])     # np.random.choice's triples after the same seed
    np.random.seed(0)
    for _ in range(int(gold["early_winner"]) + 1 if case == "early" else n_hyp):   # the plain loop
        np.random.choice(len(p), 3, replace=False)
    assert _state_equal(after, np.random.get_state())
    assert isinstance(R, np.ndarray) and R.shape == (3, 3) and t.shape == (3,) and isinstance(s, float)
    assert np.abs(R - gold[f"{case}_R"]).max() <= 1e-12 and np.abs(t - gold[f"{case}_t"]).max() <= 1e-12
    assert abs(s - gold[f"{case}_s"]) <= 1e-12


def test_ransac_errors(pose_fit):
    p = np.random.default_rng(0).normal(size=(10, 3))
    with pytest.raises(ValueError, match="same length"):
        pose_fit.pc_align_ransac(p, p[:9])
    with pytest.raises(ValueError, match="At least 3 points"):
        pose_fit.pc_align_ransac(p[:2], p[:2])
    with pytest.raises(NotImplementedError):
        pose_fit.pc_align_ransac(p, p, method="umeyama_gen")
    with pytest.raises(NotImplementedError):
        pose_fit.ransac_fit(p, p, np.zeros((1, 3), np.int32), 0.1, method="umeyama_gen")
    with pytest.raises(ValueError):
        pose_fit.pc_align_ransac(p, p, method="procrustes")
    with pytest.raises(ValueError, match="No inliers found in RANSAC."):
        pose_fit.pc_align_ransac(p, p[::-1].copy(), threshold=1e-9, max_iterations=20)
    for bad in ([[0, 1, 10]], [[-1, 1, 2]], [[0, 1]], np.zeros((0, 3), np.int32)):
        with pytest.raises(ValueError):
            pose_fit.ransac_fit(p, p, np.asarray(bad), 0.1)
    with pytest.raises(ValueError):
        pose_fit.ransac_fit(p, p, np.zeros((1, 3), np.int32), float("nan"))


def test_adam_host_side(pose_fit):
    rng = np.random.default_rng(1)
    p = rng.normal(size=(50, 3))
    q = p * 1.1 + 0.02
    out = pose_fit.adam_algorithm_3d3d_9dof(p, q, iterations=5, verbose_interval=0)
    assert [a.shape for a in out] == [(3, 3), (3,), (3,), (3, 3)] and all(a.dtype == np.float32 for a in out)
    assert np.array_equal(pose_fit.run_adam.init_scale, [1.0, 1.0, 1.0])
    pose_fit.adam_algorithm_3d3d_9dof(p, q, iterations=1, verbose_interval=0, init_scale=[0.8, 1.0, 1.2])
    assert np.array_equal(pose_fit.run_adam.init_scale, [0.8, 1.0, 1.2])
    for outside in (2.0, [0.8, 1.0, 1.6], (0.7, 1.0, 1.0)):                  # one component outside: all three the mid-point
        pose_fit.adam_algorithm_3d3d_9dof(p, q, iterations=1, verbose_interval=0, init_scale=outside)
        assert np.array_equal(pose_fit.run_adam.init_scale, [1.125, 1.125, 1.125])
    for bad in (1, [1.0, 1.0], "1.0", np.ones((1, 3))):                       # (an int is refused there too)
        with pytest.raises(ValueError, match="init_scale"):
            pose_fit.adam_algorithm_3d3d_9dof(p, q, iterations=1, init_scale=bad)
    with pytest.raises(ValueError):
        pose_fit.adam_algorithm_3d3d_9dof(p, q, iterations=1_000_001)
    with pytest.raises(ValueError):
        pose_fit.adam_algorithm_3d3d_9dof(p, q, iterations=-1)
    with pytest.raises(ValueError):
        pose_fit.adam_algorithm_3d3d_9dof(p, q, iterations=1, device="cpu")
    with pytest.raises(ValueError):
        pose_fit.adam_algorithm_3d3d_9dof(p[:2], q[:2], iterations=1)


def test_adam_prints_the_loss_every_interval(pose_fit, capsys):
    p = np.random.default_rng(2).normal(size=(20, 3))
    pose_fit.adam_algorithm_3d3d_9dof(p, p, iterations=10, verbose_interval=5)
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("Iteration")]
    assert [l.split("|")[0].split()[1] for l in lines] == ["5", "10"]
