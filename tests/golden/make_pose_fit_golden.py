"""Generate tests/golden/pose_fit.npz by CALLING the reference's pose-fit functions (utils/solution.py: pc_align_ransac,
umeyama_algorithm_np, kabsch_algorithm_np, compute_residuals, adam_algorithm_3d3d_9dof) on synthetic pair sets.

Run where the reference tree is, with it on the path (about a minute, CPU only):
    PYTHONPATH=<reference root> python tests/golden/make_pose_fit_golden.py
Only inputs and recorded results are stored; no reference source text is copied.

RANSAC cases (1 500 pairs of unit extent, a planted similarity: 12 degrees, scale 1.15, 4 mm noise, 30 % gross outliers,
threshold 0.02, np.random.seed(0), 2 000 triples): the pairs, the triples, every hypothesis's inlier count, the winner and
pc_align_ransac's (R, t, s) for method umeyama, for kabsch, and for umeyama with a min_inlier_ratio at which the early exit
fires.  The data seed is the first from 7 on for which the early exit picks another hypothesis than the full run, no
(hypothesis, pair) residual lies within 1e-10 of the threshold and every triple's covariance has s2 / s1 >= 1e-6: then
float64 rounding (1e-15) cannot move a count, and "every count equal" is a fair demand on another float64 implementation.
Adam case: pairs from an anisotropic map (s = (1.1, 0.9, 1.25) in a rotated frame, a 12 degree rotation, 2 mm noise),
adam_algorithm_3d3d_9dof(iterations=3000, device="cpu") on them and on three fixed permutations of them.  A permutation
changes only the fp32 summation order, so the largest distance between any two of the four results is the reference's own
rounding spread; it is recorded per returned array and for M = R Ro^T diag(s) Ro.  That reading holds only while the 3 000
steps are a stable map of their input.  They need not be: late in a run, with the gradients small and Adam's second
moments decaying, a trajectory can magnify a 1e-16 difference to 1e-4 within a few hundred steps (data seed 11 does: two
float64 yardstick runs on permuted pairs end 1e-4 apart in Ro), and then no spread of four samples describes it.  So, as
for the RANSAC margins, the data seed is the first from 11 on for which two FLOAT64 yardstick runs on permuted pairs agree
to 1e-9 in every array (a hundredth of an fp32 ulp of a unit entry; a stable run gives 1e-10 or less); the criterion uses
the yardstick alone.  The recorded order sensitivity is stored beside the spread."""
import contextlib
import io
import os
import sys

import numpy as np

from utils.solution import (adam_algorithm_3d3d_9dof, compute_residuals, kabsch_algorithm_np, pc_align_ransac,  # noqa: E402
                            umeyama_algorithm_np)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests.pose_fit_reference import adam_9dof, compose, rotation_about  # noqa: E402

N, N_HYP, THRESHOLD, EARLY_RATIO = 1500, 2000, 0.02, 0.6
SOLVERS = {"umeyama": umeyama_algorithm_np, "kabsch": kabsch_algorithm_np}


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def ransac_data(seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.5, 0.5, (N, 3))
    R = rotation_about((0.3, -0.5, 0.8), 12.0)
    q = 1.15 * p @ R.T + (0.3, -0.2, 0.1) + rng.normal(scale=0.004, size=p.shape)
    out = rng.choice(N, int(0.3 * N), replace=False)
    q[out] += rng.normal(scale=0.05, size=(len(out), 3))   # gross: 12 noise sigmas, a few land inside the threshold by chance
    return p, q


def hypotheses(p, q, triples, method):
    """Per hypothesis, from the reference's own solver and residual: (count, smallest |residual - threshold|, s2 / s1)."""
    counts, gap, cond = np.zeros(len(triples), np.int32), np.inf, np.inf
    for h, idx in enumerate(triples):
        R, t, s = SOLVERS[method](p[idx], q[idx])
        r = compute_residuals(p, q, R, t, s)
        counts[h] = (r < THRESHOLD).sum()
        gap = min(gap, float(np.abs(r - THRESHOLD).min()))
        pc, qc = p[idx] - p[idx].mean(0), q[idx] - q[idx].mean(0)
        sv = np.linalg.svd(pc.T @ qc, compute_uv=False)
        cond = min(cond, float(sv[1] / sv[0]))
    return counts, gap, cond


def draws_consumed(state_before, state_after, limit):
    """How many np.random.choice(N, 3, replace=False) calls lead from one generator state to the other."""
    keep = np.random.get_state()
    np.random.set_state(state_before)
    for k in range(limit + 1):
        s = np.random.get_state()
        if s[2] == state_after[2] and np.array_equal(s[1], state_after[1]):
            np.random.set_state(keep)
            return k
        np.random.choice(N, 3, replace=False)
    raise AssertionError("generator state not reached")


def ransac_cases():
    for seed in range(7, 64):
        p, q = ransac_data(seed)
        np.random.seed(0)
        triples = np.stack([np.random.choice(N, 3, replace=False) for _ in range(N_HYP)]).astype(np.int32)
        out = {"ransac_source": p, "ransac_target": q, "ransac_triples": triples, "ransac_threshold": THRESHOLD,
               "ransac_data_seed": seed, "ransac_early_ratio": EARLY_RATIO}
        ok = True
        for method in SOLVERS:
            counts, gap, cond = hypotheses(p, q, triples, method)
            if gap < 1e-10 or cond < 1e-6:
                ok = False
                break
            out[f"{method}_counts"], out[f"{method}_gap"], out[f"{method}_cond"] = counts, gap, cond
            out[f"{method}_winner"] = int(np.argmax(counts))
            np.random.seed(0)
            before = np.random.get_state()
            R, t, s = quiet(pc_align_ransac, p, q, threshold=THRESHOLD, max_iterations=N_HYP, method=method)
            assert draws_consumed(before, np.random.get_state(), N_HYP) == N_HYP
            out[f"{method}_R"], out[f"{method}_t"], out[f"{method}_s"] = R, t, float(s)
        if not ok:
            continue
        counts = out["umeyama_counts"]
        over = np.nonzero(counts > EARLY_RATIO * N)[0]
        if not (len(over) and counts[over[0]] < counts.max()):
            continue   # the early exit must fire, and on a hypothesis that is not the full run's winner
        np.random.seed(0)
        before = np.random.get_state()
        R, t, s = quiet(pc_align_ransac, p, q, threshold=THRESHOLD, max_iterations=N_HYP, min_inlier_ratio=EARLY_RATIO)
        assert draws_consumed(before, np.random.get_state(), N_HYP) == over[0] + 1
        out["early_winner"], out["early_R"], out["early_t"], out["early_s"] = int(over[0]), R, t, float(s)
        print(f"ransac: data seed {seed}, top count {counts.max()} at {np.nonzero(counts == counts.max())[0]}, gap "
              f"{out['umeyama_gap']:.3g} / {out['kabsch_gap']:.3g}, s2/s1 {out['umeyama_cond']:.3g}, early exit at {over[0]}")
        return out
    raise AssertionError("no data seed gave the margins")


def adam_data(seed, n=1500):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.5, 0.5, (n, 3))
    Ro = rotation_about((0.2, 0.9, -0.4), 25.0)
    M = rotation_about((-0.6, 0.3, 0.7), 12.0) @ Ro.T @ np.diag([1.1, 0.9, 1.25]) @ Ro
    q = p @ M.T + (0.05, -0.03, 0.02) + rng.normal(scale=0.002, size=p.shape)
    return p.astype(np.float32), q.astype(np.float32)


def adam_case():
    n, iterations = 1500, 3000
    perms = np.stack([np.random.default_rng(100 + k).permutation(n) for k in range(3)]).astype(np.int32)
    names = ("rotation", "translation", "scale", "rotation_orthogonal")
    for seed in range(11, 64):
        p, q = adam_data(seed, n)
        a, b = adam_9dof(p, q, iterations), adam_9dof(p[perms[0]], q[perms[0]], iterations)
        sens = {k: float(np.abs(a[k] - b[k]).max()) for k in names + ("M",)}
        print(f"adam: data seed {seed}: float64 order sensitivity {max(sens.values()):.3g}")
        if max(sens.values()) <= 1e-9:
            break
    else:
        raise AssertionError("no data seed gave a stable run")
    runs = []
    for order in [np.arange(n)] + list(perms):
        res = adam_algorithm_3d3d_9dof(p[order], q[order], iterations=iterations, verbose_interval=0, device="cpu")
        run = dict(zip(names, res))
        run["M"] = compose(run["rotation"], run["scale"], run["rotation_orthogonal"])
        runs.append(run)
    out = {"adam_source": p, "adam_target": q, "adam_perms": perms, "adam_iterations": iterations, "adam_data_seed": seed}
    for k in names + ("M",):
        out[f"adam_{k}"] = runs[0][k]
        out[f"adam_spread_{k}"] = max(float(np.abs(np.float64(a[k]) - np.float64(b[k])).max()) for a in runs for b in runs)
        out[f"adam_f64_order_{k}"] = sens[k]
        print(f"adam: spread of {k}: {out[f'adam_spread_{k}']:.3g}")
    return out


if __name__ == "__main__":
    data = ransac_cases()
    data.update(adam_case())
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pose_fit.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")
