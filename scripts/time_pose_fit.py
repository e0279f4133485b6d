"""Time the pose fit (scorp_amd.pose_fit) at the alignment scripts' size: 4 000 pairs, 2 000 RANSAC hypotheses, 3 000 Adam
steps.  For each routine: the GPU call (host clock around a synchronised call, median of --reps after a warm-up) next to
the yardstick's form of the reference pattern on the same machine - the numpy loop for RANSAC (BLAS / OpenMP threads as
the environment sets them; 16 for the numbers in DESIGN.md 4.11) and the torch loop with device="cuda" in fp32 for Adam.
Prints one JSON line.  The kernel times come from a run of their own:

    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/time_pose_fit.py --reps 1 --no-pattern
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, reps, sync):
    fn()   # warm-up
    times = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times)), [round(t, 3) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4000)
    ap.add_argument("--hypotheses", type=int, default=2000)
    ap.add_argument("--iterations", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-pattern", action="store_true", help="skip the reference-pattern loops")
    a = ap.parse_args()
    import torch
    from scorp_amd import pose_fit
    from tests import pose_fit_reference as ref

    rng = np.random.default_rng(0)
    n = a.pairs
    p = rng.uniform(-0.5, 0.5, (n, 3))
    Ro = ref.rotation_about((0.2, 0.9, -0.4), 25.0)
    M = ref.rotation_about((-0.6, 0.3, 0.7), 12.0) @ Ro.T @ np.diag([1.1, 0.9, 1.25]) @ Ro
    q = p @ M.T + (0.05, -0.03, 0.02) + rng.normal(scale=0.004, size=p.shape)
    out = rng.choice(n, int(0.3 * n), replace=False)
    q_ransac = q.copy()
    q_ransac[out] += rng.normal(scale=0.05, size=(len(out), 3))
    np.random.seed(0)
    triples = ref.draw_triples(n, a.hypotheses)
    dev = torch.device("cuda:0")
    P, Q, Qr = (torch.tensor(x, device=dev) for x in (p, q, q_ransac))
    sync = torch.cuda.synchronize
    res = {"pairs": n, "hypotheses": a.hypotheses, "iterations": a.iterations}
    res["ransac_gpu_ms"], res["ransac_gpu_ms_all"] = median_ms(lambda: pose_fit.ransac_fit(P, Qr, triples, 0.02), a.reps, sync)
    res["adam_gpu_ms"], res["adam_gpu_ms_all"] = median_ms(lambda: pose_fit.adam_fit_9dof(P, Q, iterations=a.iterations), a.reps, sync)
    fit = pose_fit.ransac_fit(P, Qr, triples, 0.02)
    res["ransac_winner"], res["ransac_count"] = fit.winner, fit.count
    if not a.no_pattern:
        t0 = time.perf_counter()
        y = ref.ransac_fit(p, q_ransac, triples, 0.02)
        res["ransac_pattern_ms"] = (time.perf_counter() - t0) * 1e3
        res["ransac_counts_equal"] = bool(np.array_equal(y["counts"], fit.counts))
        ref.adam_9dof(p, q, 20, device="cuda", dtype=torch.float32)   # warm-up
        sync()
        t0 = time.perf_counter()
        ref.adam_9dof(p, q, a.iterations, device="cuda", dtype=torch.float32)
        sync()
        res["adam_pattern_ms"] = (time.perf_counter() - t0) * 1e3
        res["ransac_ratio"] = res["ransac_pattern_ms"] / res["ransac_gpu_ms"]
        res["adam_ratio"] = res["adam_pattern_ms"] / res["adam_gpu_ms"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
