"""Time the multi-start ICP (scorp_amd.icp) at the reference's size: a 100 k-point target, a 200 k-point source, the
67 inits of rotations_64.npz, max_iteration = 400, r = 0.16 x the mean bounding-box edge (the alignment script's
threshold).  Prints one JSON line: total ms per call (median of --reps after a warm-up call), iterations per init, and
the 16-thread scipy cKDTree correspondence pass of the yardstick on the same machine.  --estimation point_to_plane runs
the same fixture through scorp_icp_point_to_plane on normals estimated from the target (knn 30), and times that
estimation too.  --estimation generalized runs it through scorp_icp_generalized on covariances estimated from both
clouds (estimate_covariances: normals at knn 30, then the epsilon rule), timed apart in the same way.  --estimation colored
runs it through scorp_icp_colored on a smooth texture of position (tests/icp_color_fixtures.smooth_texture) as both clouds'
intensity, the target's estimated normals and its estimate_color_gradients (knn 30), timed apart too.  --gradient-sizes N ...
times scorp_color_gradients alone (stored neighbour lists, knn 30) on N surface points and exits.  The per-pass kernel
time comes from a run under `rocprofv3 --kernel-trace` (icp_pass_kernel / icp_solve_kernel, icp_plane_pass_kernel /
icp_plane_solve_kernel, icp_generalized_pass_kernel and icp_colored_pass_kernel with the plane solve: the thin kernels of csrc/icp.hip around its one
pass body and one solve body: the first launch has every init active, the last ones a single init):

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/time_icp.py --estimation E --reps 1 --scipy-passes 0
    python scripts/time_icp.py --estimation E --kernel-stats <dir>/.../*_kernel_stats.csv

The second command folds the pass, solve and set-up kernels of that run into one JSON line."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fold_kernel_stats(path):
    """{kernel: calls, total ms, mean / min / max microseconds} of the ICP kernels in a rocprofv3 kernel-stats CSV"""
    out = {}
    for r in csv.DictReader(open(path)):
        name = r.get("Name") or r.get("KernelName") or ""
        for frag in ("icp_pass_kernel", "icp_plane_pass_kernel", "icp_generalized_pass_kernel", "icp_colored_pass_kernel",
                     "icp_solve_kernel", "icp_plane_solve_kernel", "icp_normals_kernel", "icp_gather_covariances_kernel",
                     "icp_gather_intensity_kernel", "icp_color_gradients_kernel"):
            if frag in name:
                out[frag] = {"calls": int(r.get("Calls") or 0), "total_ms": float(r.get("TotalDurationNs") or 0.0) / 1e6,
                             "mean_us": float(r.get("AverageNs") or 0.0) / 1e3, "min_us": float(r.get("MinNs") or 0.0) / 1e3,
                             "max_us": float(r.get("MaxNs") or 0.0) / 1e3}
    if not out:
        raise SystemExit(f"no ICP kernel in {path}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--target", type=int, default=100_000)
    ap.add_argument("--source", type=int, default=200_000)
    ap.add_argument("--max-iteration", type=int, default=400)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scipy-passes", type=int, default=5, help="yardstick passes to time (0: skip)")
    ap.add_argument("--estimation", choices=["point_to_point", "point_to_plane", "generalized", "colored"],
                    default="point_to_point")
    ap.add_argument("--gradient-sizes", type=int, nargs="+", help="time scorp_color_gradients at these cloud sizes and exit")
    ap.add_argument("--kernel-stats", help="fold a rocprofv3 kernel-stats CSV of a run of this script into one line and exit")
    a = ap.parse_args()
    if a.kernel_stats:
        print(json.dumps({"estimation": a.estimation, "source": "rocprofv3 --kernel-trace --stats", "reps": a.reps,
                          "kernels": fold_kernel_stats(a.kernel_stats)}))
        return
    import torch
    from scipy.spatial import cKDTree
    from scorp_amd import icp
    from tests import icp_reference as ref
    from tests.icp_color_fixtures import smooth_texture

    def median_ms(f):
        ts = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    if a.gradient_sizes:
        for n in a.gradient_sizes:
            pts = ref.asymmetric_object(n, 1).astype(np.float32)
            P = torch.tensor(pts, device="cuda:0")
            I = icp.intensities(smooth_texture(pts))
            N, nb = icp.estimate_normals(P, knn=30, return_neighbors=True)
            icp.color_gradients(P, N, I, nb)   # warm-up
            print(json.dumps({"what": "scorp_color_gradients", "points": len(pts), "knn": 30, "reps": a.reps,
                              "color_gradients_ms": median_ms(lambda: icp.color_gradients(P, N, I, nb)),
                              "estimate_normals_with_neighbors_ms": median_ms(lambda: icp.estimate_normals(P, knn=30, return_neighbors=True))}),
                  flush=True)
        return

    rng = np.random.default_rng(0)
    tgt = ref.asymmetric_object(a.target, 1).astype(np.float32)
    R0 = ref.random_rotation(rng)
    obj = ref.asymmetric_object(a.source, 2)
    src = ((obj - 0.1) @ R0 + rng.normal(scale=0.002, size=obj.shape)).astype(np.float32)
    rots = np.load(os.path.join(ROOT, "tests", "golden", "rotations_64.npz"))["rotations"]
    inits = icp.icp_inits(rots, tgt.mean(axis=0), src.mean(axis=0))
    r = float(np.ptp(tgt, axis=0).mean() * 0.16)
    dev = torch.device("cuda:0")
    S, Q = torch.tensor(src, device=dev), torch.tensor(tgt, device=dev)
    kw = {}
    normals_ms = None
    if a.estimation == "point_to_plane":
        icp.estimate_normals(Q, knn=30)   # warm-up
        ts = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            N = icp.estimate_normals(Q, knn=30)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        normals_ms = float(np.median(ts))
        kw = {"estimation": "point_to_plane", "target_normals": N}
    covariances_ms = None
    if a.estimation == "generalized":
        icp.estimate_covariances(Q)   # warm-up
        ts = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            Cp, Cq = icp.estimate_covariances(S), icp.estimate_covariances(Q)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        covariances_ms = float(np.median(ts))
        kw = {"estimation": "generalized", "source_covariances": Cp, "target_covariances": Cq}
    gradients_ms = None
    if a.estimation == "colored":
        Ip, Iq = icp.intensities(smooth_texture(obj)), icp.intensities(smooth_texture(tgt))   # the source's: where it lies on the object
        N = icp.estimate_normals(Q, knn=30)
        icp.estimate_color_gradients(Q, Iq, normals=N)   # warm-up
        gradients_ms = median_ms(lambda: icp.estimate_color_gradients(Q, Iq, normals=N))
        kw = {"estimation": "colored", "source_colors": Ip, "target_colors": Iq, "target_normals": N,
              "target_gradients": icp.estimate_color_gradients(Q, Iq, normals=N)}
    res = icp.registration_icp(S, Q, r, inits, max_iteration=a.max_iteration, **kw)   # warm-up
    times = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = icp.registration_icp(S, Q, r, inits, max_iteration=a.max_iteration, **kw)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    it = np.sort(res.iterations)
    out = {"estimation": a.estimation, "target": len(tgt), "source": len(src), "inits": len(inits), "max_iteration": a.max_iteration, "r": r,
           "total_ms": float(np.median(times)), "total_ms_all": [round(t, 2) for t in times],
           "passes": int(res.iterations.max()) + 1, "iterations_per_init": res.iterations.tolist(),
           "iterations_median": float(np.median(it)), "iterations_max": int(it[-1]),
           "inits_at_max_iteration": int((it >= a.max_iteration).sum()), "best_fitness": float(res.fitness.max()),
           "best_rmse": float(res.inlier_rmse[int(np.argmax(res.fitness))])}
    if normals_ms is not None:
        out["estimate_normals_ms_knn30"] = normals_ms
    if covariances_ms is not None:
        out["estimate_covariances_ms_both_clouds_knn30"] = covariances_ms
    if gradients_ms is not None:
        out["estimate_color_gradients_ms_knn30"] = gradients_ms
    if a.scipy_passes > 0:
        tree = cKDTree(tgt.astype(np.float64))
        src64 = src.astype(np.float64)
        ts = []
        for j in range(a.scipy_passes):
            t0 = time.perf_counter()
            ref.correspondence_pass(tree, tgt.astype(np.float64), src64, inits[j], r, workers=16)
            ts.append((time.perf_counter() - t0) * 1e3)
        out["scipy_pass_ms_16_threads"] = float(np.median(ts))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
