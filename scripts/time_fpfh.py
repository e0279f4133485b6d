"""Time the global registration (csrc/cloud_fpfh.hip, csrc/feature_match.hip through scorp_amd/global_registration.py).
Per case a warm-up, then the median of --reps runs, a host clock around a call that ends in a synchronise:
  fpfh    compute_fpfh_feature of --points points sampled by sample_points_uniformly on a UV sphere (the timing fixture of
          scripts/time_cloud.py), radius 5 x the median nearest-neighbour spacing, max_nn 64.  The split into the search,
          SPFH and FPFH kernels comes from a run of its own under the profiler, folded in with --kernel-stats:
              rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/time_fpfh.py --cases fpfh --out /dev/null
              python scripts/time_fpfh.py --kernel-stats <dir>/.../*_kernel_stats.csv
  match   match_features at --match-sizes rows x as many (FPFH rows of two samplings of the sphere), with the achieved
          share of the float64 vector rate: ns nt 33 x 3 operations (subtract, multiply, add; contraction is off) over the
          call time and --peak-f64-tflops (78.6, AMD's published vector figure for the MI355X; a whole-call rate, which
          includes the merge kernel and the launch gaps, not a kernel's share of peak).
  route   get_FPFH_fitting_transformation against get_ICP_fitting_transformation_best with the rotations_64 table on one
          pair of --points points: the star-shaped surface of tests/fpfh_fixtures.py (a sphere has no pose to find) and
          5/7 of its points, jittered and moved by the fixture's 120-degree pose.  Pose errors against the truth are
          recorded next to the times.
Appends one JSON line per row to --out (profiles/fpfh_speed.jsonl).  No bar is set on any of these: they are records."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KERNELS = {"search": "fpfh_search_kernel", "spfh": "fpfh_spfh_kernel", "fpfh": "fpfh_feature_kernel"}


def fold_kernel_stats(path):
    """{search, spfh, fpfh, grid_setup: mean microseconds per call} from a rocprofv3 kernel-stats CSV"""
    rows = list(csv.DictReader(open(path)))
    out, calls = {k: 0.0 for k in list(KERNELS) + ["grid_setup"]}, 0
    for r in rows:
        name = r.get("Name") or r.get("KernelName") or ""
        total = float(r.get("TotalDurationNs") or r.get("TotalDuration(ns)") or 0.0)
        key = next((k for k, frag in KERNELS.items() if frag in name), None)
        if key == "search":
            calls = int(r.get("Calls") or 0)
        if key is None and ("icp_" in name or "cloud_gather" in name):
            key = "grid_setup"
        if key:
            out[key] += total
    if not calls:
        raise SystemExit(f"no {KERNELS['search']} in {path}")
    return {k: v / calls / 1e3 for k, v in out.items()}, calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["fpfh", "match", "route"], choices=["fpfh", "match", "route"])
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--match-sizes", type=int, nargs="+", default=[20_000, 100_000])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--route-reps", type=int, default=3)
    ap.add_argument("--peak-f64-tflops", type=float, default=78.6)
    ap.add_argument("--kernel-stats", help="fold a rocprofv3 kernel-stats CSV of a `--cases fpfh` run into one row and exit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fpfh_speed.jsonl"))
    a = ap.parse_args()

    def emit(row):
        print(json.dumps(row), flush=True)
        with open(a.out, "a") as out:
            out.write(json.dumps(row) + "\n")

    if a.kernel_stats:
        us, calls = fold_kernel_stats(a.kernel_stats)
        emit({"case": "fpfh_kernels", "points": a.points, "source": "rocprofv3 --kernel-trace --stats", "calls": calls,
              "mean_us_per_call": us})
        return
    import torch
    from scipy.spatial import cKDTree
    from scorp_amd import global_registration as gr
    from scorp_amd import icp
    from scorp_amd.mesh import Mesh, sample_points_uniformly
    from tests.mesh_simplify_reference import uv_sphere
    if not torch.cuda.is_available():
        raise SystemExit("time_fpfh.py needs a GPU")
    dev = torch.device("cuda:0")
    v, f = uv_sphere(64)
    mesh = Mesh(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), torch.zeros(len(v), 3, device=dev))

    def gpu_ms(fn, reps):
        ts = []
        for rep in range(reps + 1):   # (the first is the warm-up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep:
                ts.append((time.perf_counter() - t0) * 1e3)
        return {"ms": float(np.median(ts)), "ms_min": min(ts), "ms_max": max(ts), "reps": reps}

    def sphere(n, seed):
        P = sample_points_uniformly(mesh, n, seed=seed).points.contiguous()
        N = (P / P.norm(dim=1, keepdim=True)).contiguous()       # the sphere's own outward normals
        host = P.cpu().numpy().astype(np.float64)
        spacing = float(np.median(cKDTree(host).query(host[:: max(1, n // 20000)], k=2, workers=16)[0][:, 1]))
        return P, N, spacing

    if "fpfh" in a.cases:
        P, N, spacing = sphere(a.points, 1)
        radius = 5.0 * spacing
        _, _, deg, _ = gr.compute_fpfh_feature(P, N, radius, 64, return_neighbors=True)
        emit({"case": "fpfh", "points": a.points, "median_spacing": spacing, "radius": radius, "max_nn": 64,
              "mean_degree": float(deg.double().mean()), "full_lists": float((deg == 64).double().mean()),
              "gpu": gpu_ms(lambda: gr.compute_fpfh_feature(P, N, radius, 64), a.reps)})
    if "match" in a.cases:
        for n in a.match_sizes:
            feats = []
            for seed in (1, 2):
                P, N, spacing = sphere(n, seed)
                feats.append(gr.compute_fpfh_feature(P, N, 5.0 * spacing, 64).to(torch.float32).contiguous())
            t = gpu_ms(lambda: gr.match_features(feats[0], feats[1]), a.reps)
            ops = float(n) * n * 33 * 3
            emit({"case": "match_features", "source_rows": n, "target_rows": n, "split_rows": gr.match_split_rows(n, n), "gpu": t,
                  "float64_ops": ops, "tflops_whole_call": ops / (t["ms"] * 1e-3) / 1e12,
                  "share_of_f64_vector_peak": ops / (t["ms"] * 1e-3) / 1e12 / a.peak_f64_tflops, "peak_f64_tflops": a.peak_f64_tflops})
    if "route" in a.cases:
        from tests import fpfh_fixtures as fx
        from tests.fpfh_reference import pose_error
        n = a.points
        P64, _ = fx.surface_points(n, 3)
        rng = np.random.default_rng(11)
        subset = np.sort(rng.choice(n, n * 5 // 7, replace=False))
        truth = np.array(fx.registration_pair()["truth"])
        R, t = truth[:3, :3], truth[:3, 3]
        spacing = float(np.median(cKDTree(P64).query(P64[:: max(1, n // 20000)], k=2, workers=16)[0][:, 1]))
        orig = P64.astype(np.float32)
        refined = (((P64[subset] + rng.normal(0.0, 0.5 * spacing, (len(subset), 3))) - t) @ R).astype(np.float32)
        threshold = float(np.ptp(orig, axis=0).mean() * 0.16)      # the alignment scripts' ICP radius
        rot = np.load(os.path.join(ROOT, "tests", "golden", "rotations_64.npz"))["rotations"]
        results = {}
        routes = {"global": lambda: results.__setitem__("global", gr.get_FPFH_fitting_transformation(orig, refined, threshold)),
                  "sweep_rotations_64": lambda: results.__setitem__("sweep_rotations_64",
                                                                    icp.get_ICP_fitting_transformation_best(orig, refined, rot, threshold))}
        row = {"case": "route", "original_points": n, "refined_points": len(subset), "jitter": 0.5 * spacing, "threshold": threshold,
               "voxel_size": gr.default_voxel_size(orig)}
        for name, fn in routes.items():
            row[name] = gpu_ms(fn, a.route_reps)
            ang, dt = pose_error(results[name], truth)
            fit = float(icp.registration_icp(refined, orig, threshold, results[name], max_iteration=0).fitness[0])
            row[name].update({"rotation_error_deg": ang, "translation_error": dt, "icp_fitness": fit})
        row["sweep_over_global"] = row["sweep_rotations_64"]["ms"] / row["global"]["ms"]
        emit(row)


if __name__ == "__main__":
    main()
