"""Time the cloud cleaning (csrc/cloud_filter.hip through scorp_amd/cloud.py) against the host's tree searches on a
surface-like cloud: --sizes points sampled by sample_points_uniformly on a UV sphere (tests/mesh_simplify_reference.py).
The radius of the count and of DBSCAN is 3 x the median nearest-neighbour spacing, the voxel size the same.  Per case a
warm-up, then the median of --reps runs with a synchronisation round each:
  knn_mean_distance (k = 20)   against scipy's cKDTree.query(k = 20, workers = --workers);
  radius_neighbor_count        against cKDTree.query_ball_point(return_length=True, workers = --workers);
  cluster_dbscan (min_points 10) against scikit-learn's DBSCAN(n_jobs = --workers), one run; a size is skipped, and the row
                               says so, when the size before it took longer than --dbscan-host-budget / 10 seconds (ten
                               times the points would not finish within the budget);
  voxel_down_sample            no host baseline.
Appends one JSON line per case and size to --out (profiles/cloud_filter_speed.jsonl)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--dbscan-host-budget", type=float, default=60.0, help="seconds one host DBSCAN run may be expected to take")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_filter_speed.jsonl"))
    a = ap.parse_args()
    import torch
    from scipy.spatial import cKDTree
    from scorp_amd import cloud
    from scorp_amd.mesh import Mesh, sample_points_uniformly
    from tests.mesh_simplify_reference import uv_sphere
    if not torch.cuda.is_available():
        raise SystemExit("time_cloud.py needs a GPU")
    dev = torch.device("cuda:0")
    v, f = uv_sphere(64)
    mesh = Mesh(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), torch.zeros(len(v), 3, device=dev))

    def gpu_ms(fn):
        ts = []
        for rep in range(a.reps + 1):   # (the first is the warm-up)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep:
                ts.append((time.perf_counter() - t0) * 1e3)
        return {"ms": float(np.median(ts)), "ms_min": min(ts), "ms_max": max(ts), "reps": a.reps}

    def host_ms(fn, reps):
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"ms": float(np.median(ts)), "ms_min": min(ts), "ms_max": max(ts), "reps": reps, "workers": a.workers}

    dbscan_host_s = dbscan_host_n = None   # the last host DBSCAN run: seconds, points
    with open(a.out, "a") as out:
        for n in sorted(a.sizes):
            P = sample_points_uniformly(mesh, n, seed=1).points.contiguous()
            host = P.cpu().numpy().astype(np.float64)
            tree = cKDTree(host)
            spacing = float(np.median(tree.query(host[:: max(1, n // 20000)], k=2, workers=a.workers)[0][:, 1]))
            radius = 3.0 * spacing
            cases = {
                "knn_mean_distance": (lambda: cloud.knn_mean_distance(P, 20), lambda: tree.query(host, k=20, workers=a.workers)),
                "radius_neighbor_count": (lambda: cloud.radius_neighbor_count(P, radius),
                                          lambda: tree.query_ball_point(host, radius, return_length=True, workers=a.workers)),
                "cluster_dbscan": (lambda: cloud.cluster_dbscan(P, radius, 10), None),
                "voxel_down_sample": (lambda: cloud.voxel_down_sample(P, radius), None),
            }
            if dbscan_host_s is None or dbscan_host_s * (n / dbscan_host_n) <= a.dbscan_host_budget:
                from sklearn.cluster import DBSCAN
                cases["cluster_dbscan"] = (cases["cluster_dbscan"][0], lambda: DBSCAN(eps=radius, min_samples=10, n_jobs=a.workers).fit(host))
            for name, (gpu, cpu) in cases.items():
                row = {"case": name, "points": n, "median_spacing": spacing, "radius": radius, "gpu": gpu_ms(gpu)}
                if name == "radius_neighbor_count":
                    row["mean_count"] = float(cloud.radius_neighbor_count(P, radius).double().mean())
                if name == "cluster_dbscan":
                    row["clusters"] = int(cloud.cluster_dbscan(P, radius, 10).max()) + 1
                if name == "voxel_down_sample":
                    row["cells"] = int(cloud.voxel_down_sample(P, radius).shape[0])
                if cpu is not None and not a.no_host:
                    row["host"] = host_ms(cpu, a.host_reps if name != "cluster_dbscan" else 1)
                    row["host_over_gpu"] = row["host"]["ms"] / row["gpu"]["ms"]
                    if name == "cluster_dbscan":
                        dbscan_host_s, dbscan_host_n = row["host"]["ms"] / 1e3, n
                elif name == "cluster_dbscan" and not a.no_host:
                    row["host"] = f"skipped: {dbscan_host_n} points took {dbscan_host_s:.1f} s"
                print(json.dumps(row), flush=True)
                out.write(json.dumps(row) + "\n")
                out.flush()


if __name__ == "__main__":
    main()
