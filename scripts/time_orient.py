"""Time the consistent orientation of normals (csrc/cloud_orient.hip through scorp_amd/global_registration.py).
Per size a warm-up, then the median of --reps runs, a host clock around a call that ends in a synchronise:
  orient  orient_normals_consistent_tangent_plane at --sizes points sampled by sample_points_uniformly on a UV sphere (the
          timing fixture of scripts/time_cloud.py), normals and the 12-column list from estimate_normals(knn=12) (made once,
          outside the clock), with the number of Boruvka rounds that found work (the device flags of the call's workspace,
          read back after it) out of the rounds launched.  For context, on the host: scipy's minimum_spanning_tree plus a
          breadth-first order over the same graph with the same weights (one thread: scipy's csgraph does not thread; the
          machine's 16 threads only serve numpy around it).  That is a context figure for the graph step alone - it takes
          no votes and writes no normals - not a competing implementation.
  The split into the centre, the four launches of the rounds and the finish comes from a run of its own under the profiler,
  folded in with --kernel-stats:
      rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python scripts/time_orient.py --sizes 1000000 --no-host --out /dev/null
      python scripts/time_orient.py --kernel-stats <dir>/.../*_kernel_stats.csv --sizes 1000000
Appends one JSON line per row to --out (profiles/orient_speed.jsonl).  No bar is set on any of these: they are records."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PHASES = {"init": ("orient_init_kernel",), "center": ("orient_center_partial_kernel", "orient_center_kernel"),
          "weight": ("orient_weight_kernel",), "edge": ("orient_edge_kernel",), "hook": ("orient_hook_kernel",),
          "compress": ("orient_compress_kernel",), "finish": ("orient_label_kernel", "orient_vote_kernel", "orient_output_kernel")}
MAX_ROUNDS = 32


def fold_kernel_stats(path):
    """({phase: mean microseconds per call}, calls) from a rocprofv3 kernel-stats CSV"""
    out, calls = {k: 0.0 for k in PHASES}, 0
    for r in csv.DictReader(open(path)):
        name = r.get("Name") or r.get("KernelName") or ""
        total = float(r.get("TotalDurationNs") or r.get("TotalDuration(ns)") or 0.0)
        for phase, frags in PHASES.items():
            if any(f in name for f in frags):
                out[phase] += total
                if phase == "init":
                    calls = int(r.get("Calls") or 0)
    if not calls:
        raise SystemExit(f"no orient_init_kernel in {path}")
    return {k: v / calls / 1e3 for k, v in out.items()}, calls


def work_offset(n):
    """Where the round flags lie in the call's workspace (OrientLayout of csrc/cloud_orient.hip: snap, par, the two slot
    arrays, low, votes, then the flags; every block 256-byte aligned)"""
    up = lambda v: (v + 255) // 256 * 256
    return 2 * up(n * 4) + 2 * up(n * 8) + 2 * up(n * 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10_000, 100_000, 1_000_000])
    ap.add_argument("--knn", type=int, default=12)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-host", action="store_true", help="skip the scipy context figure")
    ap.add_argument("--kernel-stats", help="fold a rocprofv3 kernel-stats CSV of a one-size run into one row and exit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orient_speed.jsonl"))
    a = ap.parse_args()

    def emit(row):
        print(json.dumps(row), flush=True)
        with open(a.out, "a") as out:
            out.write(json.dumps(row) + "\n")

    if a.kernel_stats:
        us, calls = fold_kernel_stats(a.kernel_stats)
        total = sum(us.values())
        emit({"case": "orient_kernels", "points": a.sizes[0], "knn": a.knn, "source": "rocprofv3 --kernel-trace --stats", "calls": calls,
              "mean_us_per_call": us, "share": {k: v / total for k, v in us.items()}})
        return
    import torch
    from scorp_amd import _C
    from scorp_amd import global_registration as gr
    from scorp_amd import icp
    from scorp_amd.mesh import Mesh, sample_points_uniformly
    from tests.mesh_simplify_reference import uv_sphere
    if not torch.cuda.is_available():
        raise SystemExit("time_orient.py needs a GPU")
    dev = torch.device("cuda:0")
    v, f = uv_sphere(64)
    mesh = Mesh(torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev), torch.zeros(len(v), 3, device=dev))

    def clock(fn, reps, sync):
        ts = []
        for rep in range(reps + 1):   # (the first is the warm-up)
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            if rep:
                ts.append((time.perf_counter() - t0) * 1e3)
        return {"ms": float(np.median(ts)), "ms_min": min(ts), "ms_max": max(ts), "reps": reps}

    for n in a.sizes:
        P = sample_points_uniformly(mesh, n, seed=1).points.contiguous()
        N, nb = icp.estimate_normals(P, knn=a.knn, return_neighbors=True)
        out, info = gr.orient_normals_consistent_tangent_plane(P, N, neighbors=nb, return_info=True)
        outward = float(((out * P).sum(1) > 0).double().mean())
        # the rounds that found work: one more call through the C ABI on a workspace of our own
        size = _C.lib().scorp_cloud_orient_workspace_bytes(n, a.knn)
        ws = torch.zeros(size, dtype=torch.uint8, device=dev)
        counts = torch.empty(2, dtype=torch.int32, device=dev)
        _C.call("scorp_cloud_orient_normals", P, N, nb, n, a.knn, None, 0, torch.empty_like(N), None, None, None, counts, ws, size)
        torch.cuda.synchronize()
        off = work_offset(n)
        flags = ws[off:off + 4 * MAX_ROUNDS].view(torch.int32).cpu().numpy()
        launched = int(np.ceil(np.log2(n))) + 1 if n > 1 else 1
        row = {"case": "orient", "points": n, "knn": a.knn, "components": info["n_components"], "tree_edges": int(info["tree"].shape[0]),
               "outward_fraction": outward, "rounds_with_work": int(flags.sum()), "rounds_launched": launched,
               "gpu": clock(lambda: gr.orient_normals_consistent_tangent_plane(P, N, neighbors=nb), a.reps, torch.cuda.synchronize)}
        if not a.no_host:
            from scipy.sparse import coo_matrix
            from scipy.sparse.csgraph import breadth_first_order, minimum_spanning_tree
            from tests import orient_reference as ref
            Nh, nbh = N.cpu().numpy(), nb.cpu().numpy()
            e = ref.edges(nbh, n)
            w = 1.0 - np.abs(ref.dot(Nh, e[:, 0], e[:, 1])) + 1.0            # (+ 1: scipy drops explicit zeros)
            graph = coo_matrix((w, (e[:, 0], e[:, 1])), shape=(n, n)).tocsr()

            def host():
                mst = minimum_spanning_tree(graph)
                breadth_first_order(mst, 0, directed=False)

            row["host_scipy_mst_bfs"] = clock(host, 3, lambda: None)
            row["host_over_gpu"] = row["host_scipy_mst_bfs"]["ms"] / row["gpu"]["ms"]
        emit(row)


if __name__ == "__main__":
    main()
