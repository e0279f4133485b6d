"""Time point_mesh_distance (csrc/mesh_distance.hip) on the fixture of scripts/time_mesh_simplify.py: the surface-nets mesh of
a unit sphere over a ground plane, extracted from an analytic distance grid of --resolutions^3 points over [-1.6, 1.6]^3.
The queries are --queries points sampled (sample_points_uniformly) from the MARCHING-CUBES mesh of the same volume.  Per
resolution the median of --reps runs after a warm-up, with the smallest and largest, set-up and query apart:
  setup   scorp_mesh_distance_build: bounding box, grid, the pair count (with its read-backs), count / scan / fill
  query   scorp_mesh_distance_query: the queries' Morton sort and the ring walk
  whole   point_mesh_distance (allocations and check_mesh's host reads included)
  sample  sample_points_uniformly of the queries (area prefix in torch + the sampling kernel)
  torch   the baseline: all (query, triangle) pairs by torch ops on the same GPU in float64 (plane projection, else the three
          segments), in chunks of --chunk-pairs, on q queries spread evenly over all of them; q doubles until a run takes more than --baseline-seconds,
          the rate of the last run is reported with the time it implies for all queries.  Its d^2 is compared with the kernel's.
With --metrics the first resolution also reports, in voxels, chamfer and Hausdorff distances of surface nets against
marching cubes and of the mesh against its simplify_vertex_clustering and simplify_quadric_decimation outputs.
Prints one JSON line per run and appends it to --out (default profiles/mesh_distance_speed.jsonl)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_all_pairs(torch, P, A, B, C, chunk_pairs):
    """min over the triangles of d^2 for every row of P: float64, [q, F] at a time"""
    F = A.shape[0]
    out = torch.empty(P.shape[0], dtype=torch.float64, device=P.device)
    n = torch.linalg.cross(B - A, C - A)
    nn = (n * n).sum(-1)

    def segment(p, a, b):
        e = b - a
        t = (((p - a) * e).sum(-1) / (e * e).sum(-1).clamp_min(1e-300)).clamp(0.0, 1.0)
        u = p - (a + t[..., None] * e)
        return (u * u).sum(-1)

    step = max(1, chunk_pairs // F)
    for s in range(0, P.shape[0], step):
        p = P[s:s + step, None, :]
        d = torch.minimum(torch.minimum(segment(p, A, B), segment(p, B, C)), segment(p, C, A))
        inside = (nn > 0) & ((torch.linalg.cross((B - A).expand(p.shape[0], F, 3), p - A) * n).sum(-1) >= 0) & \
            ((torch.linalg.cross((C - B).expand(p.shape[0], F, 3), p - B) * n).sum(-1) >= 0) & \
            ((torch.linalg.cross((A - C).expand(p.shape[0], F, 3), p - C) * n).sum(-1) >= 0)
        off = ((p - A) * n).sum(-1)
        d = torch.where(inside, off * off / nn.clamp_min(1e-300), d)
        out[s:s + step] = d.min(1)[0]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=int, nargs="+", default=[192, 384])
    ap.add_argument("--queries", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chunk-pairs", type=int, default=1 << 23)
    ap.add_argument("--baseline-seconds", type=float, default=2.0)
    ap.add_argument("--metrics", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_distance_speed.jsonl"))
    a = ap.parse_args()
    import torch
    from scorp_amd.mesh import (Mesh, extract_surface, mesh_distance, point_mesh_distance, sample_points_uniformly,
                                simplify_quadric_decimation, simplify_vertex_clustering)
    from scorp_amd.mesh.distance import _MeshGrid
    if not torch.cuda.is_available():
        raise SystemExit("time_mesh_distance.py needs a GPU")
    dev = torch.device("cuda:0")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    def stats(v):
        return {"ms": float(np.median(v)), "ms_min": min(v), "ms_max": max(v)}

    for k, N in enumerate(a.resolutions):
        c = torch.linspace(-1.6, 1.6, N, device=dev)
        x, y, z = torch.meshgrid(c, c, c, indexing="ij")
        grid = torch.minimum(torch.sqrt(x * x + y * y + (z - 0.1) ** 2) - 1.0, z + 0.7)
        del x, y, z
        meshes = {}
        for method in ("surface_nets", "marching_cubes"):
            v, f = extract_surface(grid, (c, c, c), method=method)
            meshes[method] = Mesh(v, f, torch.zeros_like(v))
        del grid
        nets, cubes = meshes["surface_nets"], meshes["marching_cubes"]
        voxel = 3.2 / (N - 1)
        times = {n: [] for n in ("setup", "query", "whole", "sample")}
        for rep in range(a.reps + 1):   # (the first is the warm-up)
            ts, samples = wall_ms(lambda: sample_points_uniformly(cubes, a.queries, seed=1))
            q = samples.points
            tb, g = wall_ms(lambda: _MeshGrid(nets.vertices, nets.faces, a.queries))
            tq, out = wall_ms(lambda: g.query(q, float("inf")))
            tw, whole = wall_ms(lambda: point_mesh_distance(q, nets))
            if rep:
                for n, t in zip(("setup", "query", "whole", "sample"), (tb, tq, tw, ts)):
                    times[n].append(t)
        row = {"resolution": N, "voxel": voxel, "num_faces": int(nets.faces.shape[0]), "num_vertices": int(nets.vertices.shape[0]),
               "queries": a.queries, "query_mesh_faces": int(cubes.faces.shape[0]), "reps": a.reps, "grid": g.header,
               "separate_calls_equal_whole": bool(torch.equal(out.squared_distance, whole.squared_distance) and torch.equal(out.face, whole.face)),
               "mean_distance_voxels": float(out.distance.mean()) / voxel, "max_distance_voxels": float(out.distance.max()) / voxel}
        row.update({n: stats(v) for n, v in times.items()})
        row["setup_share"] = row["setup"]["ms"] / (row["setup"]["ms"] + row["query"]["ms"])
        row["queries_per_second"] = a.queries / (row["query"]["ms"] * 1e-3)
        fl = nets.faces.long()
        A, B, C = (nets.vertices[fl[:, j]].double() for j in range(3))
        nq = 256
        while True:
            pick = torch.arange(nq, device=dev) * (a.queries // nq)
            tt, base = wall_ms(lambda: torch_all_pairs(torch, q[pick].double(), A, B, C, a.chunk_pairs))
            if tt > a.baseline_seconds * 1e3 or nq >= a.queries:
                break
            nq = min(2 * nq, a.queries)
        row["torch"] = {"queries": nq, "ms": tt, "pairs_per_second": nq * A.shape[0] / (tt * 1e-3),
                        "ms_implied_for_all_queries": tt * a.queries / nq,
                        "max_abs_d2_difference": float((base - out.squared_distance[pick]).abs().max()),
                        "max_d2": float(out.squared_distance[pick].max())}
        row["torch_over_setup_plus_query"] = row["torch"]["ms_implied_for_all_queries"] / (row["setup"]["ms"] + row["query"]["ms"])
        emit(row)
        if a.metrics and k == 0:
            pairs = {"surface_nets_vs_marching_cubes": (nets, cubes),
                     "vs_vertex_clustering_2_voxels": (nets, simplify_vertex_clustering(nets, 2.0 * voxel)),
                     "vs_quadric_decimation_to_a_tenth": (nets, simplify_quadric_decimation(nets, nets.faces.shape[0] // 10))}
            for name, (ma, mb) in pairs.items():
                tm, m = wall_ms(lambda: mesh_distance(ma, mb, samples=a.queries))
                emit({"resolution": N, "comparison": name, "faces_a": int(ma.faces.shape[0]), "faces_b": int(mb.faces.shape[0]),
                      "samples": a.queries, "ms": tm, "accuracy_voxels": m.accuracy / voxel, "completeness_voxels": m.completeness / voxel,
                      "chamfer_voxels": m.chamfer / voxel, "hausdorff_ab_voxels": m.hausdorff_ab / voxel,
                      "hausdorff_ba_voxels": m.hausdorff_ba / voxel})
        del meshes, nets, cubes


if __name__ == "__main__":
    main()
