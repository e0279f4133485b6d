"""Time the triangle clustering (csrc/mesh_cluster.hip) and post_process_mesh on the surface-nets mesh of the scene
scripts/time_tsdf.py times: a unit sphere over a ground plane, ray-cast into --views ring cameras, fused over a
--resolution^3 lattice of the contracted space and meshed by extract_surface.  Per form the median of --reps runs after a
warm-up, with the smallest and largest:
  link / roots / stats   hipEvent pairs round each C-ABI call (the scan between the last two is torch.cumsum, timed apart);
  post_process_mesh      hipEvent pair round the whole call (clustering, threshold, compaction);
  numpy                  scorp_amd.mesh's own CPU form of the clustering on the same faces, host clock, --numpy-reps runs.
Prints one JSON line."""
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
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--numpy-reps", type=int, default=1)
    ap.add_argument("--cluster-to-keep", type=int, default=50)
    a = ap.parse_args()
    import torch
    from scorp_amd import _C
    from scorp_amd.mesh import Mesh, _cluster_numpy, cluster_connected_triangles, extract_surface, post_process_mesh, tsdf_fuse
    from scorp_amd.synthetic import ring_cameras
    from tests import tsdf_reference as ref
    if not torch.cuda.is_available():
        raise SystemExit("time_mesh_cluster.py needs a GPU")
    dev = torch.device("cuda:0")
    cams = ring_cameras(a.views, a.width, a.height, 7, radius=4.0)
    depth = torch.from_numpy(np.stack([ref.raycast_depth(c, size=(a.width, a.height)) for c in cams])).to(dev)
    fp = torch.stack([c.full_proj_transform for c in cams]).to(dev)
    N = a.resolution
    coords = tuple(torch.linspace(-1.2, 1.2, N, device=dev) for _ in range(3))
    grid = tsdf_fuse(depth, None, fp, coords, 2 * 4.0 / N, contracted=True, center=(0.0, 0.0, 0.0), radius=4.0)
    verts, faces = extract_surface(grid, coords)
    print(f"mesh: {verts.shape[0]} vertices, {faces.shape[0]} faces", file=sys.stderr, flush=True)
    del grid, depth
    F = faces.shape[0]
    colors = torch.rand(verts.shape[0], 3, device=dev)
    L = _C.lib()
    stream = _C.current_stream_ptr()
    slots = 1 << (6 * F - 1).bit_length()
    keys = torch.empty(slots, dtype=torch.int64, device=dev)
    owner = torch.empty(slots, dtype=torch.int32, device=dev)
    parent = torch.empty(F, dtype=torch.int32, device=dev)
    root = torch.empty(F, dtype=torch.int32, device=dev)
    is_root = torch.empty(F, dtype=torch.uint8, device=dev)
    cluster = torch.empty(F, dtype=torch.int32, device=dev)
    state = {}

    def link():
        _C.check(L.scorp_mesh_cluster_link(faces.data_ptr(), F, keys.data_ptr(), owner.data_ptr(), slots, parent.data_ptr(), stream), "link")

    def roots():
        _C.check(L.scorp_mesh_cluster_roots(parent.data_ptr(), F, root.data_ptr(), is_root.data_ptr(), stream), "roots")

    def scan():
        state["scan"] = torch.cumsum(is_root, 0, dtype=torch.int32)

    def stats():
        C = state["C"]
        state["counts"] = torch.empty(C, dtype=torch.int32, device=dev)
        state["area"] = torch.empty(C, dtype=torch.float64, device=dev)
        _C.check(L.scorp_mesh_cluster_stats(faces.data_ptr(), verts.data_ptr(), verts.shape[0], root.data_ptr(), state["scan"].data_ptr(),
                                            F, C, cluster.data_ptr(), state["counts"].data_ptr(), state["area"].data_ptr(), stream), "stats")

    def post():
        state["mesh"] = post_process_mesh(Mesh(verts, faces, colors), cluster_to_keep=a.cluster_to_keep)

    def event_ms(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    times = {k: [] for k in ("link", "roots", "scan", "stats", "post_process_mesh")}
    for rep in range(a.reps + 1):   # (the first is the warm-up)
        row = {"link": event_ms(link), "roots": event_ms(roots), "scan": event_ms(scan)}
        state["C"] = int(state["scan"][-1])
        row["stats"] = event_ms(stats)
        row["post_process_mesh"] = event_ms(post)
        if rep:
            for k, v in row.items():
                times[k].append(v)
    out = {"resolution": N, "views": a.views, "width": a.width, "height": a.height, "vertices": int(verts.shape[0]), "faces": F,
           "slots": slots, "clusters": state["C"], "largest_clusters": sorted(state["counts"].tolist())[-5:],
           "faces_after": int(state["mesh"].faces.shape[0]), "vertices_after": int(state["mesh"].vertices.shape[0]),
           "cluster_to_keep": a.cluster_to_keep, "reps": a.reps}
    for k, v in times.items():
        out[k] = {"ms": float(np.median(v)), "ms_min": min(v), "ms_max": max(v), "ms_all": [round(x, 4) for x in v]}
    print("kernels timed; the numpy form on the host", file=sys.stderr, flush=True)
    tc, counts, _ = cluster_connected_triangles(faces, verts)
    f_host, v_host = faces.cpu().numpy(), verts.cpu().numpy()
    ts = []
    for _ in range(a.numpy_reps):
        t0 = time.perf_counter()
        ntc, ncounts, _ = _cluster_numpy(f_host, v_host)
        ts.append((time.perf_counter() - t0) * 1e3)
    out["numpy"] = {"ms": float(np.median(ts)), "ms_all": [round(x, 1) for x in ts], "reps": a.numpy_reps,
                    "equal_to_kernels": bool(np.array_equal(ntc, tc.cpu().numpy()) and np.array_equal(ncounts, counts.cpu().numpy()))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
