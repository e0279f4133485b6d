"""Time the mesh smoothing and the normals (csrc/mesh_smooth.hip, scorp_amd/mesh/smooth.py) on the meshes scripts/time_mesh_render.py
renders: --surfels opaque surfels on a unit sphere, --views ring cameras at --width x --height, GaussianExtractor.reconstruction
-> extract_mesh_bounded at its default voxel size (depth_trunc 6), and that mesh after simplify_vertex_clustering with cells of
--cluster-voxel.  After a warm-up, the median of --reps runs with the smallest and largest, timed by torch.cuda.Event pairs
round the whole Python call (check_mesh's host reads and the allocations included) unless said otherwise.  One line per mesh:
  mesh_adjacency                         the sorts and scans that build both CSRs and the boundary flags
  face_normals, vertex_normals           the latter with the adjacency reused
  half_step_call                         scorp_mesh_smooth alone, one uniform half-step into a buffer that exists
  filter_smooth_laplacian_1              one uniform half-step through Python, the adjacency reused
  filter_smooth_taubin_10 / _reused      ten iterations (twenty half-steps), the adjacency built inside / reused
  index_add_half_step                    what a user would write without this: float32 index_add_ over the directed edge list
                                         (built beforehand), one uniform half-step - float atomics, not reproducible
  normal_map_flat / _interpolated        all views of the render at --width x --height (the render itself is not timed)
and how many of the index_add_ form's values differ between two runs, and from the kernel's.  The positions of either mesh
fit in the Infinity Cache, so the gathers are cache hits: these are cache-resident figures.
Prints each JSON line and appends it to --out (default profiles/mesh_smooth_speed.jsonl)."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--surfels", type=int, default=2000)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cluster-voxel", type=float, default=0.05, help="0: the extracted mesh only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_smooth_speed.jsonl"))
    a = ap.parse_args()
    import torch
    from scorp_amd import _C
    from scorp_amd.mesh import (GaussianExtractor, face_normals, filter_smooth_laplacian, filter_smooth_taubin, mesh_adjacency, normal_map,
                                simplify_vertex_clustering, vertex_normals)
    from scorp_amd.renderer2d import GaussianModel2D, render
    from scorp_amd.synthetic import ring_cameras
    from scorp_amd.train import PipelineParams
    from tests.test_mesh_gpu import sphere_surfels
    if not torch.cuda.is_available():
        raise SystemExit("time_mesh_smooth.py needs a GPU")
    dev = torch.device("cuda:0")

    def timed(fn):
        """median, smallest and largest of --reps runs after one warm-up, and the last result"""
        ts = []
        for rep in range(a.reps + 1):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            out = fn()
            t1.record()
            torch.cuda.synchronize()
            if rep:
                ts.append(t0.elapsed_time(t1))
        return {"ms": float(np.median(ts)), "ms_min": min(ts), "ms_max": max(ts)}, out

    model = GaussianModel2D.from_raw(sphere_surfels(a.surfels), 0, device=dev)
    model.active_sh_degree = 0
    pipe = PipelineParams()
    pipe.depth_ratio = 0.0
    ex = GaussianExtractor(model, render, pipe)
    ex.reconstruction(ring_cameras(a.views, a.width, a.height, 3, radius=4.0, device=dev))
    extracted = ex.extract_mesh_bounded(depth_trunc=6)
    meshes = [("extracted", extracted)]
    if a.cluster_voxel > 0:
        meshes.append((f"simplify_vertex_clustering({a.cluster_voxel})", simplify_vertex_clustering(extracted, a.cluster_voxel)))
    for name, mesh in meshes:
        F, Nv = int(mesh.faces.shape[0]), int(mesh.vertices.shape[0])
        print(f"{name}: {Nv} vertices, {F} faces", file=sys.stderr, flush=True)
        row = {"mesh": name, "num_faces": F, "num_vertices": Nv, "views": a.views, "width": a.width, "height": a.height, "surfels": a.surfels,
               "reps": a.reps}
        row["mesh_adjacency"], adj = timed(lambda: mesh_adjacency(mesh))
        row["neighbor_entries"] = int(adj.neighbors.shape[0])
        row["boundary_vertices"] = int(adj.boundary.sum())
        row["face_normals"], _ = timed(lambda: face_normals(mesh))
        row["vertex_normals"], normals = timed(lambda: vertex_normals(mesh, adjacency=adj))
        verts, out = mesh.vertices.contiguous(), torch.empty_like(mesh.vertices)
        half = (ctypes.c_double * 1)(0.5)
        row["half_step_call"], _ = timed(lambda: _C.call("scorp_mesh_smooth", verts, Nv, adj.neighbor_offsets, adj.neighbors, None, half, 1,
                                                         _C.MESH_SMOOTH_UNIFORM, None, out))
        row["filter_smooth_laplacian_1"], ours = timed(lambda: filter_smooth_laplacian(mesh, 1, adjacency=adj))
        row["filter_smooth_taubin_10"], _ = timed(lambda: filter_smooth_taubin(mesh, 10))
        row["filter_smooth_taubin_10_reused"], _ = timed(lambda: filter_smooth_taubin(mesh, 10, adjacency=adj))
        src = torch.repeat_interleave(torch.arange(Nv, device=dev), torch.diff(adj.neighbor_offsets.long()))
        dst = adj.neighbors.long()
        ones = torch.ones(src.shape[0], device=dev)

        def index_add_half_step():
            s = torch.zeros_like(verts).index_add_(0, src, verts[dst])
            n = torch.zeros(Nv, device=dev).index_add_(0, src, ones)
            return torch.where(n[:, None] > 0, verts + 0.5 * (s / n[:, None] - verts), verts)
        row["index_add_half_step"], theirs = timed(index_add_half_step)
        again = index_add_half_step()
        row["index_add_values_that_differ_between_two_runs"] = int((theirs != again).sum())
        row["index_add_values_that_differ_from_the_kernel"] = int((theirs != ours.vertices).sum())
        row["index_add_largest_difference_from_the_kernel"] = float((theirs - ours.vertices).abs().max())
        rendered = ex.render_mesh(mesh, colors=False, barycentric=True)
        row["normal_map_flat"], _ = timed(lambda: normal_map(rendered, mesh))
        row["normal_map_interpolated"], _ = timed(lambda: normal_map(rendered, mesh, normals))
        line = json.dumps(row)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
