"""Time render_mesh and cull_unseen_faces (csrc/mesh_render.hip) on a mesh of the synthetic surfel scene of tests/test_mesh_gpu.py:
--surfels opaque surfels on a unit sphere, --views ring cameras at --width x --height, GaussianExtractor.reconstruction ->
extract_mesh_bounded at its default voxel size (depth_trunc 6: the cameras stand 4 away) -> the mesh, rendered from the
same cameras at the same size; then the same for that mesh after simplify_vertex_clustering with cells of --cluster-voxel,
whose triangles are tens of pixels across and take the workgroup path.  After a warm-up, the median of --reps runs with the smallest and largest, timed by
torch.cuda.Event pairs round the whole Python call (workspace allocation and check_mesh's host reads included):
  one line per view   render_mesh of that view alone (depth, face and colour), the triangles, those that went to the large
                      list (a clipped box of more than 64 pixel centres) and their share, the pixels the mesh owns
  one summary line    render_mesh of all views in one call, the same with depth and face only, face_visibility,
                      GaussianExtractor.cull_unseen_faces without and with a depth tolerance, and depth_difference of the
                      mesh's depth against the surfel depth maps
Prints each JSON line and appends it to --out (default profiles/mesh_render_speed.jsonl)."""
import argparse
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
    ap.add_argument("--depth-tolerance", type=float, default=0.05)
    ap.add_argument("--cluster-voxel", type=float, default=0.05, help="0: the extracted mesh only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_render_speed.jsonl"))
    a = ap.parse_args()
    import torch
    from scorp_amd.mesh import GaussianExtractor, depth_difference, face_visibility, render_mesh, simplify_vertex_clustering
    from scorp_amd.renderer2d import GaussianModel2D, render
    from scorp_amd.synthetic import ring_cameras
    from scorp_amd.train import PipelineParams
    from tests.test_mesh_gpu import sphere_surfels
    if not torch.cuda.is_available():
        raise SystemExit("time_mesh_render.py needs a GPU")
    dev = torch.device("cuda:0")

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")

    def event_ms(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), out

    def timed(fn):
        """median, smallest and largest of --reps runs after one warm-up, and the last result"""
        ts = []
        for rep in range(a.reps + 1):
            t, out = event_ms(fn)
            if rep:
                ts.append(t)
        return {"ms": float(np.median(ts)), "ms_min": min(ts), "ms_max": max(ts)}, out

    model = GaussianModel2D.from_raw(sphere_surfels(a.surfels), 0, device=dev)
    model.active_sh_degree = 0
    pipe = PipelineParams()
    pipe.depth_ratio = 0.0
    ex = GaussianExtractor(model, render, pipe)
    ex.reconstruction(ring_cameras(a.views, a.width, a.height, 3, radius=4.0, device=dev))
    extracted = ex.extract_mesh_bounded(depth_trunc=6)
    H, W = a.height, a.width
    meshes = [("extracted", extracted)]
    if a.cluster_voxel > 0:   # the same surface in triangles tens of pixels across: the workgroup path
        meshes.append((f"simplify_vertex_clustering({a.cluster_voxel})", simplify_vertex_clustering(extracted, a.cluster_voxel)))
    for name, mesh in meshes:
        F, Nv = int(mesh.faces.shape[0]), int(mesh.vertices.shape[0])
        print(f"{name}: {Nv} vertices, {F} faces", file=sys.stderr, flush=True)
        base = {"mesh": name, "width": W, "height": H, "views": a.views, "surfels": a.surfels, "num_faces": F, "num_vertices": Nv, "reps": a.reps}
        for v in range(a.views):
            fp = ex.full_proj[v:v + 1]
            header = []
            t, out = timed(lambda: render_mesh(mesh, fp, H, W, header=header))
            large = int(header[-1][0])
            emit(dict(base, view=v, render_mesh=t, large_triangles=large, large_share=large / max(1, F), pixels_owned=int((out.face >= 0).sum())))
        row = dict(base, view="all")
        row["render_mesh_all_views"], out = timed(lambda: ex.render_mesh(mesh))
        row["render_mesh_all_views_depth_and_face_only"], _ = timed(lambda: ex.render_mesh(mesh, colors=False))
        row["face_visibility"], seen = timed(lambda: face_visibility(mesh, ex.full_proj, H, W))
        row["cull_unseen_faces"], culled = timed(lambda: ex.cull_unseen_faces(mesh))
        row["cull_unseen_faces_with_depth_tolerance"], culled_tol = timed(lambda: ex.cull_unseen_faces(mesh, depth_tolerance=a.depth_tolerance))
        row.update(depth_tolerance=a.depth_tolerance, faces_seen=int((seen > 0).sum()), faces_after_cull=int(culled.faces.shape[0]),
                   faces_after_cull_with_depth_tolerance=int(culled_tol.faces.shape[0]),
                   depth_difference_against_the_surfel_depth=depth_difference(out.depth, ex.depthmaps).overall)
        emit(row)

if __name__ == "__main__":
    main()
