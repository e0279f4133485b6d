"""Time the bounded TSDF route (scorp_amd.mesh.tsdf_blocks_fuse / extract_surface_blocks, csrc/tsdf_blocks.hip and
csrc/isosurface_blocks.hip or, with --method marching_cubes, csrc/marching_cubes_blocks.hip) at a working size:
scripts/time_tsdf.py's scene (a unit sphere over a ground plane, ray-cast; ring cameras), 32 views at 1600 x 1200, a voxel size
that gives tens of thousands of blocks.  Timed, each as the median of --reps runs after a warm-up with a hipEvent pair round
the call:
  (a) every C-ABI call on its own: touch (with its table clear), neighbors, integrate, the four surface calls;
  (b) tsdf_blocks_fuse and extract_surface_blocks as the Python layer runs them (compaction, scans and the host reads of the
      counts included), and the two together: what extract_mesh_bounded costs after its maps exist;
  (c) the integrate statements as torch ops on the GPU over the same blocks - every view over all voxels of every block that
      carries its bit, the running arrays in HBM - the only reference form that can run here.
Prints one JSON line and, with --out, writes it to a file."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def integrate_torch(depth, rgb, cam, keys, mask, voxel_length, sdf_trunc):
    """The integrate rule of include/scorp_gs.h as torch ops, one view at a time over the blocks that carry its bit."""
    import torch
    V, H, W = depth.shape
    B, dev = keys.numel(), depth.device
    coords = torch.stack([((keys >> s) & 0x1FFFFF) - (1 << 20) for s in (42, 21, 0)], -1)
    local = torch.stack(torch.unravel_index(torch.arange(4096, device=dev), (16, 16, 16)), -1)
    tsdf, w = torch.zeros(B * 4096, device=dev), torch.zeros(B * 4096, device=dev)
    col = torch.zeros(B * 4096, 3, device=dev)
    lane = torch.arange(4096, device=dev)
    for i in range(V):
        blocks = torch.nonzero((mask[:, i >> 5] >> (i & 31)) & 1)[:, 0]
        if blocks.numel() == 0:
            continue
        C = cam[i]
        c = voxel_length * ((coords[blocks][:, None, :] * 16 + local[None]).float() + 0.5)
        x, y, z = c[..., 0].reshape(-1), c[..., 1].reshape(-1), c[..., 2].reshape(-1)
        at = (blocks[:, None] * 4096 + lane[None]).reshape(-1)
        px, py, pz = (((C[4 * r] * x + C[4 * r + 1] * y) + C[4 * r + 2] * z) + C[4 * r + 3] for r in range(3))
        uf, vf = (px * C[12] / pz + C[14]) + 0.5, (py * C[13] / pz + C[15]) + 0.5
        ok = (pz > 0) & (uf >= 1e-4) & (uf < W - 1e-4) & (vf >= 1e-4) & (vf < H - 1e-4)
        at, pz, u, v = at[ok], pz[ok], uf[ok].long(), vf[ok].long()
        d = depth[i][v, u]
        rx, ry = (u.float() - C[14]) / C[12], (v.float() - C[15]) / C[13]
        sdf = (d - pz) * torch.sqrt((rx * rx + ry * ry) + 1)
        hit = (d > 0) & (sdf > -sdf_trunc)
        at, s, u, v = at[hit], (sdf[hit] / sdf_trunc).clamp(max=1.0), u[hit], v[hit]
        wo = w[at]
        wp = wo + 1
        tsdf[at] = (tsdf[at] * wo + s) / wp
        col[at] = (col[at] * wo[:, None] + rgb[i][v, u].float()) / wp[:, None]
        w[at] = wp
    return tsdf.reshape(B, 4096), w.reshape(B, 4096), col.reshape(B, 4096, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel-size", type=float, default=0.004)
    ap.add_argument("--sdf-trunc", type=float, default=0.02)
    ap.add_argument("--depth-trunc", type=float, default=8.0)
    ap.add_argument("--stride", type=int, default=4)
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--method", choices=("surface_nets", "marching_cubes"), default="surface_nets")
    ap.add_argument("--skip-restatement", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from scorp_amd import _C
    from scorp_amd import mesh as M
    from scorp_amd.synthetic import ring_cameras
    from tests import tsdf_reference as ref
    if not torch.cuda.is_available():
        raise SystemExit("time_tsdf_blocks.py needs a GPU")
    dev = torch.device("cuda:0")
    cams = ring_cameras(a.views, a.width, a.height, 7, radius=4.0)
    depth = torch.from_numpy(np.stack([ref.raycast_depth(c, size=(a.width, a.height)) for c in cams])).to(dev)
    depth[depth > a.depth_trunc] = 0      # (the ray-cast gives its `far` where a ray hits nothing)
    rgb = torch.randint(0, 256, (a.views, a.height, a.width, 3), dtype=torch.uint8, device=dev)
    E = torch.stack([c.world_view_transform.T[:3] for c in cams]).to(dev)
    # the pixel centres of raycast_depth are grid_sample's align_corners ones: u = (ndc + 1) / 2 * (W - 1)
    K = torch.tensor([[(a.width - 1) / 2 / np.tan(c.FoVx / 2), (a.height - 1) / 2 / np.tan(c.FoVy / 2), (a.width - 1) / 2, (a.height - 1) / 2]
                      for c in cams], dtype=torch.float32)
    vl, trunc = float(np.float32(a.voxel_size)), float(np.float32(a.sdf_trunc))

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ts, out = [], None
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return {"ms": float(np.median(ts)), "ms_all": [round(t, 3) for t in ts]}, out

    mc = a.method == "marching_cubes"
    out = {"method": a.method} if mc else {}   # (the default's record keeps the keys it always had)
    out.update({"views": a.views, "width": a.width, "height": a.height, "voxel_size": vl, "sdf_trunc": trunc, "stride": a.stride})
    out["tsdf_blocks_fuse"], vol = timed(lambda: M.tsdf_blocks_fuse(depth, rgb, E, K, vl, trunc, stride=a.stride))
    B = vol.keys.numel()
    out["blocks"], out["observed_share"] = B, float((vol.weight > 0).float().mean())
    out["extract_surface_blocks"], mesh = timed(lambda: M.extract_surface_blocks(vol, method=a.method))
    out["vertices"], out["faces"] = mesh.vertices.shape[0], mesh.faces.shape[0]
    out["fuse_and_extract"], _ = timed(lambda: M.extract_surface_blocks(M.tsdf_blocks_fuse(depth, rgb, E, K, vl, trunc, stride=a.stride), method=a.method))

    # (a) the calls on their own, on buffers sized once
    L, stream = _C.lib(), _C.current_stream_ptr()
    d32, cam = depth.contiguous(), torch.cat([E.reshape(a.views, 12), K.to(dev)], 1).contiguous()
    views = _C.ScorpTsdfBlockViews(depth=d32.data_ptr(), rgb=rgb.data_ptr(), cam=cam.data_ptr(), num_views=a.views, width=a.width, height=a.height)
    words = (a.views + 31) // 32
    slots = 1 << (2 * B - 1).bit_length()
    tk = torch.empty(slots, dtype=torch.int64, device=dev)
    tm = torch.empty(slots, words, dtype=torch.int32, device=dev)
    ov = torch.empty(1, dtype=torch.int32, device=dev)
    out["table_slots"] = slots
    out["touch"], _ = timed(lambda: _C.check(L.scorp_tsdf_blocks_touch(ctypes.byref(views), vl, trunc, a.stride, tk.data_ptr(), tm.data_ptr(), slots,
                                                                      ov.data_ptr(), stream), "touch"))
    assert int(ov) == 0 and int((tk != -1).sum()) == B
    nbr = torch.empty(B, 27, dtype=torch.int32, device=dev)
    out["neighbors"], _ = timed(lambda: _C.check(L.scorp_tsdf_blocks_neighbors(vol.keys.data_ptr(), B, nbr.data_ptr(), stream), "neighbors"))
    t, w, c = torch.empty_like(vol.tsdf), torch.empty_like(vol.weight), torch.empty_like(vol.colour)
    out["integrate"], _ = timed(lambda: _C.check(L.scorp_tsdf_blocks_integrate(ctypes.byref(views), vl, trunc, vol.keys.data_ptr(), vol.view_mask.data_ptr(),
                                                                              B, t.data_ptr(), w.data_ptr(), c.data_ptr(), stream), "integrate"))
    out["integrate"]["voxel_views_per_s"] = float(vol.weight.sum()) / (out["integrate"]["ms"] * 1e-3)
    out["integrate_without_colour"], _ = timed(lambda: _C.check(L.scorp_tsdf_blocks_integrate(
        ctypes.byref(views), vl, trunc, vol.keys.data_ptr(), vol.view_mask.data_ptr(), B, t.data_ptr(), w.data_ptr(), None, stream), "integrate"))
    vp = (vol.tsdf.data_ptr(), vol.weight.data_ptr(), nbr.data_ptr(), B)   # what every surface call starts with
    flags = torch.empty(B * 4096, dtype=torch.uint8, device=dev)
    counts = torch.empty(B * 4096, dtype=torch.uint8, device=dev)
    verts_of = lambda n: (torch.empty(n, 3, device=dev), torch.empty(n, 3, device=dev))
    if mc:   # count_edges / emit_vertices / count_faces / emit_faces; flags = the edge masks, first_scan = the edge scan
        edge_counts = torch.empty(B * 4096, dtype=torch.uint8, device=dev)
        out["count_edges"], _ = timed(lambda: _C.check(L.scorp_marching_cubes_blocks_count_edges(*vp, flags.data_ptr(), edge_counts.data_ptr(), stream),
                                                       "count_edges"))
        first_scan = torch.cumsum(edge_counts, 0, dtype=torch.int64).to(torch.int32)
        nv = int(first_scan[-1])
        verts, cols = verts_of(nv)
        out["emit_vertices"], _ = timed(lambda: _C.check(L.scorp_marching_cubes_blocks_emit_vertices(
            vol.tsdf.data_ptr(), vol.weight.data_ptr(), vol.colour.data_ptr(), vol.keys.data_ptr(), nbr.data_ptr(), B, vl, flags.data_ptr(),
            first_scan.data_ptr(), nv, verts.data_ptr(), cols.data_ptr(), stream), "emit_vertices"))
        out["count_faces"], _ = timed(lambda: _C.check(L.scorp_marching_cubes_blocks_count_faces(*vp, counts.data_ptr(), stream), "count_faces"))
        face_scan = torch.cumsum(counts, 0, dtype=torch.int64).to(torch.int32)
        nf = int(face_scan[-1])
        faces = torch.empty(nf, 3, dtype=torch.int32, device=dev)
        out["emit_faces"], _ = timed(lambda: _C.check(L.scorp_marching_cubes_blocks_emit_faces(
            *vp, flags.data_ptr(), first_scan.data_ptr(), face_scan.data_ptr(), nf, faces.data_ptr(), stream), "emit_faces"))
        first_counts = edge_counts
    else:
        out["count_cells"], _ = timed(lambda: _C.check(L.scorp_isosurface_blocks_count_cells(*vp, flags.data_ptr(), stream), "count_cells"))
        cell_scan = torch.cumsum(flags, 0, dtype=torch.int64).to(torch.int32)
        nv = int(cell_scan[-1])
        verts, cols = verts_of(nv)
        out["emit_vertices"], _ = timed(lambda: _C.check(L.scorp_isosurface_blocks_emit_vertices(
            vol.tsdf.data_ptr(), vol.weight.data_ptr(), vol.colour.data_ptr(), vol.keys.data_ptr(), nbr.data_ptr(), B, vl, cell_scan.data_ptr(), nv,
            verts.data_ptr(), cols.data_ptr(), stream), "emit_vertices"))
        out["count_faces"], _ = timed(lambda: _C.check(L.scorp_isosurface_blocks_count_faces(*vp, counts.data_ptr(), stream), "count_faces"))
        edge_scan = torch.cumsum(counts, 0, dtype=torch.int64).to(torch.int32)
        nq = int(edge_scan[-1])
        faces = torch.empty(2 * nq, 3, dtype=torch.int32, device=dev)
        out["emit_faces"], _ = timed(lambda: _C.check(L.scorp_isosurface_blocks_emit_faces(
            *vp, cell_scan.data_ptr(), edge_scan.data_ptr(), nq, faces.data_ptr(), stream), "emit_faces"))
        first_counts = flags
    out["scans"], _ = timed(lambda: (torch.cumsum(first_counts, 0, dtype=torch.int64).to(torch.int32),
                                     torch.cumsum(counts, 0, dtype=torch.int64).to(torch.int32)))
    if not a.skip_restatement:
        out["integrate_torch_ops"], (t_ref, w_ref, c_ref) = timed(lambda: integrate_torch(d32, rgb, cam, vol.keys, vol.view_mask, vl, trunc))
        out["weights_differing_kernel_vs_torch_ops"] = int((w_ref != vol.weight).sum())
        same = w_ref == vol.weight
        out["max_abs_tsdf_difference_where_weights_agree"] = float((t_ref - vol.tsdf)[same].abs().max())
        out["speedup_integrate_vs_torch_ops"] = out["integrate_torch_ops"]["ms"] / out["integrate"]["ms"]
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
