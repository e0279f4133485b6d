"""Time the vertex-clustering simplifier (csrc/mesh_simplify.hip) on the surface-nets mesh of a unit sphere over a ground
plane, extracted by extract_surface from an analytic distance grid of --resolutions^3 points over [-1.6, 1.6]^3, at cells of
--cells voxels, in both placements.  Per form the median of --reps runs after a warm-up, with the smallest and largest:
  cells / roots / accumulate / place / faces   hipEvent pairs round each C-ABI call (buffers allocated before);
  scan, compact                                the torch ops between and after them (cumsum of the root bytes; the face mask);
  cluster_vertices                             hipEvent pair round the whole call of scorp_amd.mesh (allocations, the host
                                               reads of the bounds, the cell count and the index range included);
  torch                                        a composition of torch ops that gives the same result on the same GPU:
                                               torch.unique on the cell keys, index_add_ for the sums, torch.linalg.eigh for the
                                               quadrics, torch.unique on the ordered triples.
The integer outputs of the two are compared, and the positions' largest difference is reported.  Prints one JSON line per
(resolution, cell, placement)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_composition(torch, verts, colors, faces, h, quadric):
    """rules 1 - 5 of include/scorp_gs.h with torch ops: (vertex_cell, positions, colours, faces)"""
    Nv = verts.shape[0]
    dev = verts.device
    v = verts.double()
    origin = verts.amin(0).double() - 0.5 * h
    ijk = torch.floor((v - origin) / h).long()
    _, inverse = torch.unique(ijk[:, 0] << 42 | ijk[:, 1] << 21 | ijk[:, 2], return_inverse=True)
    C = int(inverse.max()) + 1
    index = torch.arange(Nv, device=dev)
    first = torch.full((C,), Nv, dtype=torch.long, device=dev).scatter_reduce_(0, inverse, index, "amin")
    number = torch.empty_like(first)
    number[torch.argsort(first)] = torch.arange(C, device=dev)
    cell = number[inverse]
    sums = torch.zeros(C, 7, dtype=torch.float64, device=dev).index_add_(
        0, cell, torch.cat([v, colors.double(), torch.ones(Nv, 1, dtype=torch.float64, device=dev)], 1))
    count = sums[:, 6:7]
    mean = sums[:, :3] / count
    colours = (sums[:, 3:6] / count).float()
    positions = mean.float()
    if quadric:
        centre = torch.empty(C, 3, dtype=torch.float64, device=dev)
        centre[cell] = origin + (ijk.double() + 0.5) * h
        f = faces.long()
        p0 = v[f[:, 0]]
        N = torch.linalg.cross(v[f[:, 1]] - p0, v[f[:, 2]] - p0)
        length = torch.linalg.vector_norm(N, dim=1)
        live = length > 0
        f, p0, N, length = f[live], p0[live], N[live], length[live]
        a, n = 0.5 * length, N / length[:, None]
        corner = cell[f]                                                     # [T, 3]
        d = -((p0[:, None, :] - centre[corner]) * n[:, None, :]).sum(-1)     # [T, 3]
        outer = (a[:, None, None] * n[:, :, None] * n[:, None, :]).reshape(-1, 1, 9).expand(-1, 3, 9)
        rows = torch.cat([outer, (a[:, None] * d)[:, :, None] * n[:, None, :]], 2).reshape(-1, 12)
        Q = torch.zeros(C, 12, dtype=torch.float64, device=dev).index_add_(0, corner.reshape(-1), rows)
        A, b = Q[:, :9].reshape(C, 3, 3), Q[:, 9:]
        m = mean - centre
        sigma, vec = torch.linalg.eigh(A)
        r = -b - (A @ m[:, :, None])[:, :, 0]
        take = sigma > 1e-3 * sigma[:, 2:3]
        coef = torch.where(take, (vec * r[:, :, None]).sum(1) / sigma, torch.zeros_like(sigma))
        x = m + (vec * coef[:, None, :]).sum(2)
        moved = (count[:, 0] > 1) & (sigma[:, 2] > 0) & (x.abs() <= h).all(1)
        positions = torch.where(moved[:, None], (centre + x).float(), positions)
    t = cell[faces.long()]
    t = t[(t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 2] != t[:, 0])]
    t = torch.gather(t, 1, (torch.argmin(t, 1)[:, None] + torch.arange(3, device=dev)[None]) % 3)
    _, same = torch.unique(t, dim=0, return_inverse=True)
    at = torch.arange(t.shape[0], device=dev)
    winner = torch.full((int(same.max()) + 1,), t.shape[0], dtype=torch.long, device=dev).scatter_reduce_(0, same, at, "amin")
    return cell.int(), positions, colours, t[winner[same] == at].int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolutions", type=int, nargs="+", default=[192, 384, 640])
    ap.add_argument("--cells", type=float, nargs="+", default=[2.0, 4.0])
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    import torch
    from scorp_amd import _C
    from scorp_amd.mesh import Mesh, cluster_vertices, extract_surface
    if not torch.cuda.is_available():
        raise SystemExit("time_mesh_simplify.py needs a GPU")
    dev = torch.device("cuda:0")
    L = _C.lib()
    stream = _C.current_stream_ptr()

    def event_ms(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    for N in a.resolutions:
        c = torch.linspace(-1.6, 1.6, N, device=dev)
        x, y, z = torch.meshgrid(c, c, c, indexing="ij")
        grid = torch.minimum(torch.sqrt(x * x + y * y + (z - 0.1) ** 2) - 1.0, z + 0.7)
        del x, y, z
        verts, faces = extract_surface(grid, (c, c, c))
        del grid
        Nv, F = verts.shape[0], faces.shape[0]
        colors = torch.rand(Nv, 3, device=dev)
        lo = verts.amin(0).contiguous()
        spacing = 3.2 / (N - 1)
        for cells in a.cells:
            h = cells * spacing
            for quadric in (0, 1):
                i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
                slots, fslots = 1 << (2 * Nv - 1).bit_length(), 1 << (2 * F - 1).bit_length()
                keys = torch.empty(slots, dtype=torch.int64, device=dev)
                owner, slot, overflow, rep, vertex_cell = i32(slots), i32(Nv), i32(1), i32(Nv), i32(Nv)
                is_root = torch.empty(Nv, dtype=torch.uint8, device=dev)
                table, rotated = i32(fslots), i32(F, 3)
                keep = torch.empty(F, dtype=torch.uint8, device=dev)
                state = {}

                def cells_call():
                    _C.check(L.scorp_mesh_simplify_cells(verts.data_ptr(), Nv, lo.data_ptr(), h, keys.data_ptr(), owner.data_ptr(), slots,
                                                         slot.data_ptr(), overflow.data_ptr(), stream), "cells")

                def roots_call():
                    _C.check(L.scorp_mesh_simplify_roots(owner.data_ptr(), slots, slot.data_ptr(), Nv, rep.data_ptr(), is_root.data_ptr(), stream), "roots")

                def scan():
                    state["scan"] = torch.cumsum(is_root, 0, dtype=torch.int32)

                def accumulate_call():
                    _C.check(L.scorp_mesh_simplify_accumulate(verts.data_ptr(), colors.data_ptr(), Nv, faces.data_ptr(), F, lo.data_ptr(), h,
                                                              rep.data_ptr(), state["scan"].data_ptr(), state["C"], quadric, vertex_cell.data_ptr(),
                                                              state["ijk"].data_ptr(), state["acc"].data_ptr(), stream), "accumulate")

                def place_call():
                    _C.check(L.scorp_mesh_simplify_place(state["acc"].data_ptr(), state["ijk"].data_ptr(), state["C"], lo.data_ptr(), h, quadric,
                                                         state["pos"].data_ptr(), state["col"].data_ptr(), stream), "place")

                def faces_call():
                    _C.check(L.scorp_mesh_simplify_faces(faces.data_ptr(), F, vertex_cell.data_ptr(), Nv, table.data_ptr(), fslots, rotated.data_ptr(),
                                                         keep.data_ptr(), stream), "faces")

                def compact():
                    state["faces"] = rotated[keep.bool()]

                def whole():
                    state["whole"] = cluster_vertices(Mesh(verts, faces, colors), h, "quadric" if quadric else "average")

                def composition():
                    state["torch"] = torch_composition(torch, verts, colors, faces, h, quadric)

                names = ("cells", "roots", "scan", "accumulate", "place", "faces", "compact", "cluster_vertices", "torch")
                times = {k: [] for k in names}
                for rep_no in range(a.reps + 1):   # (the first is the warm-up)
                    row = {"cells": event_ms(cells_call), "roots": event_ms(roots_call), "scan": event_ms(scan)}
                    C = state["C"] = int(state["scan"][-1])
                    state["ijk"], state["acc"] = i32(C, 3), torch.empty(C, 16, dtype=torch.float64, device=dev)
                    state["pos"], state["col"] = torch.empty(C, 3, device=dev), torch.empty(C, 3, device=dev)
                    row.update({"accumulate": event_ms(accumulate_call), "place": event_ms(place_call), "faces": event_ms(faces_call),
                                "compact": event_ms(compact)})
                    row["cluster_vertices"] = event_ms(whole)   # (the two whole forms alternate)
                    row["torch"] = event_ms(composition)
                    if rep_no:
                        for k, v in row.items():
                            times[k].append(v)
                vc, mesh = state["whole"]
                tvc, tpos, tcol, tfaces = state["torch"]
                out = {"resolution": N, "cell_voxels": cells, "voxel_size": h, "contraction": "quadric" if quadric else "average",
                       "num_vertices": Nv, "num_faces": F, "num_cells": state["C"], "faces_after": int(mesh.faces.shape[0]), "reps": a.reps,
                       "overflow": int(overflow),
                       "separate_calls_equal_whole": bool(torch.equal(vertex_cell, vc) and torch.equal(state["faces"], mesh.faces)),
                       "torch_integers_equal": bool(torch.equal(tvc, vc) and torch.equal(tfaces, mesh.faces)),
                       "torch_position_max_abs_diff": float((tpos - mesh.vertices).abs().max()),
                       "torch_colour_max_abs_diff": float((tcol - mesh.colors).abs().max())}
                for k, v in times.items():
                    out[k] = {"ms": float(np.median(v)), "ms_min": min(v), "ms_max": max(v)}
                out["kernels_ms"] = sum(out[k]["ms"] for k in ("cells", "roots", "scan", "accumulate", "place", "faces", "compact"))
                out["torch_over_cluster_vertices"] = out["torch"]["ms"] / out["cluster_vertices"]["ms"]
                out["torch_over_kernels"] = out["torch"]["ms"] / out["kernels_ms"]
                print(json.dumps(out), flush=True)
                del keys, owner, slot, table, rotated, keep, state


if __name__ == "__main__":
    main()
