"""Time the edge-collapse decimator (csrc/mesh_decimate.hip through scorp_amd.mesh.simplify_quadric_decimation) on the
surface-nets mesh of a unit sphere, extracted by extract_surface from an analytic distance grid of --resolution^3 points over
[-1.6, 1.6]^3, down to --fraction of its triangles.  Each of --reps runs after a warm-up is the whole Python call between
two synchronisations (wall clock: the call reads one count per round on the host, so the host is part of what a user
waits for).  Appends one JSON line to --out: the rounds, the time per round (total / rounds), the total time as the median
of the runs with the smallest and largest, the faces removed per round, and whether all runs gave the same tensors.
One more run goes through the same host loop with a hipEvent pair round each of the seven C-ABI calls (`calls_ms`, summed
over the rounds; the events add a little host time, so that run's own total is `split_total_ms`): the rest of a round is
torch's sorts, `unique`, scans and compaction and the host's read of the candidate count.
There is no earlier time to hold it to and no threshold: the file is the record."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class TimedCalls:
    """the seven calls of `ops`, each between two events"""

    def __init__(self, torch, ops):
        self.torch, self.ops, self.events = torch, ops, []

    def __getattr__(self, name):
        call = getattr(self.ops, name)

        def timed(*args):
            t0, t1 = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
            t0.record()
            call(*args)
            t1.record()
            self.events.append((name, t0, t1))
        return timed

    def totals(self):
        self.torch.cuda.synchronize()
        out = {}
        for name, t0, t1 in self.events:
            out[name] = out.get(name, 0.0) + t0.elapsed_time(t1)
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=384)
    ap.add_argument("--fraction", type=float, default=0.1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_decimate_speed.jsonl"))
    a = ap.parse_args()
    import torch
    from scorp_amd import _C
    from scorp_amd.mesh import Mesh, extract_surface, simplify_quadric_decimation
    if not torch.cuda.is_available():
        raise SystemExit("time_mesh_decimate.py needs a GPU")
    dev = torch.device("cuda:0")
    N = a.resolution
    c = torch.linspace(-1.6, 1.6, N, device=dev)
    x, y, z = torch.meshgrid(c, c, c, indexing="ij")
    grid = torch.sqrt(x * x + y * y + (z - 0.1) ** 2) - 1.0
    del x, y, z
    verts, faces = extract_surface(grid, (c, c, c))
    del grid
    mesh = Mesh(verts, faces, torch.rand(verts.shape[0], 3, device=dev))
    target = int(a.fraction * faces.shape[0])
    times, same, out, rounds = [], True, None, []
    for rep in range(a.reps + 1):   # (the first is the warm-up)
        rounds = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = simplify_quadric_decimation(mesh, target, rounds=rounds)
        torch.cuda.synchronize()
        if rep:
            times.append(1e3 * (time.perf_counter() - t0))
        if out is not None:
            same = same and torch.equal(got.faces, out.faces) and torch.equal(got.vertices, out.vertices) and torch.equal(got.colors, out.colors)
        out = got
    from scorp_amd.mesh import _decimate, _DecimateHip
    timed = TimedCalls(torch, _DecimateHip())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    split = _decimate(mesh.vertices, mesh.colors, mesh.faces, target, float("inf"), 1.0, timed)
    calls_ms = timed.totals()
    split_total_ms = 1e3 * (time.perf_counter() - t0)
    same = same and torch.equal(split.faces, out.faces) and torch.equal(split.vertices, out.vertices)
    radius = torch.linalg.vector_norm(out.vertices.double() - torch.tensor([0.0, 0.0, 0.1], dtype=torch.float64, device=dev), dim=1)
    removed = [r[3] for r in rounds]
    row = {"source_sha": _C.lib().scorp_source_sha().decode(), "device": torch.cuda.get_device_name(0), "resolution": N,
           "num_vertices": int(verts.shape[0]), "num_faces": int(faces.shape[0]), "target": target,
           "faces_after": int(out.faces.shape[0]), "vertices_after": int(out.vertices.shape[0]), "rounds": len(rounds), "reps": a.reps,
           "total_ms": float(np.median(times)), "total_ms_min": min(times), "total_ms_max": max(times),
           "ms_per_round": float(np.median(times)) / max(1, len(rounds)),
           "calls_ms": calls_ms, "calls_ms_sum": sum(calls_ms.values()), "split_total_ms": split_total_ms,
           "removed_over_window": float(np.mean([0.5 * r[3] / r[2] for r in rounds])) if rounds else 0.0,
           "faces_removed_first_rounds": removed[:8], "faces_removed_last_rounds": removed[-8:],
           "worst_radial_deviation": float((radius - 1.0).abs().max()), "runs_equal": bool(same)}
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
