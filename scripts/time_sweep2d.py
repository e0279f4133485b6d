"""Time the 128-rotation sweep of a surfel object (scorp_amd.align) at the align loop's size: a 100 k-surfel SH-0 object,
15 cameras at 800x800, rotations_128.npz, in the forms a caller can reach:

  per_view        the object rotated per hypothesis, one renderer2d.render per camera and the comparison in torch
                  (the generic branch of hypothesis_fitness: what a surfel sweep ran before the stacked kernels);
  eager_stacked   the object rotated per hypothesis, its 15 views as ONE stacked scoring launch set
                  (rotation_sweep(..., use_graph=False));
  stacked_b1/2/3  the cameras moved instead of the object, 1 / 2 / 3 hypotheses per stacked scoring launch set
                  (align.StackedSweep: what rotation_sweep picks for an SH-0 GaussianModel2D).

Every form is warmed up, then timed over whole sweeps with a host clock around work that ends in a device synchronise; the
forms alternate inside each of --reps repeats, so that drift of the shared host hits all of them alike.  One JSON line per
form (hypotheses/s: median and every repeat, the arg-max it found) is printed and appended to --out."""
import argparse
import copy
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--surfels", type=int, default=100_000)
    ap.add_argument("--cameras", type=int, default=15)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--rotations", type=int, default=128)
    ap.add_argument("--depth-ratio", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=12, help="hypotheses scored per form before the timed repeats")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep2d_speed.jsonl"))
    a = ap.parse_args()
    import torch
    from scorp_amd import renderer2d
    from scorp_amd.align import SweepPlan, render_views
    from scorp_amd.rasterizer3d import PairPolicy
    from scorp_amd.synthetic import make_gaussians, ring_cameras
    from scorp_amd.transforms import gaussians_rotate

    assert torch.cuda.is_available(), "time_sweep2d.py needs a GPU"
    dev = torch.device("cuda:0")
    rots = np.load(os.path.join(ROOT, "tests", "golden", "rotations_128.npz"))["rotations"][:a.rotations]
    planted = min(77, len(rots) - 1)
    raw = make_gaussians(a.surfels, 0, 4, extent=0.8, log_scale_mean=math.log(0.01), scale_dims=2)   # bench.py's sweep object, as surfels
    raw["xyz"][:, 0] *= 1.6
    obj = renderer2d.GaussianModel2D.from_raw(raw, 0, device=dev)
    cams = ring_cameras(a.cameras, a.size, a.size, 4, radius=3.0, device=dev)
    bg = torch.zeros(3, device=dev)
    tgt = copy.copy(obj)
    tgt._xyz, tgt._rotation, tgt._features_rest = obj._xyz.detach().clone(), obj._rotation.detach().clone(), obj._features_rest.detach().clone()
    gaussians_rotate(tgt, torch.tensor(rots[planted], dtype=torch.float32, device=dev), fix_center=True)
    targets = render_views(tgt, cams, bg, render_fn=renderer2d.render, depth_ratio=a.depth_ratio)

    per_view = lambda *args, **kw: renderer2d.render(*args, **kw)   # not renderer2d.render itself: the generic branch
    plans = {"per_view": SweepPlan(obj, cams, targets, bg, use_graph=False, render_fn=per_view, depth_ratio=a.depth_ratio),
             "eager_stacked": SweepPlan(obj, cams, targets, bg, use_graph=False, depth_ratio=a.depth_ratio)}
    for b in (1, 2, 3):
        p = SweepPlan(obj, cams, targets, bg, depth_ratio=a.depth_ratio)
        assert p.stacked is not None, "the stacked sweep refused the surfel object"
        p.stacked.batch = b
        plans[f"stacked_b{b}"] = p
    ids = list(range(len(rots)))

    def sweep(plan, which):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scores = torch.stack(plan.score(rots, which))
        best = int(torch.argmax(scores[:, 0]))      # (a device-to-host read: the sweep's result)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, which[best], float(scores[best, 0])

    for plan in plans.values():
        sweep(plan, ids[:a.warmup])
    secs = {k: [] for k in plans}
    found = {}
    for _ in range(a.reps):
        for name, plan in plans.items():    # the forms alternate inside a repeat
            dt, best, fit = sweep(plan, ids)
            secs[name].append(dt)
            found[name] = (best, fit)
    PairPolicy.reset()
    base = float(np.median(secs["per_view"]))
    lines = []
    for name in plans:
        med = float(np.median(secs[name]))
        lines.append({"form": name, "surfels": a.surfels, "cameras": a.cameras, "size": a.size, "rotations": len(rots),
                      "depth_ratio": a.depth_ratio, "hypotheses_per_s": round(len(rots) / med, 1),
                      "hypotheses_per_s_all": [round(len(rots) / t, 1) for t in secs[name]], "seconds_per_sweep": round(med, 4),
                      "speedup_over_per_view": round(base / med, 2), "best_id": found[name][0], "planted_id": planted,
                      "best_fitness": found[name][1], "device": torch.cuda.get_device_name(0)})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        for rec in lines:
            print(json.dumps(rec))
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
