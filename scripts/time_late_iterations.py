"""Time FULL training iterations after depth_from_iter (train_3dgs.py:109-150: three quarters of a default run) at the
bench's S3 size - 1 M Gaussians, 1600x1200, SH degree 3 - as bench.py --full times the early ones: training_iteration with
fused_view=True, PairPolicy "reserve", densification and opacity reset off, device events around --iters iterations after
--warmup warm-up ones.  Three regimes:

    iso         iterations from 7001, the isotropic regulariser only (the reference's default run with no depth files)
    iso_depth   iterations from 7001, isotropic + sensor depth + estimated depth
    early       the same loop from iteration 5001 (no extra term: the ceiling for the other two)

--surfels times the 2DGS loop instead (train_2dgs.py; use --scene S6): "early" then starts at iteration 8000 with the
isotropic weight 0 (no extra term, the normal regulariser on), "iso" and "iso_depth" start at 9000, where the estimate also
brings the two depth-normal terms.  --no-fused-view takes the loop's autograd branch (the A/B side for the terms a parent
commit's loop does not compute).

Prints one JSON line.  --tree DIR imports scorp_amd from another checkout (A/B against the parent commit, whose loop
leaves the one-call view for render() + autograd + FusedAdam.step() in the first two regimes); SCORP_GS_LIB selects the
library as everywhere.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT, help="checkout to import scorp_amd from")
    ap.add_argument("--scene", default="S3")
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--cams", type=int, default=8)
    ap.add_argument("--regimes", default="iso,iso_depth,early")
    ap.add_argument("--surfels", action="store_true")
    ap.add_argument("--no-fused-view", action="store_true")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    import scorp_amd
    from scorp_amd import rasterizer3d as R
    from scorp_amd.gaussian_model import GaussianModel, OptimizationParams
    from scorp_amd.rasterizer3d import PairPolicy
    from scorp_amd.renderer import render
    from scorp_amd.synthetic import SCENES, make_gaussians, ring_cameras
    from scorp_amd.train import PipelineParams, training_iteration
    if a.surfels:
        from scorp_amd.gaussian_model import OptimizationParams2D as OptimizationParams
        from scorp_amd.renderer2d import GaussianModel2D as GaussianModel, render

    dev = torch.device("cuda:0")
    N, W, H, deg, seed, ncam = SCENES[a.scene]
    raw = make_gaussians(N, deg, seed)
    if a.surfels:
        raw["scaling"] = raw["scaling"][:, :2].copy()
    loop_kw = dict(fused_view=not a.no_fused_view)
    if a.surfels:
        loop_kw.update(surfels=True, render_fn=render)
    cams = ring_cameras(ncam, W, H, seed, device=dev)[:a.cams]
    bg, pipe = torch.zeros(3, device=dev), PipelineParams()
    g = torch.Generator(device=dev).manual_seed(1234)
    rand = lambda *s: torch.rand(*s, device=dev, generator=g)
    res = {"tree": os.path.dirname(os.path.abspath(scorp_amd.__file__)), "lib": os.environ.get("SCORP_GS_LIB", "in-tree"),
           "scene": a.scene, "gaussians": N, "iters": a.iters, "warmup": a.warmup, "surfels": a.surfels,
           "fused_view": not a.no_fused_view}
    for regime in a.regimes.split(","):
        model = GaussianModel.from_raw(raw, deg, device=dev)
        model.active_sh_degree = deg
        PairPolicy.mode = "exact"
        gts, sensors, ests = [], [], []
        n0 = len(R.LAST_NUM_PAIRS_LOG)
        with torch.no_grad():
            for cam in cams:
                out = render(cam, model, pipe, bg)
                gts.append((out["render"] + 0.05 * torch.randn(out["render"].shape, device=dev, generator=g)).clamp(0, 1))
                s, e = 2.0 + 2.0 * rand(1, H, W), rand(1, H, W)
                s[rand(1, H, W) < 0.1] = 0.0
                e[rand(1, H, W) < 0.1] = 0.0
                sensors.append(s)
                ests.append(e)
        PairPolicy.reset()
        PairPolicy.mode, PairPolicy.reserve = "reserve", int(max(R.LAST_NUM_PAIRS_LOG[n0:]) * 1.25) + 1024
        opt = OptimizationParams()
        opt.densify_from_iter, opt.opacity_reset_interval, opt.random_background = 1 << 30, 1 << 30, False
        if a.surfels:
            start = 8000 if regime == "early" else 9000
            if regime == "early":
                opt.lambda_isotropic = 0.0
        elif regime == "early":
            start = 5001
        else:
            start = opt.depth_from_iter + 1
        model.training_setup(opt)

        def it(i):
            k = i % len(cams)
            kw = dict(gt_depth=sensors[k], gt_depth_est=ests[k]) if regime == "iso_depth" else {}
            loss, _ = training_iteration(model, cams[k], gts[k], opt, pipe, bg, start + i, scene_extent=3.0, **loop_kw, **kw)
            return loss

        for i in range(a.warmup):
            it(i)
        PairPolicy.drain()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(a.iters):
            loss = it(a.warmup + i)
        e1.record()
        PairPolicy.drain()
        torch.cuda.synchronize()
        res[regime + "_iterations_per_s"] = round(a.iters / (e0.elapsed_time(e1) * 1e-3), 1)
        res[regime + "_last_loss"] = round(float(loss), 6)
        del model
        torch.cuda.empty_cache()
    PairPolicy.mode = "exact"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
