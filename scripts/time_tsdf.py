"""Time the multi-view TSDF fusion (scorp_amd.mesh.tsdf_fuse, csrc/tsdf.hip) at a working size: 256^3 lattice samples of
the contracted space against 32 views at 1600 x 1200 (a unit sphere over a ground plane, ray-cast; ring cameras).  Three forms:
  (a) the kernel, one launch, without colour (how the volume is filled) and with it;
  (b) the reference's statements (tests/tsdf_reference.unbounded_tsdf) on the GPU with the maps resident;
  (c) the same with the maps on the host and copied per view, the reference's actual pattern.
(b) and (c) always sample and average the colour maps as well, as the reference does: the like-for-like kernel form is the
one with colour.
Prints one JSON line: ms per call (median of --reps after a warm-up call, host clock around a device synchronise),
sample-views/s, and for (a) the share of HBM bandwidth over its compulsory bytes (every map and coordinate read once, the
output written once), and the largest difference between (a) and (b)."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12   # bytes/s: the specification, and a measured float4 copy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--views", type=int, default=32)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-restatement", action="store_true")
    a = ap.parse_args()
    import torch
    from scorp_amd.mesh import tsdf_fuse
    from scorp_amd.synthetic import ring_cameras
    from tests import tsdf_reference as ref
    if not torch.cuda.is_available():
        raise SystemExit("time_tsdf.py needs a GPU")
    dev = torch.device("cuda:0")
    cams = ring_cameras(a.views, a.width, a.height, 7, radius=4.0)
    depth_h = torch.from_numpy(np.stack([ref.raycast_depth(c, size=(a.width, a.height)) for c in cams])).pin_memory()
    rgb_h = torch.zeros(a.views, 3, a.height, a.width).pin_memory()
    fp = torch.stack([c.full_proj_transform for c in cams]).to(dev)
    depth = depth_h.to(dev)
    N = a.resolution
    coords = tuple(torch.linspace(-1.2, 1.2, N, device=dev) for _ in range(3))
    voxel, kw = 2 * 4.0 / N, dict(center=(0.0, 0.0, 0.0), radius=4.0)
    M = N ** 3

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts)), [round(t, 3) for t in ts], out

    out = {"samples": M, "views": a.views, "width": a.width, "height": a.height}
    ms, all_ms, grid = timed(lambda: tsdf_fuse(depth, None, fp, coords, voxel, contracted=True, **kw))
    compulsory = 4 * M + 4 * a.views * a.width * a.height + 64 * a.views + 12 * N
    out["kernel"] = {"ms": ms, "ms_all": all_ms, "sample_views_per_s": M * a.views / (ms * 1e-3), "compulsory_bytes": compulsory,
                     "hbm_share_of_8.0TBps": compulsory / (ms * 1e-3) / HBM_PEAK,
                     "hbm_share_of_6.29TBps_copy": compulsory / (ms * 1e-3) / HBM_COPY}
    rgb = torch.zeros(a.views, 3, a.height, a.width, device=dev)
    ms, all_ms, _ = timed(lambda: tsdf_fuse(depth, rgb, fp, coords, voxel, contracted=True, **kw))
    out["kernel_with_colour"] = {"ms": ms, "ms_all": all_ms, "sample_views_per_s": M * a.views / (ms * 1e-3)}
    if not a.skip_restatement:
        pts = ref.lattice_points(coords)
        ms, all_ms, (t_ref, _) = timed(lambda: ref.unbounded_tsdf(pts, depth, rgb, fp, voxel, True, **kw))
        out["restatement_resident"] = {"ms": ms, "ms_all": all_ms, "sample_views_per_s": M * a.views / (ms * 1e-3)}
        out["max_abs_difference_kernel_vs_restatement"] = float((grid.reshape(-1) - t_ref).abs().max())
        out["share_differing_by_more_than_1e-4"] = float(((grid.reshape(-1) - t_ref).abs() > 1e-4).float().mean())

        def host_maps():   # mesh_utils.py:204-205: depthmap.cuda(), rgbmap.cuda() inside the per-view call
            class PerView:
                def __init__(self, t): self.t = t
                def to(self, dtype): return self
                @property
                def shape(self): return self.t.shape
                def __getitem__(self, i): return self.t[i].to(dev, non_blocking=False)
            return ref.unbounded_tsdf(pts, PerView(depth_h), PerView(rgb_h), fp, voxel, True, **kw)
        ms, all_ms, _ = timed(host_maps)
        out["restatement_host_maps"] = {"ms": ms, "ms_all": all_ms, "sample_views_per_s": M * a.views / (ms * 1e-3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
