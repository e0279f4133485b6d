"""ms per camera of the 3-D segmentation vote at S3 (1 M Gaussians, 1600x1200; scorp_amd.synthetic), K objects:
(a) the reference pattern (utils/mask.py:42-100) through this library's drop-in render(..., override_color=ones) with the
    deterministic backward: 1 + 2K autograd passes with retain_graph and the norm votes;
(b) scorp_amd.segment.mask_votes: one render + one mask-vote pass per camera.
One JSON line per (K, form).  Device events around each camera after a warm-up.

    python scripts/time_mask_votes.py [--ks 1,4,8] [--cameras 3] [--only b]
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch


def blob_masks(K, H, W, seed, dev):
    rng = np.random.default_rng(seed)
    yy, xx = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    out = torch.zeros((K, H, W), dtype=torch.bool, device=dev)
    for k in range(K):
        for _ in range(3):
            cx, cy, r = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(0.05, 0.25) * min(H, W)
            out[k] |= (xx - cx) ** 2 + (yy - cy) ** 2 < r * r
    return out


class _Pipe:
    debug = False
    compute_cov3D_python = False
    convert_SHs_python = False


def reference_pattern(g, cam, masks, render, backward_precision):
    N, dev = g.get_xyz.shape[0], g.get_xyz.device
    votes = torch.zeros((masks.shape[0], N), device=dev)
    with backward_precision("deterministic"):
        colors = torch.ones((N, 3), requires_grad=True, device=dev)
        img = render(cam, g, _Pipe(), torch.zeros(3, device=dev), override_color=colors)["render"]
        img.permute(1, 2, 0).mean().backward(retain_graph=True)
        for k in range(masks.shape[0]):
            for sign, mm in ((1.0, masks[k]), (-1.0, ~masks[k])):
                colors.grad.zero_()
                (img.permute(1, 2, 0) * mm[..., None]).mean().backward(retain_graph=True)
                votes[k] += sign * colors.grad.norm(dim=1)
    return votes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", default="1,4,8")
    ap.add_argument("--cameras", type=int, default=3)
    ap.add_argument("--only", choices=["a", "b"], default=None)
    a = ap.parse_args()
    from scorp_amd.gaussian_model import GaussianModel
    from scorp_amd.rasterizer3d import backward_precision
    from scorp_amd.renderer import render
    from scorp_amd.segment import mask_votes
    from scorp_amd.synthetic import scene
    dev = torch.device("cuda:0")
    raw, cams, deg = scene("S3", device=dev, n_cameras=a.cameras + 1)
    g = GaussianModel.from_raw(raw, deg, device=dev)
    g.active_sh_degree = deg
    W, H = cams[0].resolution
    for K in [int(k) for k in a.ks.split(",")]:
        masks = [blob_masks(K, H, W, 100 + i, dev) for i in range(len(cams))]
        forms = {"a_reference_pattern": lambda c, m: reference_pattern(g, c, m, render, backward_precision),
                 "b_mask_votes": lambda c, m: mask_votes(g, [c], [m], "gradient")}
        for name, fn in forms.items():
            if a.only and not name.startswith(a.only):
                continue
            fn(cams[0], masks[0])                 # warm-up
            torch.cuda.synchronize()
            ms = []
            for c, m in zip(cams[1:], masks[1:]):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(c, m)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            print(json.dumps({"scene": "S3", "N": g.get_xyz.shape[0], "W": W, "H": H, "K": K, "form": name,
                              "ms_per_camera": round(float(np.median(ms)), 3), "ms_all": [round(x, 3) for x in ms]}), flush=True)


if __name__ == "__main__":
    main()
