"""What the four ICP estimators of scorp_amd.icp make of two DIFFERENT samplings of one surface: tests/icp_reference's
asymmetric_object sampled twice (--points each, two seeds), the second sampling moved 5 degrees and 2 % of the extent off
and given noise of 0 / 0.3 % / 1 % of the extent, three seeds.  Every estimator starts at the identity with
r = 0.16 x the mean bounding-box edge and --max-iteration updates; point-to-plane gets estimate_normals of the target,
generalized estimate_covariances of both clouds (knn 30, epsilon 1e-3), coloured a smooth texture of position
(tests/icp_color_fixtures.smooth_texture, the source's taken where it lies on the object) with the target's estimated normals
and colour gradients.  Prints one JSON line per (noise, seed): the final rotation error in degrees and translation error
(relative to the extent) of each estimator, and its updates.

Then the workload geometry cannot fix: the textured sheet of tests/icp_color_fixtures.py (a gently curved 40 x 40 lattice
with a smooth texture; 900 independent samples of it moved 2 degrees and (0.03, -0.02, 0.004) in its own plane), three
seeds, rebuilt here with the GPU's normals and gradients at knn 20.  One JSON line per seed: the RMS alignment error at the
start and after each estimator's run of up to --sheet-max-iteration updates, and its updates."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=3000)
    ap.add_argument("--max-iteration", type=int, default=30)
    ap.add_argument("--noise", type=float, nargs="+", default=[0.0, 0.003, 0.01], help="shares of the extent")
    ap.add_argument("--seeds", type=int, nargs="+", default=[0, 1, 2])
    ap.add_argument("--sheet-max-iteration", type=int, default=100)
    a = ap.parse_args()
    from scorp_amd import icp
    from tests import icp_color_fixtures as cfx
    from tests import icp_reference as ref

    ang = np.deg2rad(5.0)
    R0 = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
    for noise in a.noise:
        for seed in a.seeds:
            tgt = ref.asymmetric_object(a.points, seed).astype(np.float32)
            t64 = tgt.astype(np.float64)
            extent = float(np.ptp(t64, axis=0).max())
            t0 = 0.02 * extent * np.array([0.6, -0.64, 0.48])
            rng = np.random.default_rng(1000 + seed)
            other = ref.asymmetric_object(a.points, 100 + seed)
            other = other + rng.normal(scale=noise * extent, size=other.shape)
            src = ((other - t0) @ R0).astype(np.float32)            # q = R0 p + t0 maps it back
            r = float(np.ptp(t64, axis=0).mean() * 0.16)
            out = {"points": a.points, "noise": noise, "seed": seed, "max_iteration": a.max_iteration}
            for est in icp.ESTIMATIONS:
                colors = {"source_colors": cfx.smooth_texture(other), "target_colors": cfx.smooth_texture(tgt)} if est == "colored" else {}
                res = icp.registration_icp(src, tgt, r, np.eye(4), max_iteration=a.max_iteration, estimation=est, **colors)
                T = res.transformation[0]
                dR = T[:3, :3] @ R0.T
                out[est] = {"rotation_error_deg": float(np.rad2deg(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0)))),
                            "translation_error_of_extent": float(np.linalg.norm(T[:3, 3] - t0) / extent),
                            "updates": int(res.iterations[0]), "fitness": float(res.fitness[0])}
            print(json.dumps(out), flush=True)

    want = cfx.sheet_truth()
    back = np.linalg.inv(want)
    for seed in a.seeds:
        rng = np.random.default_rng(seed)
        g = np.stack(np.meshgrid(np.arange(40) * 0.025, np.arange(40) * 0.025, indexing="ij"), -1).reshape(-1, 2)
        xy = g + rng.uniform(-0.006, 0.006, g.shape)
        tgt = np.column_stack([xy, cfx.sheet_height(xy[:, 0])]).astype(np.float32)
        sxy = rng.uniform(0.15 * 0.975, 0.85 * 0.975, (900, 2))
        samples = np.column_stack([sxy, cfx.sheet_height(sxy[:, 0])])
        src = (samples @ back[:3, :3].T + back[:3, 3]).astype(np.float32)
        Iq, Ip = cfx.sheet_texture(tgt[:, 0].astype(np.float64), tgt[:, 1].astype(np.float64)), cfx.sheet_texture(sxy[:, 0], sxy[:, 1])
        N = icp.estimate_normals(tgt, knn=cfx.SHEET_KNN)
        C = icp.covariances_from_normals(N)
        out = {"workload": "textured sheet", "seed": seed, "target": len(tgt), "source": len(src), "r": cfx.SHEET_R,
               "max_iteration": a.sheet_max_iteration, "start_rms_alignment_error": cfx.rms_alignment_error(np.eye(4), src)}
        for est in icp.ESTIMATIONS:
            kw = {"point_to_plane": {"target_normals": N}, "generalized": {"target_covariances": C},
                  "colored": {"target_normals": N, "source_colors": Ip, "target_colors": Iq,
                              "target_gradients": icp.estimate_color_gradients(tgt, Iq, normals=N, knn=cfx.SHEET_KNN)}}.get(est, {})
            res = icp.registration_icp(src, tgt, cfx.SHEET_R, np.eye(4), max_iteration=a.sheet_max_iteration, estimation=est, **kw)
            out[est] = {"rms_alignment_error": cfx.rms_alignment_error(res.transformation[0], src), "updates": int(res.iterations[0]),
                        "fitness": float(res.fitness[0])}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
