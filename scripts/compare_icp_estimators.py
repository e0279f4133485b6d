"""What the three ICP estimators of scorp_amd.icp make of two DIFFERENT samplings of one surface: tests/icp_reference's
asymmetric_object sampled twice (--points each, two seeds), the second sampling moved 5 degrees and 2 % of the extent off
and given noise of 0 / 0.3 % / 1 % of the extent, three seeds.  Every estimator starts at the identity with
r = 0.16 x the mean bounding-box edge and --max-iteration updates; point-to-plane gets estimate_normals of the target,
generalized estimate_covariances of both clouds (knn 30, epsilon 1e-3).  Prints one JSON line per (noise, seed): the final
rotation error in degrees and translation error (relative to the extent) of each estimator, and its updates."""
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
    a = ap.parse_args()
    from scorp_amd import icp
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
                res = icp.registration_icp(src, tgt, r, np.eye(4), max_iteration=a.max_iteration, estimation=est)
                T = res.transformation[0]
                dR = T[:3, :3] @ R0.T
                out[est] = {"rotation_error_deg": float(np.rad2deg(np.arccos(np.clip((np.trace(dR) - 1.0) / 2.0, -1.0, 1.0)))),
                            "translation_error_of_extent": float(np.linalg.norm(T[:3, 3] - t0) / extent),
                            "updates": int(res.iterations[0]), "fitness": float(res.fitness[0])}
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
