"""The float64 reference pipeline on the concave registration pair of tests/orient_fixtures.py (a mug): numpy PCA normals
of 12 neighbours, oriented by tests/orient_reference.py (tangent plane) or away from the centroid, the FPFH, matching and
RANSAC of tests/fpfh_reference.py at the FPFH fixtures' settings (radius 0.3, max_nn 64, 4096 fixed triples, distance
0.08), no ICP.  Prints per orientation the share of normals signed outward and the pose error; about 20 s each on one
core.  tests/test_orient_gpu.py::test_route_on_a_concave_object quotes its figures."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import fpfh_reference as fref          # noqa: E402
from tests import orient_fixtures as fx           # noqa: E402
from tests import orient_reference as oref        # noqa: E402


def main():
    pair = fx.mug_pair()
    for mode in ("tangent_plane", "away_from"):
        feats = []
        for name in ("source", "target"):
            P, truth = pair[name], pair[name + "_normals"]
            N, nb = oref.pca_normals(P, 12)
            N = oref.orient(P, N, nb)["normals"] if mode == "tangent_plane" else oref.away_from(P, N)
            print(f"{mode} {name}: {len(P)} points, {fx.outward_fraction(N, truth):.4f} outward", flush=True)
            feats.append(fref.fpfh(P, N, 0.3, 64)["feature"])
        c = len(fref.correspondences(feats[0], feats[1]))
        samples = np.random.default_rng(13).integers(0, c, (4096, 3))
        out = fref.ransac(pair["source"], pair["target"], feats[0], feats[1], 0.08, samples)
        ang, dt = fref.pose_error(out["transformation"], pair["truth"])
        print(f"{mode}: {c} correspondences, winner {out['inlier_count']} inliers, rotation error {ang:.4f} deg, translation error "
              f"{dt / pair['diagonal']:.2e} of the diagonal {pair['diagonal']:.3f}", flush=True)


if __name__ == "__main__":
    main()
