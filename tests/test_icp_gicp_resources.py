"""Register budget of the generalized ICP pass (icp.hip), checked at compile time (no GPU), as
tests/test_icp_plane_resources.py checks the point-to-plane pass of the same file: the generalized pass carries the same
29 float64 sums plus the 3x3 inverse of a pair's combined covariance - no scratch, and no fewer waves per SIMD than the
point-to-plane pass gets in the same compile - and no kernel of the file spills."""
import os

import pytest

from scorp_amd.build import HIPCC
from tests.test_kernel_resources import _resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_icp_generalized_pass_keeps_the_plane_pass_occupancy():
    res = _resources("icp.hip")
    gicp = {k: v for k, v in res.items() if "icp_generalized_pass_kernel" in k}
    plane = {k: v for k, v in res.items() if "icp_plane_pass_kernel" in k}
    assert len(gicp) == 1 and len(plane) == 1, sorted(res)
    (name, r), (_, p) = *gicp.items(), *plane.items()
    print(f"{name}: {r['NumVgprs']} VGPRs, scratch {r['ScratchSize']}, occupancy {r['Occupancy']} (point-to-plane pass: "
          f"{p['NumVgprs']} VGPRs, occupancy {p['Occupancy']})")
    assert r["ScratchSize"] == 0, f"{name}: {r['ScratchSize']} bytes of scratch (spills in the pair arithmetic)"
    assert r["Occupancy"] >= p["Occupancy"], f"{name}: {r['Occupancy']} waves per SIMD, the point-to-plane pass has {p['Occupancy']}"
    assert any("icp_gather_covariances_kernel" in k for k in res)
    for name, r in res.items():
        assert r["ScratchSize"] == 0, f"{name}: {r['ScratchSize']} bytes of scratch"
