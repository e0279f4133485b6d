"""Register budget of the point-to-plane ICP and normal-estimation kernels (icp.hip), checked at compile time (no
GPU), as tests/test_icp_resources.py checks the point-to-point pair of the same file: the pass carries 29 float64 sums and the ring search in registers -
no scratch, at most 128 VGPRs (four waves per SIMD) - the normals kernel keeps its candidate list in LDS, not in scratch,
and no kernel of the file spills."""
import os

import pytest

from scorp_amd.build import HIPCC
from tests.test_kernel_resources import _resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_icp_plane_kernels_keep_their_occupancy():
    res = _resources("icp.hip")
    search = {k: v for k, v in res.items() if "icp_plane_pass_kernel" in k}
    assert len(search) == 1, sorted(res)
    for name, r in search.items():
        assert r["ScratchSize"] == 0, f"{name}: {r['ScratchSize']} bytes of scratch (spills in the search loop)"
        assert r["NumVgprs"] <= 128, f"{name}: {r['NumVgprs']} VGPRs > 128"
        assert r["Occupancy"] >= 4, f"{name}: the compiler reports {r['Occupancy']} waves per SIMD, 4 expected"
    assert any("icp_plane_solve_kernel" in k for k in res)
    normals = {k: v for k, v in res.items() if "icp_normals_kernel" in k}
    assert len(normals) == 1, sorted(res)
    for name, r in normals.items():
        assert r["ScratchSize"] == 0, f"{name}: {r['ScratchSize']} bytes of scratch (the candidate list belongs in LDS)"
        assert r["LDSByteSize"] >= 32 * 64 * 8, f"{name}: the candidate list is not in LDS ({r['LDSByteSize']} bytes)"
    for name, r in res.items():
        assert r["ScratchSize"] == 0, f"{name}: {r['ScratchSize']} bytes of scratch"
