"""Register budget of the ICP kernels (icp.hip), checked at compile time (no GPU), as tests/test_kernel_resources.py checks
the blend kernels': the correspondence pass keeps its 17 float64 sums and the ring search in registers - no scratch, at
most 96 VGPRs (five waves per SIMD) - and no kernel of the file spills."""
import os

import pytest

from scorp_amd.build import HIPCC
from tests.test_kernel_resources import _resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_icp_kernels_keep_their_occupancy():
    res = _resources("icp.hip")
    search = {k: v for k, v in res.items() if "icp_pass_kernel" in k}
    assert len(search) == 1, sorted(res)
    for name, r in search.items():
        assert r["ScratchSize"] == 0, f"{name}: {r['ScratchSize']} bytes of scratch (spills in the search loop)"
        assert r["NumVgprs"] <= 96, f"{name}: {r['NumVgprs']} VGPRs > 96"
        assert r["Occupancy"] >= 5, f"{name}: the compiler reports {r['Occupancy']} waves per SIMD, 5 expected"
    assert any("icp_solve_kernel" in k for k in res)
    for name, r in res.items():
        assert r["ScratchSize"] == 0, f"{name}: {r['ScratchSize']} bytes of scratch"
