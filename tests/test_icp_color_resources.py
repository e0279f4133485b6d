"""Register budget of the coloured ICP pass and the colour-gradient kernel (icp.hip), checked at compile time (no GPU), as
tests/test_icp_gicp_resources.py checks the generalized pass of the same file: the coloured pass carries the same 29
float64 sums and less pair arithmetic than the generalized pass - no scratch, and no fewer waves per SIMD than that pass
gets in the same compile; the gradient kernel walks its neighbour row without copying it - no scratch."""
import os

import pytest

from scorp_amd.build import HIPCC
from tests.test_kernel_resources import _resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_icp_colored_kernels_use_no_scratch_and_keep_the_generalized_pass_occupancy():
    res = _resources("icp.hip")
    colored = {k: v for k, v in res.items() if "icp_colored_pass_kernel" in k}
    grads = {k: v for k, v in res.items() if "icp_color_gradients_kernel" in k}
    gicp = {k: v for k, v in res.items() if "icp_generalized_pass_kernel" in k}
    assert len(colored) == 1 and len(grads) == 1 and len(gicp) == 1, sorted(res)
    (name, r), (gname, g), (_, p) = *colored.items(), *grads.items(), *gicp.items()
    print(f"{name}: {r['NumVgprs']} VGPRs, scratch {r['ScratchSize']}, occupancy {r['Occupancy']} (generalized pass: "
          f"{p['NumVgprs']} VGPRs, occupancy {p['Occupancy']}); {gname}: {g['NumVgprs']} VGPRs, scratch {g['ScratchSize']}, "
          f"occupancy {g['Occupancy']}")
    assert r["ScratchSize"] == 0, f"{name}: {r['ScratchSize']} bytes of scratch (spills in the pair arithmetic)"
    assert g["ScratchSize"] == 0, f"{gname}: {g['ScratchSize']} bytes of scratch (the neighbour row or the 3x3 Jacobi spilt)"
    assert r["Occupancy"] >= p["Occupancy"], f"{name}: {r['Occupancy']} waves per SIMD, the generalized pass has {p['Occupancy']}"
    assert any("icp_gather_intensity_kernel" in k for k in res)
