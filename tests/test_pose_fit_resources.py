"""Register budget of the pose-fit kernels (pose_fit.hip), checked at compile time (no GPU), as tests/test_icp_resources.py
checks the ICP's: no kernel of the file uses scratch - not the per-hypothesis fit with its 3x3 SVD in registers, and not
pose_adam_kernel, whose 14 parameters, 28 Adam moments and 3x3 temporaries all stay in the one wave's registers."""
import os

import pytest

from scorp_amd.build import HIPCC
from tests.test_kernel_resources import _resources

KERNELS = ("ransac_fit_kernel", "ransac_count_kernel", "ransac_select_kernel", "pose_sums_kernel", "pose_moments_kernel",
           "ransac_final_kernel", "pose_adam_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_pose_fit_kernels_use_no_scratch():
    res = _resources("pose_fit.hip")
    for frag in KERNELS:
        assert sum(frag in k for k in res) == 1, (frag, sorted(res))
    assert len(res) == len(KERNELS), sorted(res)
    for name, r in res.items():
        assert r["ScratchSize"] == 0, f"{name}: {r['ScratchSize']} bytes of scratch"
    count = next(r for k, r in res.items() if "ransac_count_kernel" in k)
    assert count["NumVgprs"] <= 64 and count["Occupancy"] >= 8   # the one kernel with a large grid (pairs x hypotheses)
