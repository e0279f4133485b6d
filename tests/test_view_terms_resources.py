"""Register budget of the late iterations' loss-term kernels (depth_terms.hip), checked at compile time (no GPU), as
tests/test_pose_fit_resources.py checks the pose fit's: four streaming kernels, none of which uses scratch."""
import os

import pytest

from scorp_amd.build import HIPCC
from tests.test_kernel_resources import _resources

KERNELS = ("depth_terms_pass1_kernel", "depth_terms_pass2_kernel", "isotropic_value_kernel", "view_terms_finalize_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_view_terms_kernels_use_no_scratch():
    res = _resources("depth_terms.hip")
    for frag in KERNELS:
        assert sum(frag in k for k in res) == 1, (frag, sorted(res))
    assert len(res) == len(KERNELS), sorted(res)
    for name, r in res.items():
        assert r["ScratchSize"] == 0, f"{name}: {r['ScratchSize']} bytes of scratch"
        assert r["NumVgprs"] <= 64 and r["Occupancy"] >= 8, (name, r)     # memory-bound passes: full occupancy


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_isotropic_per_gaussian_backward_uses_no_scratch_and_keeps_the_plain_kernels_budget():
    """The per-Gaussian backward with the isotropic gradient is a separate instantiation: no scratch, and no more registers
    than the plain kernel of the same SH degree (training layout)."""
    res = _resources("gs3d_pergaussian.hip")
    iso = {k: r for k, r in res.items() if "preprocess_backward_iso_kernel" in k}
    assert len(iso) == 4, sorted(res)
    for deg in range(4):
        k_iso = next(r for k, r in iso.items() if f"ILi{deg}E" in k)
        k_plain = next(r for k, r in res.items() if f"preprocess_backward_kernelILi{deg}ELb1E" in k)
        assert k_iso["ScratchSize"] == 0
        assert k_iso["NumVgprs"] <= k_plain["NumVgprs"] + 8 and k_iso["Occupancy"] >= k_plain["Occupancy"], (deg, k_iso, k_plain)
