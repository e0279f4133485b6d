"""Register budget of the cloud kernels (cloud_filter.hip), checked at compile time (no GPU): every kernel is there exactly
once under its name, none uses scratch (the k-best list of the k-nearest kernel lives in LDS sized at the launch, never in
a runtime-indexed per-thread array), and none holds static LDS."""
import os

import pytest

from scorp_amd.build import HIPCC
from tests.test_kernel_resources import _resources

KERNELS = ("cloud_gather_kernel", "cloud_knn_kernel", "cloud_count_kernel", "cloud_link_kernel", "cloud_roots_kernel",
           "cloud_border_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_cloud_kernels_use_no_scratch():
    res = {k: r for k, r in _resources("cloud_filter.hip").items() if "cloud_" in k}
    for frag in KERNELS:
        assert sum(frag in k for k in res) == 1, (frag, sorted(res))
    assert len(res) == len(KERNELS), sorted(res)
    for name, r in res.items():
        print(name, r)
        assert r["ScratchSize"] == 0, f"{name}: {r['ScratchSize']} bytes of scratch"
        assert r["LDSByteSize"] == 0, f"{name}: {r['LDSByteSize']} bytes of static LDS"
        assert r["NumVgprs"] <= 128, f"{name}: {r['NumVgprs']} VGPRs (fewer than 4 waves per SIMD)"
