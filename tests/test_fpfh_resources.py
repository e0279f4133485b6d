"""Register budget of the global-registration kernels (cloud_fpfh.hip, feature_match.hip), checked at compile time (no
GPU): every kernel is there exactly once under its name and none uses scratch - the k-best list of the search lives in LDS
sized at the launch, never in a runtime-indexed per-thread array, and the match kernel's 33 source values stay in
registers.  Static LDS only where the design has it: the 7 x 33 sums of the FPFH kernel and the match kernel's tile."""
import os

import pytest

from scorp_amd.build import HIPCC
from scorp_amd.global_registration import FPFH_DIM, MATCH_TILE
from tests.test_kernel_resources import _resources

# kernel: static LDS bytes
FPFH_KERNELS = {"cloud_gather_kernel": 0, "fpfh_search_kernel": 0, "fpfh_spfh_kernel": 0, "fpfh_feature_kernel": (256 // FPFH_DIM) * FPFH_DIM * 8}
MATCH_KERNELS = {"feature_match_kernel": MATCH_TILE * (FPFH_DIM + 1) * 8, "feature_match_merge_kernel": 0}


def _check(src, kernels, select, vgprs):
    res = {k: r for k, r in _resources(src).items() if select(k)}
    for frag in kernels:
        assert sum(frag in k for k in res) == 1, (frag, sorted(res))
    assert len(res) == len(kernels), sorted(res)
    for name, r in res.items():
        print(name, r)
        lds = next(v for frag, v in kernels.items() if frag in name)
        assert r["ScratchSize"] == 0, f"{name}: {r['ScratchSize']} bytes of scratch"
        assert r["LDSByteSize"] == lds, f"{name}: {r['LDSByteSize']} bytes of static LDS, {lds} expected"
        assert r["NumVgprs"] <= vgprs, f"{name}: {r['NumVgprs']} VGPRs (fewer than 4 waves per SIMD)"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_fpfh_kernels_use_no_scratch():
    _check("cloud_fpfh.hip", FPFH_KERNELS, lambda k: "fpfh_" in k or "cloud_" in k, 128)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_match_kernels_use_no_scratch():
    _check("feature_match.hip", MATCH_KERNELS, lambda k: "feature_match" in k, 128)
