"""Register / LDS budget of the mask-vote kernel (mask_vote.hip), checked at compile time (no GPU), as
tests/test_kernel_resources.py checks the blend kernels': no scratch (no spills in the hit loop), at most 128 VGPRs and
10 KiB of LDS per wave, so that four waves per SIMD fit (the LDS holds 160 KiB per CU)."""
import os

import pytest

from scorp_amd.build import HIPCC
from tests.test_kernel_resources import _resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_mask_vote_kernels_keep_their_occupancy():
    res = _resources("mask_vote.hip")
    kernels = {k: v for k, v in res.items() if "mask_vote_wave_kernel" in k}
    assert len(kernels) == 2, sorted(res)   # the 3DGS and the 2DGS replay
    for name, r in kernels.items():
        assert r["ScratchSize"] == 0, f"{name}: {r['ScratchSize']} bytes of scratch (spills in the hit loop)"
        assert r["NumVgprs"] <= 128, f"{name}: {r['NumVgprs']} VGPRs > 128"
        assert r["LDSByteSize"] <= 160 * 1024 // 16, f"{name}: {r['LDSByteSize']} bytes of LDS > 10 KiB"
        assert r["Occupancy"] >= 4, f"{name}: the compiler reports {r['Occupancy']} waves per SIMD, 4 expected"
    epi = {k: v for k, v in res.items() if "vote_epilogue_kernel" in k}
    assert epi and all(v["ScratchSize"] == 0 for v in epi.values())
