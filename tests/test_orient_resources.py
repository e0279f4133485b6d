"""Register budget of the normal-orientation kernels (cloud_orient.hip), checked at compile time (no GPU): every kernel is
there exactly once under its name, none uses scratch (no kernel keeps a per-thread array: a row of the neighbour list is
walked entry by entry) and none needs more than 128 VGPRs.  Static LDS only where the design has it: the 256 x 3 partial
sums of the default centre."""
import os

import pytest

from scorp_amd.build import HIPCC
from tests.test_kernel_resources import _resources

# kernel: static LDS bytes
ORIENT_KERNELS = {"orient_init_kernel": 0, "orient_center_partial_kernel": 0, "orient_center_kernel": 256 * 3 * 8,
                  "orient_weight_kernel": 0, "orient_edge_kernel": 0, "orient_hook_kernel": 0,
                  "orient_compress_kernel": 0, "orient_label_kernel": 0, "orient_vote_kernel": 0, "orient_output_kernel": 0}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_orient_kernels_use_no_scratch():
    res = _resources("cloud_orient.hip")
    for frag in ORIENT_KERNELS:
        assert sum(frag in k for k in res) == 1, (frag, sorted(res))
    assert len(res) == len(ORIENT_KERNELS), sorted(res)
    for name, r in res.items():
        print(name, r)
        lds = next(v for frag, v in ORIENT_KERNELS.items() if frag in name)
        assert r["ScratchSize"] == 0, f"{name}: {r['ScratchSize']} bytes of scratch"
        assert r["LDSByteSize"] == lds, f"{name}: {r['LDSByteSize']} bytes of static LDS, {lds} expected"
        assert r["NumVgprs"] <= 128, f"{name}: {r['NumVgprs']} VGPRs (fewer than 4 waves per SIMD)"
