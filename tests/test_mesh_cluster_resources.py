"""Register budget of the triangle-clustering kernels (mesh_cluster.hip), checked at compile time (no GPU), as
tests/test_mesh_resources.py checks the other mesh kernels': every kernel is there exactly once under its name, none uses
scratch, and only the stats kernel - the one that combines a wave's lanes before its atomics - may hold LDS."""
import os

import pytest

from scorp_amd.build import HIPCC
from tests.test_kernel_resources import _resources

KERNELS = ("cluster_init_kernel", "cluster_link_kernel", "cluster_roots_kernel", "cluster_stats_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_mesh_cluster_kernels_use_no_scratch():
    res = _resources("mesh_cluster.hip")
    for frag in KERNELS:
        assert sum(frag in k for k in res) == 1, (frag, sorted(res))
    assert len(res) == len(KERNELS), sorted(res)
    for name, r in res.items():
        assert r["ScratchSize"] == 0, f"{name}: {r['ScratchSize']} bytes of scratch"
        if "cluster_stats_kernel" not in name:
            assert r["LDSByteSize"] == 0, f"{name}: {r['LDSByteSize']} bytes of LDS"
