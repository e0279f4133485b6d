"""Register budget of the mesh-distance kernels (mesh_distance.hip), checked at compile time (no GPU), as
tests/test_mesh_simplify_resources.py checks the vertex clustering's: every kernel is there exactly once under its name and
none uses scratch - the query kernel inlines the float64 closest-point construction and the ring walk without spilling.
(The file includes icp_search.hpp, so its copies of the ICP set-up kernels are there too; of those the bounding-box and scan
kernels use LDS, which is why LDS is not held to zero here.)"""
import os

import pytest

from scorp_amd.build import HIPCC
from tests.test_kernel_resources import _resources

KERNELS = ("mesh_pair_total_kernel", "mesh_grid_grow_kernel", "mesh_pair_count_kernel", "mesh_pair_fill_kernel",
           "mesh_miss_kernel", "mesh_query_kernel", "mesh_sample_kernel", "nearest_point_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_mesh_distance_kernels_use_no_scratch():
    res = _resources("mesh_distance.hip")
    for frag in KERNELS:
        assert sum(frag in k for k in res) == 1, (frag, sorted(res))
    for name, r in res.items():
        print(name, r)
        assert r["ScratchSize"] == 0, f"{name}: {r['ScratchSize']} bytes of scratch"
    own = {k: r for k, r in res.items() if any(frag in k for frag in KERNELS)}
    assert len(own) == len(KERNELS), sorted(own)
    for name, r in own.items():
        assert r["LDSByteSize"] == 0, f"{name}: {r['LDSByteSize']} bytes of LDS"
