"""Register budget of the vertex-clustering kernels (mesh_simplify.hip), checked at compile time (no GPU), as
tests/test_mesh_cluster_resources.py checks the triangle clustering's: every kernel is there exactly once under its name and
none uses scratch - the place kernel inlines the 3x3 float64 SVD of svd3.hpp without spilling - or LDS."""
import os

import pytest

from scorp_amd.build import HIPCC
from tests.test_kernel_resources import _resources

KERNELS = ("simplify_init_kernel", "simplify_cells_kernel", "simplify_roots_kernel", "simplify_vertex_sums_kernel",
           "simplify_quadrics_kernel", "simplify_place_kernel", "simplify_faces_remap_kernel", "simplify_faces_insert_kernel",
           "simplify_faces_keep_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_mesh_simplify_kernels_use_no_scratch():
    res = _resources("mesh_simplify.hip")
    for frag in KERNELS:
        assert sum(frag in k for k in res) == 1, (frag, sorted(res))
    assert len(res) == len(KERNELS), sorted(res)
    for name, r in res.items():
        assert r["ScratchSize"] == 0, f"{name}: {r['ScratchSize']} bytes of scratch"
        assert r["LDSByteSize"] == 0, f"{name}: {r['LDSByteSize']} bytes of LDS"
