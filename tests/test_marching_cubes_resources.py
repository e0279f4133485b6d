"""Resources of the marching-cubes kernels (marching_cubes.hip, marching_cubes_blocks.hip), checked at compile time (no GPU) as
tests/test_mesh_resources.py checks the surface-nets kernels': each of the eight kernels is there exactly once, and none uses
scratch - the table row is read by one vector load and taken apart with constant shifts, the (corner, axis) of an edge id
comes out of a packed immediate, so nothing is indexed at run time."""
import os

import pytest

from scorp_amd.build import HIPCC
from tests.test_kernel_resources import _resources

KERNELS = {
    "marching_cubes.hip": ("mc_count_edges_kernel", "mc_emit_vertices_kernel", "mc_count_faces_kernel", "mc_emit_faces_kernel"),
    "marching_cubes_blocks.hip": ("mc_blocks_count_edges_kernel", "mc_blocks_emit_vertices_kernel", "mc_blocks_count_faces_kernel",
                                  "mc_blocks_emit_faces_kernel"),
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("src", sorted(KERNELS))
def test_marching_cubes_kernels_use_no_scratch(src):
    res = _resources(src)
    for frag in KERNELS[src]:
        assert sum(frag in k for k in res) == 1, (frag, sorted(res))
    assert len(res) == len(KERNELS[src]), sorted(res)
    for name, r in res.items():
        print(f"{name}: {r}")
        assert r["ScratchSize"] == 0, f"{name}: {r['ScratchSize']} bytes of scratch"
