"""Resources of the block-volume kernels (tsdf_blocks.hip, isosurface_blocks.hip), checked at compile time (no GPU), as
tests/test_mesh_cluster_resources.py checks the clustering kernels': every kernel is there exactly once under its name, none
uses scratch, none holds LDS - the neighbour row of a block is 27 integers at a workgroup-uniform address, and no kernel
stages it - and each stays within 64 VGPRs, the most at which a SIMD of gfx950 (512 VGPRs a lane) still holds 8 waves:
these kernels hide gather latency with waves in flight, not with unrolling."""
import os

import pytest

from scorp_amd.build import HIPCC
from tests.test_kernel_resources import _resources

KERNELS = {
    "tsdf_blocks.hip": ("blocks_clear_kernel", "blocks_touch_kernel", "blocks_neighbors_kernel", "blocks_integrate_kernel"),
    "isosurface_blocks.hip": ("iso_blocks_count_cells_kernel", "iso_blocks_emit_vertices_kernel", "iso_blocks_count_faces_kernel",
                              "iso_blocks_emit_faces_kernel"),
}
LDS_KERNELS = ()   # the kernels that may hold LDS: none
MAX_VGPRS, MIN_WAVES = 64, 8


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("src", sorted(KERNELS))
def test_block_kernels_use_no_scratch_and_no_lds(src):
    res = _resources(src)
    for frag in KERNELS[src]:
        assert sum(frag in k for k in res) == 1, (frag, sorted(res))
    assert len(res) == len(KERNELS[src]), sorted(res)
    for name, r in res.items():
        print(f"{name}: {r}")
        assert r["ScratchSize"] == 0, f"{name}: {r['ScratchSize']} bytes of scratch"
        assert r["NumVgprs"] <= MAX_VGPRS and r["Occupancy"] >= MIN_WAVES, f"{name}: {r['NumVgprs']} VGPRs, {r['Occupancy']} waves per SIMD"
        if not any(frag in name for frag in LDS_KERNELS):
            assert r["LDSByteSize"] == 0, f"{name}: {r['LDSByteSize']} bytes of LDS"
