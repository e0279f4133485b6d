"""Register budget of the mesh kernels (tsdf.hip, isosurface.hip), checked at compile time (no GPU), as
tests/test_pose_fit_resources.py checks the pose fit's: every kernel is there exactly once, none uses scratch, and the
no-colour fusion kernel - the one with a 10^9-lane grid, about 20 live values - keeps 8 waves per SIMD."""
import os

import pytest

from scorp_amd.build import HIPCC
from tests.test_kernel_resources import _resources

TSDF = ("tsdf_fuse_kernelILb0ELb0EE", "tsdf_fuse_kernelILb0ELb1EE", "tsdf_fuse_kernelILb1ELb0EE", "tsdf_fuse_kernelILb1ELb1EE")
ISO = ("iso_count_cells_kernel", "iso_emit_vertices_kernel", "iso_count_faces_kernel", "iso_emit_faces_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("src, kernels", [("tsdf.hip", TSDF), ("isosurface.hip", ISO)])
def test_mesh_kernels_use_no_scratch(src, kernels):
    res = _resources(src)
    for frag in kernels:
        assert sum(frag in k for k in res) == 1, (frag, sorted(res))
    assert len(res) == len(kernels), sorted(res)
    for name, r in res.items():
        assert r["ScratchSize"] == 0, f"{name}: {r['ScratchSize']} bytes of scratch"
        assert r["LDSByteSize"] == 0, f"{name}: {r['LDSByteSize']} bytes of LDS"
    if src == "tsdf.hip":
        for name, r in res.items():
            if "ILb0E" in name.split("tsdf_fuse_kernel")[1][:5]:   # <kRgb = false, ...>
                assert r["NumVgprs"] <= 64 and r["Occupancy"] >= 8, (name, r)
