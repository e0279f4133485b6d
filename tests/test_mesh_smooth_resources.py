"""Register budget of the mesh-smooth kernels (mesh_smooth.hip), checked at compile time (no GPU), as
tests/test_mesh_distance_resources.py checks the mesh distance's: each of the four kernels is there exactly once under its
name, and none uses scratch (the neighbour and the corner walks are plain loops over the CSR, with no array a thread could
spill) or LDS.  The block size the strip fixtures are built on is read from the source."""
import os
import re

import pytest

from scorp_amd.build import CSRC, HIPCC
from tests import mesh_smooth_fixtures as fx
from tests.test_kernel_resources import _resources

KERNELS = ("mesh_face_normals_kernel", "mesh_vertex_normals_kernel", "mesh_smooth_step_kernel", "mesh_normal_map_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_mesh_smooth_kernels_use_no_scratch_and_no_lds():
    res = _resources("mesh_smooth.hip")
    for frag in KERNELS:
        assert sum(frag in k for k in res) == 1, (frag, sorted(res))
    assert len(res) == len(KERNELS), sorted(res)
    for name, r in res.items():
        print(name, r)
        assert r["ScratchSize"] == 0, f"{name}: {r['ScratchSize']} bytes of scratch"
        assert r["LDSByteSize"] == 0, f"{name}: {r['LDSByteSize']} bytes of LDS"


def test_the_fixtures_know_the_kernels_block_size():
    text = open(os.path.join(CSRC, "mesh_smooth.hip")).read()
    assert int(re.search(r"kMeshSmoothThreads = (\d+);", text).group(1)) == fx.BLOCK
    verts = {len(fx.fixture(f"strip{n}")[0]) for n in fx.STRIP_VERTICES}
    faces = {len(fx.fixture(f"strip{n}")[1]) for n in fx.STRIP_VERTICES}
    assert {fx.BLOCK - 1, fx.BLOCK, fx.BLOCK + 1} <= verts and {fx.BLOCK - 1, fx.BLOCK, fx.BLOCK + 1} <= faces
