"""Register budget of the mesh-render kernels (mesh_render.hip), checked at compile time (no GPU), as
tests/test_mesh_distance_resources.py checks the mesh distance's: every kernel is there exactly once under its name, none
uses scratch (the triangle set-up travels in registers through all three kernels that need it) and none uses LDS.  The
two constants the fixtures build their block-edge cases on are read from the source."""
import os
import re

import pytest

from scorp_amd.build import CSRC, HIPCC
from tests import mesh_render_fixtures as fx
from tests.test_kernel_resources import _resources

KERNELS = ("mesh_render_project_kernel", "mesh_render_small_kernel", "mesh_render_large_kernel", "mesh_render_resolve_kernel",
           "mesh_render_count_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_mesh_render_kernels_use_no_scratch_and_no_lds():
    res = _resources("mesh_render.hip")
    for frag in KERNELS:
        assert sum(frag in k for k in res) == 1, (frag, sorted(res))
    assert len(res) == len(KERNELS), sorted(res)
    for name, r in res.items():
        print(name, r)
        assert r["ScratchSize"] == 0, f"{name}: {r['ScratchSize']} bytes of scratch"
        assert r["LDSByteSize"] == 0, f"{name}: {r['LDSByteSize']} bytes of LDS"


def test_the_fixtures_know_the_kernels_constants():
    text = open(os.path.join(CSRC, "mesh_render.hip")).read()
    assert int(re.search(r"kMeshRenderLargeGroups = (\d+);", text).group(1)) == fx.LARGE_GROUPS
    assert int(re.search(r"kMeshRenderSmallBox = (\d+);", text).group(1)) == fx.SMALL_BOX
    assert int(re.search(r"kMeshRenderThreads = (\d+);", text).group(1)) == 256 and 256 in fx.COUNT_EDGES
