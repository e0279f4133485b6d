"""Register budget of the decimation kernels (mesh_decimate.hip), checked at compile time (no GPU), as
tests/test_mesh_simplify_resources.py checks the vertex clustering's: every kernel is there exactly once under its name and
none uses scratch - the candidate kernel holds a quadric, three points and the cofactors in registers - or LDS."""
import os

import pytest

from scorp_amd.build import HIPCC
from tests.test_kernel_resources import _resources

KERNELS = ("decimate_quadrics_kernel", "decimate_flags_kernel", "decimate_candidates_kernel", "decimate_hash_kernel",
           "decimate_vmin_init_kernel", "decimate_vmin_kernel", "decimate_vmin2_kernel", "decimate_select_kernel",
           "decimate_identity_kernel", "decimate_apply_kernel", "decimate_faces_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_mesh_decimate_kernels_use_no_scratch():
    res = _resources("mesh_decimate.hip")
    for frag in KERNELS:
        assert sum(frag in k for k in res) == 1, (frag, sorted(res))
    assert len(res) == len(KERNELS), sorted(res)
    for name, r in res.items():
        assert r["ScratchSize"] == 0, f"{name}: {r['ScratchSize']} bytes of scratch"
        assert r["LDSByteSize"] == 0, f"{name}: {r['LDSByteSize']} bytes of LDS"
