"""Register / LDS budgets of the late 2DGS iterations' kernels, checked at compile time (no GPU), with the bounds of
tests/test_view_terms_resources.py: the streaming kernels of surfel_terms.hip use no scratch and reach full occupancy, the
maps backward with the terms holds as many waves as the regularisers' instantiation, and the per-surfel backward with the
isotropic gradient stays within the plain kernel's budget."""
import os

import pytest

from scorp_amd.build import HIPCC
from tests.test_kernel_resources import _resources

KERNELS = ("surfel_terms_pass1_kernelILb0E", "surfel_terms_pass1_kernelILb1E", "surfel_terms_pass2_kernel",
           "isotropic2_value_kernel", "surfel_terms_finalize_kernel")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_surfel_terms_kernels_use_no_scratch_and_reach_full_occupancy():
    res = _resources("surfel_terms.hip")
    for frag in KERNELS:
        assert sum(frag in k for k in res) == 1, (frag, sorted(res))
    assert len(res) == len(KERNELS), sorted(res)
    for name, r in res.items():
        assert r["ScratchSize"] == 0, f"{name}: {r['ScratchSize']} bytes of scratch"
        assert r["NumVgprs"] <= 64 and r["Occupancy"] >= 8, (name, r)     # memory-bound passes: full occupancy


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_maps_backward_with_the_terms_keeps_the_regularisers_occupancy():
    res = _resources("gs2d_maps.hip")
    terms = [r for k, r in res.items() if "maps_backward_terms_kernel" in k]
    reg = [r for k, r in res.items() if "maps_backward_tiled_kernelILb1E" in k]
    assert len(terms) == 1 and len(reg) == 1, sorted(res)
    assert terms[0]["ScratchSize"] == 0
    assert terms[0]["Occupancy"] >= reg[0]["Occupancy"] and terms[0]["LDSByteSize"] <= reg[0]["LDSByteSize"], (terms, reg)


# (VGPRs, LDS bytes, waves per SIMD) of the two instantiations as they compiled before the tiled body took the kTerms
# parameter; they compile to the same figures with it
MAPS_BACKWARD_BEFORE = {"maps_backward_tiled_kernelILb0E": (25, 16032, 8), "maps_backward_tiled_kernelILb1E": (27, 20784, 7)}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_the_two_earlier_maps_backward_instantiations_keep_their_resources():
    res = _resources("gs2d_maps.hip")
    for frag, (vgprs, lds, waves) in MAPS_BACKWARD_BEFORE.items():
        r = [r for k, r in res.items() if frag in k]
        assert len(r) == 1, (frag, sorted(res))
        assert r[0]["ScratchSize"] == 0, (frag, r[0])
        assert r[0]["NumVgprs"] <= vgprs and r[0]["LDSByteSize"] <= lds and r[0]["Occupancy"] >= waves, (frag, r[0])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_isotropic_per_surfel_backward_uses_no_scratch_and_keeps_the_plain_kernels_budget():
    res = _resources("gs2d_pergaussian.hip")
    iso = {k: r for k, r in res.items() if "preprocess2d_backward_iso_kernel" in k}
    assert len(iso) == 4, sorted(res)
    for deg in range(4):
        k_iso = next(r for k, r in iso.items() if f"ILi{deg}E" in k)
        k_plain = next(r for k, r in res.items() if f"preprocess2d_backward_kernelILi{deg}ELb1E" in k)
        assert k_iso["ScratchSize"] == 0
        assert k_iso["NumVgprs"] <= k_plain["NumVgprs"] + 8 and k_iso["Occupancy"] >= k_plain["Occupancy"], (deg, k_iso, k_plain)
