"""The block-volume kernels (csrc/tsdf_blocks.hip) against the float64 yardstick (tests/tsdf_blocks_reference.py) on the scene of
tests/test_tsdf_blocks_cpu.py, whose docstring says what the scene is and how the decisions too close to call are treated:
block keys and view masks EQUAL in every bit the yardstick can call (they are integers, independent of the execution
order), weights EQUAL on the kept voxels, tsdf within 4 e_ref and colour within 4 e_ref_colour, both e_ref evaluated here on
the CPU.  Then the table's edges: one key from every lane, a table that is just large enough, one that is too small."""
import ctypes

import numpy as np
import pytest
import torch

from tests import tsdf_blocks_reference as ref
from tests.test_tsdf_blocks_cpu import _fuse

pytestmark = pytest.mark.gpu

CASES = [dict(), dict(num_views=1), dict(num_views=33), dict(blank_view=2), dict(shift=(-7.0, -7.0, -7.0))]


def _numpy(vol):
    return (vol.keys.cpu().numpy(), vol.view_mask.cpu().numpy(), vol.tsdf.cpu().numpy(), vol.weight.cpu().numpy(),
            vol.colour.cpu().numpy() if vol.colour is not None else None)


@pytest.fixture(scope="module")
def fused():
    assert torch.cuda.is_available()
    return _fuse(*ref.inputs(), device="cuda:0")


@pytest.mark.parametrize("kw", CASES, ids=str)
def test_kernels_match_the_float64_yardstick(kw):
    """V = 33 repeats the five views, so the mask needs a second word; blank_view: a view that sees nothing; shift: every
    block at negative coordinates."""
    c = ref.case(**kw)
    vol = _fuse(*ref.inputs(**kw), device="cuda:0")
    keys, mask, tsdf, weight, colour = _numpy(vol)
    err, err_colour = ref.compare_volume(c, keys, mask, tsdf, weight, colour)
    print(f"{kw}: {keys.size} blocks; tsdf {err:.3e} (e_ref {c['e_ref']:.3e}), colour {err_colour:.3e} (e_ref_colour {c['e_ref_colour']:.3e})")
    assert mask.shape[1] == (ref.inputs(**kw)[0].shape[0] + 31) // 32
    if kw.get("blank_view") is not None:
        assert not (mask[:, 0] >> kw["blank_view"] & 1).any()
    if kw.get("shift"):
        assert vol.coords.max().item() < 0


def test_volume_without_colour(fused):
    depth, _, cam = ref.inputs()
    vol = _fuse(depth, None, cam, device="cuda:0")
    assert vol.colour is None and torch.equal(vol.tsdf, fused.tsdf) and torch.equal(vol.weight, fused.weight)


def test_every_lane_inserts_the_same_key():
    depth, rgb, cam, vl, trunc, stride = ref.one_block_inputs()
    vol = _fuse(depth, rgb, cam, vl, trunc, stride, device="cuda:0")
    assert vol.keys.tolist() == [ref.key_of((0, 0, 0))] and vol.view_mask.tolist() == [[1]]
    ref.compare_volume(ref.fuse_case(depth, rgb, cam, vl, trunc, stride), *_numpy(vol))
    one_slot = _fuse(depth, rgb, cam, vl, trunc, stride, device="cuda:0", num_slots=1)   # the smallest table there is
    assert torch.equal(one_slot.keys, vol.keys) and torch.equal(one_slot.tsdf, vol.tsdf)


def _touch(num_slots, guard=64):
    """scorp_tsdf_blocks_touch on the scene with a table of num_slots inside larger buffers: (keys, masks, overflow word,
    guards intact)."""
    from scorp_amd import _C
    depth, rgb, cam = (torch.from_numpy(a).cuda() for a in ref.inputs())
    V, H, W = depth.shape
    keys = torch.full((num_slots + 2 * guard,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    mask = torch.full((num_slots + 2 * guard,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    over = torch.full((1 + 2 * guard,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    views = _C.ScorpTsdfBlockViews(depth=depth.data_ptr(), rgb=rgb.data_ptr(), cam=cam.data_ptr(), num_views=V, width=W, height=H)
    rc = _C.lib().scorp_tsdf_blocks_touch(ctypes.byref(views), ref.VOXEL, ref.TRUNC, ref.STRIDE, keys[guard:].data_ptr(),
                                         mask[guard:].data_ptr(), num_slots, over[guard:].data_ptr(), _C.current_stream_ptr())
    assert rc == 0, _C.lib().scorp_last_error()
    torch.cuda.synchronize()
    intact = all(bool((t[:guard] == 0x5A5A5A5A).all()) and bool((t[guard + n:] == 0x5A5A5A5A).all())
                 for t, n in ((keys, num_slots), (mask, num_slots), (over, 1)))
    k, m = keys[guard:guard + num_slots], mask[guard:guard + num_slots]
    taken = k != -1
    k, order = torch.sort(k[taken])
    return k, m[taken][order], int(over[guard]), intact


def test_table_of_the_smallest_size_that_holds_the_blocks(fused):
    B = fused.keys.numel()
    slots = 1 << (B - 1).bit_length()   # 98 blocks in 128 slots: long probe runs, and runs that wrap past the end
    assert slots // 2 < B <= slots
    keys, mask, overflow, intact = _touch(slots)
    assert overflow == 0 and intact
    assert torch.equal(keys, fused.keys) and torch.equal(mask, fused.view_mask[:, 0])


def test_table_that_is_too_small(fused):
    B = fused.keys.numel()
    slots = 1 << (B - 1).bit_length() - 1
    assert slots < B
    keys, mask, overflow, intact = _touch(slots)   # the call returns: probing is bounded by the table's size
    assert overflow == 1 and intact
    assert keys.numel() == slots                   # every slot taken, each by a block of the scene, with bits of its mask only
    at = torch.searchsorted(fused.keys, keys)
    assert torch.equal(fused.keys[at], keys) and not bool((mask & ~fused.view_mask[at, 0]).any())
    retried = _fuse(*ref.inputs(), device="cuda:0", num_slots=slots)   # the Python layer doubles the table and repeats
    for a, b in ((retried.keys, fused.keys), (retried.view_mask, fused.view_mask), (retried.tsdf, fused.tsdf),
                 (retried.weight, fused.weight), (retried.colour, fused.colour)):
        assert torch.equal(a, b)


def test_two_calls_give_identical_bits(fused):
    again = _fuse(*ref.inputs(), device="cuda:0")
    for a, b in ((again.keys, fused.keys), (again.view_mask, fused.view_mask), (again.tsdf, fused.tsdf), (again.weight, fused.weight),
                 (again.colour, fused.colour), (again.coords, fused.coords)):
        assert torch.equal(a, b)


def test_neighbour_table(fused):
    from scorp_amd.mesh import block_neighbors
    nbr = block_neighbors(fused.keys).cpu().numpy()
    rank = {ref.coords_of(int(k)): r for r, k in enumerate(fused.keys.cpu().numpy())}
    want = np.array([[rank.get((b[0] + dx, b[1] + dy, b[2] + dz), -1) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1)]
                     for b in rank], np.int32)
    assert np.array_equal(nbr, want) and (want == -1).any() and np.array_equal(nbr, block_neighbors(fused.keys.cpu()).numpy())
