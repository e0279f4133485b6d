"""Marching cubes through block borders (csrc/marching_cubes_blocks.hip) on hand-made volumes, no fusion, against the float64
yardstick (tests/marching_cubes_reference.marching_cubes_blocks): vertex count and every face index EQUAL, positions within
1e-5 voxel_length + 2 * 2^-23 max |coordinate| and colours within 2^-20 - the bounds of the surface-nets block tests, whose
vertices go through the same t, the same voxel_length ((g + 0.5) + t) and the same c0 + t (c1 - c0)."""
import functools

import numpy as np
import pytest
import torch

from tests import marching_cubes_reference as ref
from tests import tsdf_blocks_reference as blk

pytestmark = pytest.mark.gpu

CASES = ("sphere_8_blocks", "sphere_hole", "sphere_unseen_layer", "plane_in_block_face", "single_block", "tilted_plane_3x1x1")
FULL_BOXES = ("sphere_8_blocks", "plane_in_block_face", "single_block", "tilted_plane_3x1x1")


def _case(name):
    return ref.random_blocks() if name == "random" else blk.surface_cases()[name]


@functools.lru_cache(maxsize=None)
def _reference(name):
    return ref.marching_cubes_blocks(*_case(name))


def _volume(name, colour=True):
    from scorp_amd.mesh import BlockVolume, block_coords
    blocks, vl = _case(name)
    keys, tsdf, w, col = (torch.from_numpy(a).cuda() for a in blk.volume_arrays(blocks))
    return BlockVolume(keys, block_coords(keys), None, tsdf, w, col if colour else None, vl)


def _mesh(name, colour=True):
    from scorp_amd.mesh import extract_surface_blocks
    return extract_surface_blocks(_volume(name, colour), method="marching_cubes")


@pytest.mark.parametrize("name", CASES)
def test_surface_matches_the_yardstick(name):
    rv, rf, rc = _reference(name)
    vl = _case(name)[1]
    m = _mesh(name)
    v, f, c = m.vertices.cpu().numpy(), m.faces.cpu().numpy(), m.colors.cpu().numpy()
    assert len(v) == len(rv) > 0 and len(rf) > 0
    assert np.array_equal(f, rf)
    err, err_colour = float(np.abs(v - rv).max()), float(np.abs(c - rc).max())
    print(f"{name}: {len(v)} vertices, {len(f)} faces; position {err:.3e}, colour {err_colour:.3e}")
    assert err <= 1e-5 * vl + 2 * 2.0 ** -23 * np.abs(rv).max()
    assert err_colour <= 2.0 ** -20
    again = _mesh(name)
    assert torch.equal(again.vertices, m.vertices) and torch.equal(again.faces, m.faces) and torch.equal(again.colors, m.colors)
    plain = _mesh(name, colour=False)
    assert torch.equal(plain.vertices, m.vertices) and torch.equal(plain.faces, m.faces) and not bool(plain.colors.any())


def test_hole_and_unseen_layer_are_open_and_use_every_vertex():
    full = _mesh("sphere_8_blocks")
    assert ref.is_closed_and_oriented(full.faces.cpu().numpy())
    for name in ("sphere_hole", "sphere_unseen_layer"):
        m = _mesh(name)
        v, f = m.vertices.cpu().numpy(), m.faces.cpu().numpy()
        assert 0 < len(v) < full.vertices.shape[0] and not ref.is_closed_and_oriented(f)
        assert f.min() >= 0 and f.max() < len(v) and len(np.unique(f)) == len(v)


@pytest.mark.parametrize("name", FULL_BOXES)
def test_full_box_is_the_dense_mesh(name):
    from scorp_amd.mesh import extract_surface
    blocks, vl = _case(name)
    m = _mesh(name)
    T, g0 = blk.gather_dense(blocks)
    coords = [torch.from_numpy((vl * (np.arange(n) + g0[d] + 0.5)).astype(np.float32)).cuda() for d, n in enumerate(T.shape)]
    dv, df = extract_surface(torch.from_numpy(T).cuda(), coords, method="marching_cubes")
    v, f = ref.canonical(m.vertices.cpu().numpy(), m.faces.cpu().numpy())
    dv, df = ref.canonical(dv.cpu().numpy(), df.cpu().numpy())
    assert v.shape == dv.shape and f.shape == df.shape
    assert np.array_equal(v, dv) and np.array_equal(f, df)


def test_random_volume_has_every_case_and_is_closed():
    blocks, vl = ref.random_blocks()
    T, _ = blk.gather_dense(blocks)
    assert len(np.unique(ref.cell_cases(T))) == 256
    rv, rf, rc = _reference("random")
    m = _mesh("random")
    v, f, c = m.vertices.cpu().numpy(), m.faces.cpu().numpy(), m.colors.cpu().numpy()
    assert len(v) == len(rv) and np.array_equal(f, rf)
    assert np.abs(v - rv).max() <= 1e-5 * vl + 2 * 2.0 ** -23 * np.abs(rv).max()
    assert np.abs(c - rc).max() <= 2.0 ** -20
    assert ref.is_closed_and_oriented(f) and len(np.unique(f)) == len(v)
