"""Surface nets through block borders (csrc/isosurface_blocks.hip) on hand-made volumes, no fusion, against the float64
yardstick (tests/tsdf_blocks_reference.surface_blocks, itself held to the dense extractor in tests/test_tsdf_blocks_cpu.py):
vertex count and every face index EQUAL, positions within 1e-5 voxel_length + 2 * 2^-23 max |coordinate| (the dense test's
bound plus the two roundings of voxel_length ((g + 0.5) + frac)), colours within 2^-20.  On a full box with every weight
positive the mesh is, bit for bit, the dense extract_surface's of the gathered grid (voxel_length is a power of two there, so
that x[i] + frac (x[i + 1] - x[i]) and voxel_length ((g + 0.5) + frac) round alike)."""
import functools

import numpy as np
import pytest
import torch

from tests import tsdf_blocks_reference as ref

pytestmark = pytest.mark.gpu

CASES = ("sphere_8_blocks", "sphere_hole", "sphere_unseen_layer", "plane_in_block_face", "single_block", "tilted_plane_3x1x1")
FULL_BOXES = ("sphere_8_blocks", "plane_in_block_face", "single_block", "tilted_plane_3x1x1")


@functools.lru_cache(maxsize=None)
def _reference(name):
    blocks, vl = ref.surface_cases()[name]
    return ref.surface_blocks(blocks, vl)


def _volume(name, colour=True):
    from scorp_amd.mesh import BlockVolume, block_coords
    blocks, vl = ref.surface_cases()[name]
    keys, tsdf, w, col = (torch.from_numpy(a).cuda() for a in ref.volume_arrays(blocks))
    return BlockVolume(keys, block_coords(keys), None, tsdf, w, col if colour else None, vl)


@pytest.mark.parametrize("name", CASES)
def test_surface_matches_the_yardstick(name):
    from scorp_amd.mesh import extract_surface_blocks
    rv, rf, rc = _reference(name)
    vl = ref.surface_cases()[name][1]
    m = extract_surface_blocks(_volume(name))
    v, f, c = m.vertices.cpu().numpy(), m.faces.cpu().numpy(), m.colors.cpu().numpy()
    assert len(v) == len(rv) > 0 and len(rf) > 0
    assert np.array_equal(f, rf)
    err, err_colour = float(np.abs(v - rv).max()), float(np.abs(c - rc).max())
    print(f"{name}: {len(v)} vertices, {len(f)} faces; position {err:.3e}, colour {err_colour:.3e}")
    assert err <= 1e-5 * vl + 2 * 2.0 ** -23 * np.abs(rv).max()
    assert err_colour <= 2.0 ** -20
    again = extract_surface_blocks(_volume(name))
    assert torch.equal(again.vertices, m.vertices) and torch.equal(again.faces, m.faces) and torch.equal(again.colors, m.colors)
    plain = extract_surface_blocks(_volume(name, colour=False))
    assert torch.equal(plain.vertices, m.vertices) and torch.equal(plain.faces, m.faces) and not bool(plain.colors.any())


def test_hole_and_unseen_layer_remove_what_touches_them():
    """A missing block or an unwritten voxel layer makes every cell with a corner there invalid.  On the kernels' meshes: fewer
    vertices than the full sphere, an open rim (edges with one triangle) where the full sphere is closed, no vertex in the
    removed block past the cells that reach into it, none in the cells that have a corner in the unwritten layer, and
    every face index a vertex."""
    from scorp_amd.mesh import extract_surface_blocks
    from tests.isosurface_reference import is_closed_and_oriented
    vl = ref.SURFACE_VOXEL
    mesh = lambda name: [t.cpu().numpy() for t in (lambda m: (m.vertices, m.faces))(extract_surface_blocks(_volume(name)))]
    full_v, full_f = mesh("sphere_8_blocks")
    assert is_closed_and_oriented(full_f)
    for name in ("sphere_hole", "sphere_unseen_layer"):
        v, f = mesh(name)
        assert 0 < len(v) < len(full_v) and not is_closed_and_oriented(f)
        assert f.min() >= 0 and f.max() < len(v) and len(np.unique(f)) == len(v)   # every vertex is used, every index is one
        if name == "sphere_hole":   # block (0, -1, 0): cells g.x in [-1, 15], g.y in [-17, -1], g.z in [-1, 15] have a corner in it
            gone = (v[:, 0] > 0.5 * vl) & (v[:, 1] < -0.5 * vl) & (v[:, 2] > 0.5 * vl)
        else:                       # voxel layer g.y = 3: the cells g.y in (2, 3), vertices at y in [2.5, 4.5] voxel_length
            gone = (v[:, 1] > 2.5 * vl) & (v[:, 1] < 4.5 * vl)
        assert not gone.any(), name
        full_gone = ((full_v[:, 0] > 0.5 * vl) & (full_v[:, 1] < -0.5 * vl) & (full_v[:, 2] > 0.5 * vl)) if name == "sphere_hole" \
            else ((full_v[:, 1] > 2.5 * vl) & (full_v[:, 1] < 4.5 * vl))
        assert full_gone.any(), name   # (the full sphere does have vertices there)


@pytest.mark.parametrize("name", FULL_BOXES)
def test_full_box_is_the_dense_extractor_bit_for_bit(name):
    from scorp_amd.mesh import extract_surface, extract_surface_blocks
    blocks, vl = ref.surface_cases()[name]
    m = extract_surface_blocks(_volume(name))
    T, g0 = ref.gather_dense(blocks)
    coords = [torch.from_numpy((vl * (np.arange(n) + g0[d] + 0.5)).astype(np.float32)).cuda() for d, n in enumerate(T.shape)]
    dv, df = extract_surface(torch.from_numpy(T).cuda(), coords)
    v, f, dv, df = m.vertices.cpu().numpy(), m.faces.cpu().numpy(), dv.cpu().numpy(), df.cpu().numpy()
    assert v.shape == dv.shape and f.shape == df.shape
    order, dense_order = np.lexsort(v.T[::-1]), np.lexsort(dv.T[::-1])
    assert np.array_equal(v[order], dv[dense_order])
    assert len(np.unique(v, axis=0)) == len(v)            # no two vertices share a position: the sorted orders correspond
    rank, dense_rank = np.empty(len(v), np.int64), np.empty(len(v), np.int64)
    rank[order], dense_rank[dense_order] = np.arange(len(v)), np.arange(len(v))
    rows = lambda a: a[np.lexsort(a[:, ::-1].T)]
    assert np.array_equal(rows(rank[f]), rows(dense_rank[df]))
