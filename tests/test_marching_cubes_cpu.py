"""Marching cubes without a GPU: the generated case table (scorp_amd/mc_table.py against its committed header and against the
properties any closed table must have), the float64 yardstick (tests/marching_cubes_reference.py) on fields whose surfaces are
known, and the numpy forms of scorp_amd.mesh.extract_surface / extract_surface_blocks against the yardstick: faces EQUAL,
positions within 1e-5 h - the bound the surface-nets tests use for the same t = (level - f0) / (f1 - f0), here with a single
crossing per vertex instead of a mean of up to twelve."""
import functools

import numpy as np
import pytest
import torch

from scorp_amd import mc_table
from tests import marching_cubes_reference as ref
from tests import tsdf_blocks_reference as blk


# ---- the table ----

def test_committed_header_is_the_generators_output():
    assert open(mc_table.HEADER, "rb").read() == mc_table.header_text().encode()


def test_table_counts():
    t = mc_table.table()
    assert t.shape == (256, 16) and t.dtype == np.uint8
    n = t[:, 15]
    assert int(n.sum()) == 820 and int(n.max()) == 5
    assert np.bincount(n, minlength=6).tolist() == [2, 16, 50, 80, 76, 32]
    assert max(len(l) for case in range(256) for l in mc_table.loops(case)) == 7
    for case in range(256):
        assert (t[case, :3 * n[case]] < 12).all() and (t[case, 3 * n[case]:15] == 0xFF).all()


def test_triangles_use_exactly_the_crossed_edges():
    t = mc_table.table()
    for case in range(256):
        used = set(t[case, :3 * t[case, 15]].tolist())
        assert used == set(mc_table.crossed_edges(case)), case


def test_fan_is_inadmissible_in_the_eighteen_listed_cases():
    bad = []
    for case in range(256):
        for l in mc_table.loops(case):
            if not mc_table._admissible(l, [(l[0], l[i], l[i + 1]) for i in range(1, len(l) - 1)]):
                bad.append(case)
    assert bad == [61, 62, 94, 123, 125, 173, 183, 188, 190, 203, 211, 215, 218, 222, 227, 229, 235, 237]


# ---- the yardstick on known surfaces ----

@functools.lru_cache(maxsize=None)
def reference(name, level=0.0):
    if name == "random":
        g, coords = ref.random_field()
        return ref.marching_cubes(g, coords)
    return ref.marching_cubes(ref.field(name), ref.lattice(), level=np.float32(level))


def test_random_field_has_every_case_and_a_closed_mesh():
    g, _ = ref.random_field()
    assert len(np.unique(ref.cell_cases(g))) == 256
    v, f = reference("random")
    assert ref.is_closed_and_oriented(f)
    inside = g < 0
    crossed = sum(int((inside.take(range(0, 23), a) != inside.take(range(1, 24), a)).sum()) for a in range(3))
    assert len(v) == crossed == 16700
    assert len(np.unique(f)) == len(v)


def test_sphere():
    coords = ref.lattice()
    h = ref.max_edge(coords)
    v, f = reference("sphere")
    assert ref.is_closed_and_oriented(f) and ref.euler_characteristic(v, f) == 2
    r = np.sqrt(((v - np.array([0.03, -0.02, 0.05])) ** 2).sum(1))
    assert np.abs(r - 0.7).max() < h
    vol = ref.signed_volume(v, f)
    assert 4 / 3 * np.pi * (0.7 - h) ** 3 < vol < 4 / 3 * np.pi * (0.7 + h) ** 3   # positive: the normals point outwards


def test_torus():
    v, f = reference("torus")
    assert ref.is_closed_and_oriented(f) and ref.euler_characteristic(v, f) == 0


def test_plane_is_open_with_normals_along_the_gradient():
    v, f = reference("plane")
    assert len(f) > 0 and not ref.is_closed_and_oriented(f)
    n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    area = np.linalg.norm(n, axis=1)
    keep = area > 1e-12
    g = np.array([0.3, 0.5, 0.8]) / np.linalg.norm([0.3, 0.5, 0.8])
    assert ((n[keep] / area[keep, None]) @ g > 0.99).all()
    e = ref.directed_edges(f)
    assert len({(a, b) for a, b in e}) == len(e)   # no directed edge twice: consistently oriented


def test_degenerate_grids():
    v, f = ref.marching_cubes(ref.field("none"), ref.lattice())
    assert v.shape == (0, 3) and f.shape == (0, 3)
    g = np.ones((2, 2, 2), np.float32)
    g[0, 0, 0] = -1.0
    c = np.array([0.0, 1.0], np.float32)
    v, f = ref.marching_cubes(g, (c, c, c))
    assert np.array_equal(v, 0.5 * np.eye(3)) and f.shape == (1, 3)
    n = np.cross(v[f[0, 1]] - v[f[0, 0]], v[f[0, 2]] - v[f[0, 0]])
    assert (n > 0).all()   # away from the inside corner at the origin


# ---- the CPU path of the package ----

def _extract(g, coords, level=0.0):
    from scorp_amd.mesh import extract_surface
    v, f = extract_surface(torch.from_numpy(g), [torch.from_numpy(np.asarray(c)) for c in coords], level=level, method="marching_cubes")
    assert v.dtype == torch.float32 and f.dtype == torch.int32
    return v.numpy(), f.numpy()


@pytest.mark.parametrize("name", ("sphere", "torus", "plane", "random"))
def test_cpu_path_matches_the_yardstick(name):
    g, coords = ref.random_field() if name == "random" else (ref.field(name), ref.lattice())
    v, f = _extract(g, coords)
    rv, rf = reference(name)
    assert v.shape == rv.shape and np.array_equal(f, rf)
    assert np.abs(v.astype(np.float64) - rv).max() <= 1e-5 * ref.max_edge(coords)


def test_cpu_path_nonzero_level_and_degenerate_grids():
    coords = ref.lattice()
    v, f = _extract(ref.field("sphere"), coords, level=0.1)
    rv, rf = reference("sphere", 0.1)
    assert np.array_equal(f, rf) and np.abs(v.astype(np.float64) - rv).max() <= 1e-5 * ref.max_edge(coords)
    v, f = _extract(ref.field("none"), coords)
    assert v.shape == (0, 3) and f.shape == (0, 3)
    g = np.ones((2, 2, 2), np.float32)
    g[0, 0, 0] = -1.0
    c = np.array([0.0, 1.0], np.float32)
    v, f = _extract(g, (c, c, c))
    assert np.array_equal(v, 0.5 * np.eye(3, dtype=np.float32)) and np.array_equal(f, [[0, 1, 2]])


def test_unknown_method_raises():
    from scorp_amd.mesh import BlockVolume, extract_surface, extract_surface_blocks
    c = torch.tensor([0.0, 1.0])
    with pytest.raises(ValueError):
        extract_surface(torch.ones(2, 2, 2), [c, c, c], method="dual_contouring")
    with pytest.raises(ValueError):
        extract_surface_blocks(BlockVolume(torch.empty(0, dtype=torch.int64), None, None, torch.empty(0, 4096), torch.empty(0, 4096), None,
                                           1.0), method="dual_contouring")


def test_default_method_is_unchanged():
    from scorp_amd.mesh import extract_surface
    g, coords = ref.field("sphere"), [torch.from_numpy(c) for c in ref.lattice()]
    a, b = extract_surface(torch.from_numpy(g), coords), extract_surface(torch.from_numpy(g), coords, method="surface_nets")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert a[0].shape[0] != _extract(g, ref.lattice())[0].shape[0]


# ---- blocks, CPU path ----

BLOCK_CASES = ("sphere_8_blocks", "sphere_hole", "sphere_unseen_layer", "plane_in_block_face", "single_block", "tilted_plane_3x1x1")


def _volume(blocks, vl):
    from scorp_amd.mesh import BlockVolume, block_coords
    keys, tsdf, w, col = (torch.from_numpy(a) for a in blk.volume_arrays(blocks))
    return BlockVolume(keys, block_coords(keys), None, tsdf, w, col, vl)


@pytest.mark.parametrize("name", BLOCK_CASES)
def test_blocks_cpu_path_matches_the_yardstick(name):
    from scorp_amd.mesh import extract_surface_blocks
    blocks, vl = blk.surface_cases()[name]
    rv, rf, rc = ref.marching_cubes_blocks(blocks, vl)
    m = extract_surface_blocks(_volume(blocks, vl), method="marching_cubes")
    v, f, c = m.vertices.numpy(), m.faces.numpy(), m.colors.numpy()
    assert len(v) == len(rv) > 0 and len(rf) > 0
    assert np.array_equal(f, rf)
    assert np.abs(v - rv).max() <= 1e-5 * vl + 2 * 2.0 ** -23 * np.abs(rv).max()
    assert np.abs(c - rc).max() <= 2.0 ** -20
    assert len(np.unique(f)) == len(v)
    closed = ref.is_closed_and_oriented(rf)
    assert closed == (name in ("sphere_8_blocks", "single_block"))


# ---- the extractor passes `method` through (CPU tensors, the stand-in render of tests/test_mesh_cpu.py) ----

@pytest.fixture(scope="module")
def extractor():
    from scorp_amd.mesh import GaussianExtractor
    from scorp_amd.synthetic import ring_cameras
    from tests.test_mesh_cpu import H, W, _fake_render, _Points
    d = np.random.default_rng(3).normal(size=(500, 3))
    xyz = torch.from_numpy((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32))
    ex = GaussianExtractor(_Points(xyz), _fake_render, pipe=None)
    ex.reconstruction(ring_cameras(6, W, H, 3, radius=4.0))
    return ex


def test_extractor_unbounded_passes_the_method_through(extractor):
    from scorp_amd.mesh import extract_surface
    grid, coords = extractor.tsdf_volume(20)
    v, f = extract_surface(grid, coords, method="marching_cubes")
    mesh = extractor.extract_mesh_unbounded(resolution=20, method="marching_cubes")
    assert len(v) > 0 and mesh.vertices.shape == v.shape and torch.equal(mesh.faces, f)
    assert mesh.colors.shape == v.shape and float(mesh.colors.min()) >= 0.0 and float(mesh.colors.max()) <= 1.0
    assert mesh.vertices.shape != extractor.extract_mesh_unbounded(resolution=20).vertices.shape
    with pytest.raises(ValueError):
        extractor.extract_mesh_unbounded(resolution=20, method="skimage")


def test_extractor_bounded_passes_the_method_through(extractor):
    from scorp_amd.mesh import extract_surface_blocks, tsdf_blocks_fuse
    kw = dict(voxel_size=0.1, sdf_trunc=0.4, depth_trunc=6)
    mesh = extractor.extract_mesh_bounded(method="marching_cubes", **kw)
    depth, rgb, world_to_cam, intrinsics = extractor.bounded_views(6)
    want = extract_surface_blocks(tsdf_blocks_fuse(depth, rgb, world_to_cam, intrinsics, 0.1, 0.4), method="marching_cubes")
    assert mesh.vertices.shape[0] > 0 and mesh.faces.shape[0] > 0
    assert torch.equal(mesh.vertices, want.vertices) and torch.equal(mesh.faces, want.faces) and torch.equal(mesh.colors, want.colors)
    f = mesh.faces.numpy()
    assert f.min() >= 0 and len(np.unique(f)) == mesh.vertices.shape[0]   # every vertex is used
    assert mesh.vertices.shape != extractor.extract_mesh_bounded(**kw).vertices.shape
    with pytest.raises(ValueError):
        extractor.extract_mesh_bounded(method="open3d", **kw)
