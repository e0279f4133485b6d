"""scorp_amd.mesh without a GPU: GaussianExtractor over a stand-in render() (the analytic depth maps of
tests/tsdf_reference.py on CPU tensors) - the bounding sphere, the CPU route to a mesh, export_image - and the grid-size
bound of the surface-extraction entry points."""
import math
import os

import numpy as np
import pytest
import torch

from tests import tsdf_reference as ref

W, H = 40, 32


class _Points:
    """What the extractor reads of a model: get_xyz."""
    def __init__(self, xyz):
        self.get_xyz = xyz


def _fake_render(cam, gaussians, pipe, bg_color):
    depth = torch.from_numpy(ref.raycast_depth(cam, size=(W, H)))[None]
    u, v = torch.meshgrid(torch.linspace(0, 1, W), torch.linspace(0, 1, H), indexing="xy")
    return {"render": torch.stack([u, v, torch.full_like(u, 0.25 + 0.1 * cam.uid)]), "render_depth": depth}


@pytest.fixture(scope="module")
def extractor():
    from scorp_amd.mesh import GaussianExtractor
    from scorp_amd.synthetic import ring_cameras
    d = np.random.default_rng(3).normal(size=(500, 3))
    xyz = torch.from_numpy((d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32))
    ex = GaussianExtractor(_Points(xyz), _fake_render, pipe=None)
    cams = ring_cameras(6, W, H, 3, radius=4.0)
    for cam in cams[:2]:
        cam.original_image = torch.full((3, H, W), 0.5)
    ex.reconstruction(cams)
    return ex


def test_bounding_sphere_of_a_camera_ring(extractor):
    from scorp_amd.mesh import focus_point
    # every camera looks at the origin: the focus point is the origin, the radius the nearest camera's distance
    assert float(extractor.center.norm()) < 1e-5
    eyes = np.stack([c.camera_center.numpy() for c in extractor.viewpoint_stack])
    assert abs(extractor.radius - np.linalg.norm(eyes, axis=1).min()) < 1e-5
    # two rays that cross at (1, 2, 3); lengths and signs of the directions do not matter
    c = focus_point(np.array([[0.0, 2.0, 3.0], [1.0, 2.0, -4.0]]), np.array([[-5.0, 0.0, 0.0], [0.0, 0.0, 0.1]]))
    assert np.allclose(c, [1.0, 2.0, 3.0], atol=1e-12)


def test_cpu_route_to_a_coloured_mesh(extractor, tmp_path):
    from scorp_amd.ply import read_mesh_ply, write_mesh_ply
    assert extractor.depthmaps.shape == (6, H, W) and extractor.rgbmaps.shape == (6, 3, H, W)
    grid, coords = extractor.tsdf_volume(20)
    assert grid.shape == (20, 20, 20) and float(grid.min()) < 0 < float(grid.max())
    mesh = extractor.extract_mesh_unbounded(resolution=20)
    v, f, c = mesh.vertices.numpy(), mesh.faces.numpy(), mesh.colors.numpy()
    assert len(v) > 0 and len(f) > 0 and np.isfinite(v).all() and f.min() >= 0 and f.max() < len(v)
    assert c.min() >= 0.0 and c.max() <= 1.0
    path = str(tmp_path / "m.ply")
    write_mesh_ply(path, mesh)
    rv, rf, rc = read_mesh_ply(path)
    assert np.array_equal(rv, v) and np.array_equal(rf, f)
    assert np.array_equal(rc, np.rint(c.astype(np.float64) * 255).astype(np.uint8))


def test_export_image_writes_renders_depths_and_ground_truth(extractor, tmp_path):
    from PIL import Image
    extractor.export_image(str(tmp_path))
    assert sorted(os.listdir(tmp_path / "renders")) == [f"{i:05d}.png" for i in range(6)]
    assert sorted(os.listdir(tmp_path / "vis")) == [f"depth_{i:05d}.tiff" for i in range(6)]
    assert sorted(os.listdir(tmp_path / "gt")) == ["00000.png", "00001.png"]   # only the cameras that carry an image
    png = np.asarray(Image.open(tmp_path / "renders" / "00003.png"))
    want = (np.clip(extractor.rgbmaps[3].permute(1, 2, 0).numpy(), 0, 1) * 255).astype(np.uint8)
    assert png.shape == (H, W, 3) and np.array_equal(png, want)
    depth = np.asarray(Image.open(tmp_path / "vis" / "depth_00003.tiff"))
    assert depth.dtype == np.float32 and np.array_equal(depth, extractor.depthmaps[3].numpy())
    assert np.array_equal(np.asarray(Image.open(tmp_path / "gt" / "00001.png")), np.full((H, W, 3), 127, np.uint8))


def test_views_of_different_resolution_are_refused():
    from scorp_amd.mesh import GaussianExtractor
    from scorp_amd.synthetic import ring_cameras
    sizes = iter([(W, H), (W, H + 2)])

    def render(cam, g, pipe, bg_color):
        w, h = next(sizes)
        return {"render": torch.zeros(3, h, w), "render_depth": torch.ones(1, h, w)}
    ex = GaussianExtractor(_Points(torch.zeros(4, 3)), render, pipe=None)
    with pytest.raises(ValueError, match="one resolution"):
        ex.reconstruction(ring_cameras(2, W, H, 3))
    with pytest.raises(RuntimeError, match="reconstruction"):
        GaussianExtractor(_Points(torch.zeros(4, 3)), render, pipe=None).tsdf_volume(8)


def test_isosurface_entry_points_refuse_bad_grids():
    """Validation runs before any HIP call: the dummy pointers are never dereferenced, no GPU is needed."""
    from scorp_amd import _C
    L = _C.lib()
    d = 0x10000
    big = 1 << 14   # 2^42 lattice points: more than (2^31 - 1) * 256
    for dims, text in (((1, 4, 4), b"at least 2"), ((big, big, big), b"lattice points")):
        assert L.scorp_isosurface_count_cells(d, *dims, 0.0, d, None) == _C.ERR_INVALID and text in L.scorp_last_error()
        assert L.scorp_isosurface_count_faces(d, *dims, 0.0, d, None) == _C.ERR_INVALID and text in L.scorp_last_error()
        assert L.scorp_isosurface_emit_vertices(d, d, d, d, *dims, 0.0, d, 1, d, None) == _C.ERR_INVALID
        assert L.scorp_isosurface_emit_faces(d, *dims, 0.0, d, d, 1, d, None) == _C.ERR_INVALID
    assert L.scorp_isosurface_count_cells(None, 4, 4, 4, 0.0, d, None) == _C.ERR_INVALID
    assert L.scorp_isosurface_emit_faces(d, 4, 4, 4, 0.0, d, d, 0, d, None) == _C.ERR_INVALID
    assert b"num_quads" in L.scorp_last_error()
