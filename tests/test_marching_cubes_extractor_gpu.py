"""GaussianExtractor with method="marching_cubes" end to end on the scene of tests/test_mesh_gpu.py (about 2 000 opaque surfels
on a unit sphere, 8 ring cameras at 96 x 80): both routes return the mesh that the free functions give on the same volume, every
face index is a vertex, every vertex of the bounded mesh is used, and no mesh edge carries more than two triangles."""
import numpy as np
import pytest
import torch

from tests.test_mesh_gpu import sphere_surfels

pytestmark = pytest.mark.gpu

VOXEL, TRUNC, DEPTH_TRUNC = 0.05, 0.2, 6


@pytest.fixture(scope="module")
def extractor():
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    from scorp_amd.mesh import GaussianExtractor
    from scorp_amd.renderer2d import GaussianModel2D, render
    from scorp_amd.synthetic import ring_cameras
    from scorp_amd.train import PipelineParams
    model = GaussianModel2D.from_raw(sphere_surfels(), 0, device=dev)
    model.active_sh_degree = 0
    pipe = PipelineParams()
    pipe.depth_ratio = 0.0
    ex = GaussianExtractor(model, render, pipe)
    ex.reconstruction(ring_cameras(8, 96, 80, 3, radius=4.0, device=dev))
    return ex


def _edge_multiplicity(f):
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    return np.unique(e, axis=0, return_counts=True)[1]


def test_unbounded_route(extractor):
    from scorp_amd.mesh import Mesh, extract_surface, post_process_mesh
    mesh = extractor.extract_mesh_unbounded(resolution=48, method="marching_cubes")
    assert isinstance(mesh, Mesh) and mesh.vertices.is_cuda
    grid, coords = extractor.tsdf_volume(48)
    v, f = extract_surface(grid, coords, method="marching_cubes")
    assert v.shape[0] > 0 and mesh.vertices.shape == v.shape and torch.equal(mesh.faces, f)
    assert bool(torch.isfinite(mesh.vertices).all()) and mesh.colors.shape == v.shape
    assert float(mesh.colors.min()) >= 0.0 and float(mesh.colors.max()) <= 1.0
    fn = f.cpu().numpy()
    assert fn.min() >= 0 and fn.max() < v.shape[0] and _edge_multiplicity(fn).max() <= 2
    cleaned = post_process_mesh(mesh, cluster_to_keep=1)
    assert 0 < cleaned.faces.shape[0] <= f.shape[0]
    with pytest.raises(ValueError):
        extractor.extract_mesh_unbounded(resolution=48, method="skimage")


def test_bounded_route(extractor):
    from scorp_amd.mesh import Mesh, extract_surface_blocks, tsdf_blocks_fuse
    mesh = extractor.extract_mesh_bounded(voxel_size=VOXEL, sdf_trunc=TRUNC, depth_trunc=DEPTH_TRUNC, method="marching_cubes")
    assert isinstance(mesh, Mesh) and mesh.vertices.is_cuda
    depth, rgb, world_to_cam, intrinsics = extractor.bounded_views(DEPTH_TRUNC)
    want = extract_surface_blocks(tsdf_blocks_fuse(depth, rgb, world_to_cam, intrinsics, VOXEL, TRUNC), method="marching_cubes")
    assert mesh.vertices.shape[0] > 0 and mesh.faces.shape[0] > 0
    assert torch.equal(mesh.vertices, want.vertices) and torch.equal(mesh.faces, want.faces) and torch.equal(mesh.colors, want.colors)
    f = mesh.faces.cpu().numpy()
    assert f.min() >= 0 and len(np.unique(f)) == mesh.vertices.shape[0]   # every vertex is used
    assert _edge_multiplicity(f).max() <= 2
    assert float(mesh.colors.min()) >= 0.0 and float(mesh.colors.max()) <= 1.0
    with pytest.raises(ValueError):
        extractor.extract_mesh_bounded(voxel_size=VOXEL, sdf_trunc=TRUNC, depth_trunc=DEPTH_TRUNC, method="open3d")
