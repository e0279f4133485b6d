"""From a surfel model to a coloured triangle PLY through the public interface: about 2 000 opaque surfels on a unit sphere,
8 ring cameras at 96 x 80, GaussianExtractor.reconstruction -> extract_mesh_unbounded(resolution=48) -> write_mesh_ply ->
read back.  What a blurred render should give is fixed by nothing here, so the geometry is not asserted beyond its
soundness; the median vertex radius of the first run is recorded in DESIGN.md 4.12."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def sphere_surfels(n=2000):
    """Raw GaussianModel2D parameters: n surfels on a Fibonacci lattice of the unit sphere, normals radial, colour from the
    position (SH degree 0, inside [0.2, 0.8])."""
    k = np.arange(n) + 0.5
    phi, zc = math.pi * (1 + 5 ** 0.5) * k, 1 - 2 * k / n
    r = np.sqrt(1 - zc * zc)
    p = np.stack([r * np.cos(phi), r * np.sin(phi), zc], 1)
    q = np.stack([1 + p[:, 2], -p[:, 1], p[:, 0], np.zeros(n)], 1)      # (w, x, y, z): the rotation taking +z to p
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    dc = ((0.5 + 0.3 * p) - 0.5) / 0.28209479177387814
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    return dict(xyz=f32(p), scaling=f32(np.full((n, 2), math.log(0.06))), rotation=f32(q), opacity=f32(np.full((n, 1), 6.0)),
                features_dc=f32(dc[:, None, :]), features_rest=np.zeros((n, 0, 3), np.float32))


def test_surfel_sphere_to_coloured_ply(tmp_path):
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    from scorp_amd.mesh import GaussianExtractor, Mesh
    from scorp_amd.ply import read_mesh_ply, write_mesh_ply
    from scorp_amd.renderer2d import GaussianModel2D, render
    from scorp_amd.synthetic import ring_cameras
    from scorp_amd.train import PipelineParams
    model = GaussianModel2D.from_raw(sphere_surfels(), 0, device=dev)
    model.active_sh_degree = 0
    pipe = PipelineParams()
    pipe.depth_ratio = 0.0
    ex = GaussianExtractor(model, render, pipe)
    cams = ring_cameras(8, 96, 80, 3, radius=4.0, device=dev)
    ex.reconstruction(cams)
    assert ex.depthmaps.shape == (8, 80, 96) and ex.rgbmaps.shape == (8, 3, 80, 96) and ex.depthmaps.is_cuda
    assert 3.0 < ex.radius < 5.0 and float(ex.center.norm()) < 1.0
    mesh = ex.extract_mesh_unbounded(resolution=48)
    assert isinstance(mesh, Mesh)
    v, f, c = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy(), mesh.colors.cpu().numpy()
    print(f"mesh: {len(v)} vertices, {len(f)} faces, median vertex radius {np.median(np.linalg.norm(v, axis=1)):.4f}")
    assert len(v) > 0 and len(f) > 0 and c.shape == v.shape
    assert np.isfinite(v).all() and np.isfinite(c).all()
    assert f.min() >= 0 and f.max() < len(v)
    assert c.min() >= 0.0 and c.max() <= 1.0
    path = str(tmp_path / "mesh.ply")
    write_mesh_ply(path, mesh)
    rv, rf, rc = read_mesh_ply(path)
    assert np.array_equal(rv, v) and np.array_equal(rf, f)
    assert np.array_equal(rc, np.rint(c.astype(np.float64) * 255).astype(np.uint8))


def test_views_of_different_resolution_are_refused():
    dev = torch.device("cuda:0")
    from scorp_amd.mesh import GaussianExtractor
    from scorp_amd.renderer2d import GaussianModel2D, render
    from scorp_amd.synthetic import ring_cameras
    from scorp_amd.train import PipelineParams
    model = GaussianModel2D.from_raw(sphere_surfels(200), 0, device=dev)
    model.active_sh_degree = 0
    ex = GaussianExtractor(model, render, PipelineParams())
    cams = ring_cameras(2, 96, 80, 3, device=dev)[:1] + ring_cameras(2, 64, 80, 3, device=dev)[1:]
    with pytest.raises(ValueError, match="one resolution"):
        ex.reconstruction(cams)
